"""GGUF on the GPU: eggroll_gguf_dequant against the packer + closed-form values of tests/gguf_pack.py, bit for
bit in fp32 and in bf16 (the RNE rounding of that value), with sentinels after the output; a model saved as
GGUF loaded on the GPU against the CPU-path load of the same file; and a backend built from a mixed-type GGUF
file against one built from the safetensors directory of the same weights, image for image.

The end-to-end architecture is the smallest one a diffusers config.json can describe whose inner dimensions
are all multiples of the 256-element K blocks: dim 768 (ffn = int(dim / 3 * 8) = 2048), and 128 px, because a
config-built architecture carries the fixed seq_multiple 32 and 64 px would give 16 image tokens."""
import json

import numpy as np
import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import checkpoints as ck
from hyperscalees_t2i_amd import gguf as G
from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd.backend import ZImageBackend, ZImageConfig
from hyperscalees_t2i_amd.es import EggRollNoiser, flatten_params
from hyperscalees_t2i_amd.flux_vae import FluxVAEDecoder
from hyperscalees_t2i_amd.zimage import ZImageArch, ZImageTransformer2DModel
from tests import gguf_pack as P

pytestmark = pytest.mark.gpu
TINY = ZImageArch(dim=256, n_layers=2, n_refiner_layers=1, n_heads=2, ffn=512, cap_feat_dim=256, t_mid=256,
                  seq_multiple=16)
E2E = ZImageArch(dim=768, n_layers=2, n_refiner_layers=1, n_heads=6, ffn=2048, cap_feat_dim=256, t_mid=1024)
SENTINEL = 64
IDS = [G.type_name(t) for t in P.QUANT_TYPES]


def _blocks(t, which):
    """1, 7, 1031 (a prime: the last workgroup's span is short) blocks, and three rows of 10240 elements."""
    return {"1": 1, "7": 7, "1031": 1031, "3x10240": 3 * 10240 // G.GGML_TYPES[t][1]}[which]


def _run(dev, raw_dev, t, n, fp32):
    """The C entry point on an output buffer with SENTINEL elements after the end."""
    dt = torch.float32 if fp32 else torch.bfloat16
    out = torch.full((n + SENTINEL,), -7.0, dtype=dt, device=dev)
    _lib.call("eggroll_gguf_dequant", t, raw_dev.data_ptr(), n, out.data_ptr(), int(fp32),
              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out[n:] == -7.0).all()), "wrote past n_elems"
    return out[:n].cpu()


@pytest.mark.parametrize("which", ["1", "7", "1031", "3x10240"])
@pytest.mark.parametrize("t", P.QUANT_TYPES, ids=IDS)
def test_kernel_is_exact(dev, t, which):
    nb = _blocks(t, which)
    n = P.n_elems(t, nb)
    raw, want = P.case(t, nb, seed=77 * t + nb)
    want = torch.from_numpy(want)
    raw_dev = torch.from_numpy(raw).to(dev)                     # byte 0 of its own allocation
    assert raw_dev.data_ptr() % 256 == 0 and raw_dev.numel() == nb * G.GGML_TYPES[t][2]
    assert torch.equal(_run(dev, raw_dev, t, n, True), want)
    assert torch.equal(_run(dev, raw_dev, t, n, False), want.to(torch.bfloat16))
    # the wrapper (its own output allocation) and the torch front end
    assert torch.equal(K.gguf_dequant(raw_dev, t, n, torch.float32).cpu(), want)
    assert torch.equal(G.dequantize(raw, t, (n,), dev).cpu(), want.to(torch.bfloat16))


@pytest.mark.parametrize("t", P.QUANT_TYPES, ids=IDS)
def test_kernel_is_exact_from_a_2_byte_aligned_base(dev, t):
    """Blocks that start 2 bytes into an allocation (not 16-byte aligned) take the narrow staging path."""
    nb = 1031
    n = P.n_elems(t, nb)
    raw, want = P.case(t, nb, seed=5 * t + 1)
    buf = torch.zeros(raw.size + 2, dtype=torch.uint8, device=dev)
    buf[2:] = torch.from_numpy(raw).to(dev)
    assert buf[2:].data_ptr() % 16 == 2
    assert torch.equal(_run(dev, buf[2:], t, n, True), torch.from_numpy(want))
    assert torch.equal(_run(dev, buf[2:], t, n, False), torch.from_numpy(want).to(torch.bfloat16))


def test_wrapper_checks(dev):
    raw = torch.zeros(144, dtype=torch.uint8, device=dev)
    assert K.gguf_dequant(raw, G.Q4_K, 256).dtype == torch.bfloat16
    assert K.gguf_dequant(raw[:0], G.Q4_K, 0).numel() == 0
    with pytest.raises(ValueError):
        K.gguf_dequant(raw, G.Q4_K, 512)                        # byte count
    with pytest.raises(ValueError):
        K.gguf_dequant(raw, G.F16, 72)                          # not a block type of the kernel
    with pytest.raises(ValueError):
        K.gguf_dequant(raw, G.Q4_K, 256, torch.float16)
    with pytest.raises(_lib.EggrollError):
        K.gguf_dequant(raw.cpu(), G.Q4_K, 256)
    with pytest.raises(_lib.EggrollError):
        K.gguf_dequant(raw.to(torch.int8), G.Q4_K, 256)


def test_model_load_gpu_equals_cpu(dev, tmp_path):
    src = ZImageTransformer2DModel(TINY)
    src.init_weights(3)
    for single in (False, True):
        p = tmp_path / f"m{int(single)}.gguf"
        ck.save_zimage_gguf(src, p, single_file_names=single)
        on_cpu, on_gpu = ZImageTransformer2DModel(TINY), ZImageTransformer2DModel(TINY).to(dev)
        ck.load_zimage_transformer_gguf(on_cpu, p)
        ck.load_zimage_transformer_gguf(on_gpu, p)
        for (n, a), (_, b) in zip(on_cpu.named_parameters(), on_gpu.named_parameters()):
            assert b.device.type == "cuda" and torch.equal(a, b.cpu()), n
    state = ck.read_gguf_state(p, dev)
    assert all(v.device.type == "cuda" for v in state.values())
    assert {v.dtype for v in state.values()} == {torch.bfloat16, torch.float32}


def _mixed_type(name: str) -> int:
    if name.endswith((".feed_forward.w1.weight", ".feed_forward.w3.weight")):
        return G.Q4_K
    if name.endswith(".feed_forward.w2.weight"):
        return G.Q3_K
    if name.endswith((".attention.to_q.weight", ".attention.to_k.weight", ".attention.to_v.weight")):
        return G.Q6_K
    if name.endswith(".attention.to_out.0.weight"):
        return G.Q5_K
    if "adaLN_modulation" in name and name.endswith(".weight"):
        return G.Q2_K
    if name.startswith("all_x_embedder.") and name.endswith(".weight"):
        return G.Q8_0
    return G.F32


def test_backend_from_mixed_gguf_matches_safetensors(dev, tmp_path):
    src = ZImageTransformer2DModel(E2E).to(dev)
    src.init_weights(11)
    vae = FluxVAEDecoder(widths=(32, 32, 64, 64)).to(dev)
    vae.init_weights(13)
    root = tmp_path / "model"
    (root / "transformer").mkdir(parents=True)
    (root / "transformer" / "config.json").write_text(json.dumps(ck.zimage_config_from_arch(E2E)))
    ck.write_state_dir(root / "vae", ck.state_from_build(vae, ck.flux_vae_rules(vae)), ck.flux_vae_config_from_build(vae))
    rng = np.random.default_rng(17)
    tensors, used = {}, set()
    for name, w in ck.state_from_build(src, ck.zimage_rules(src)).items():
        t = _mixed_type(name)
        used.add(t)
        if t == G.F32:
            tensors[name] = (t, tuple(w.shape), w.float().cpu().contiguous().numpy().reshape(-1).view(np.uint8))
        else:
            assert w.dim() == 2 and w.shape[1] % G.GGML_TYPES[t][1] == 0, name
            f = P.random_fields(t, w.numel() // G.GGML_TYPES[t][1], rng, half_values=[0.0123, -0.0123])
            tensors[name] = (t, tuple(w.shape), P.pack(t, f))
    assert used == {G.Q4_K, G.Q3_K, G.Q6_K, G.Q5_K, G.Q2_K, G.Q8_0, G.F32}
    G.write_gguf(tmp_path / "mixed.gguf", tensors)
    del src

    kw = dict(width_px=128, height_px=128, num_inference_steps=2, batches_per_gen=2, synthetic_prompt_lens=(20, 70))
    a = ZImageBackend(str(dev), ZImageConfig(model_name=str(root), use_gguf=True,
                                             gguf_local_path=str(tmp_path / "mixed.gguf"), **kw))
    a.init_and_attach_lora()
    assert "Q4_K×" in a.es_model.weights_source and "Q2_K×" in a.es_model.weights_source
    ck.save_zimage_diffusers(a.es_model.transformer, a.es_model.vae, tmp_path / "st")
    b = ZImageBackend(str(dev), ZImageConfig(model_name=str(tmp_path / "st"), **kw))
    b.init_and_attach_lora()
    fa = {n: p for n, p in a.es_model.transformer.named_parameters() if not p.requires_grad}
    fb = {n: p for n, p in b.es_model.transformer.named_parameters() if not p.requires_grad}
    assert set(fa) == set(fb)
    for n in fa:
        assert torch.equal(fa[n], fb[n]), n
    # wiring: one Q6_K weight is the CPU dequantisation of the bytes that were written
    gt, shape, raw = tensors["layers.0.attention.to_q.weight"]
    want = torch.from_numpy(G.dequantize_numpy(raw, gt, int(np.prod(shape)))).to(torch.bfloat16).reshape(shape)
    assert torch.equal(fa["layers.0.attention.to_q.weight"].cpu(), want)
    pa, sa = a.collect_lora_params()
    pb, sb = b.collect_lora_params()
    assert sa == sb
    theta = flatten_params(pa).to(dev)
    noiser = EggRollNoiser(sa, sigma=5e-2, lr_scale=0.1, rank=4, use_antithetic=True)
    tp = noiser.perturb(theta, noiser.epoch_noise(2, seed=1), 2, 0, 2)
    flat = a.step_sampling_info(1)["flat_ids"]
    ia, ib = a.generate_population(flat, 1, 0.0, tp), b.generate_population(flat, 1, 0.0, tp)
    assert bool(torch.isfinite(ia.float()).all())
    assert torch.equal(ia, ib)
