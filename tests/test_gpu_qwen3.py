"""Qwen3 prompt encoder on the GPU: eggroll_causal_attention against an fp32 torch restatement of transformers'
eager attention, eggroll_qk_norm_rope_half against Qwen3RMSNorm + rotate_half in fp32, the encoder against
transformers' Qwen3Model (fp32 eager oracle `hidden_states[-2]`, the same model in bf16 as the yardstick), and
the prompt .txt -> encoded file -> Z-Image population pass path end to end.

Kernel bars (the ones tests/test_gpu_t5.py and tests/test_gpu_gemma2.py hold their attention kernels to): on
valid rows relative error < 1e-2 and max |d| < 3e-2 max|ref| (P is rounded to bf16 before the PV MFMA, the
output is bf16); rows >= len exactly zero.  Norm + rotation: one bf16 rounding, 2^-8.

Encoder bar: per prompt, our relative Frobenius error against the fp32 oracle over the valid rows is at most
1.5x the error of the reference model itself run in bf16 on the same GPU and inputs (the margin of
tests/test_gpu_gemma2.py: our GEMM outputs and P are bf16, the stream is fp32).  Negative controls that must
exceed the bar at every length: the encoder run through all L layers, and the q / k norm weights forced to 1.

Measured on an MI355X (profiles/qwen3_pytest_gpu.log, profiles/qwen3_encoder_vs_transformers.json): the kernel
1.7e-3 to 1.9e-3 relative, max |d| at most 7.9e-3 against max|ref| of 2.9 or more; norm + rotation max |d| 1.5e-2
against the bar 2.2e-2, relative 1.6e-3, 0.43 with wq and wk swapped; the encoder at lengths 5 / 40 / 130: ours
7.8e-3 / 9.1e-3 / 1.07e-2, the bf16 reference 1.03e-2 / 1.29e-2 / 1.68e-2, all layers 0.72 / 0.86 / 1.00, q / k norm
weights 1: 0.17 / 0.39 / 0.45; 4 query heads on one KV head, lengths 7 / 33: ours 6.7e-3 / 9.6e-3, the bf16
reference 8.4e-3 / 1.25e-2.
"""
import copy

import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import checkpoints as ck
from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd.backend import ZImageBackend, ZImageConfig
from hyperscalees_t2i_amd.es import EggRollNoiser, flatten_params
from hyperscalees_t2i_amd.qwen3 import rope_tables
from hyperscalees_t2i_amd.zimage import ZImageArch
from hyperscalees_t2i_amd.zimage_pipeline import ZImageTurboES
from tests.qwen3_tiny import LENS, export_dir, hf_config, hf_state, make_tokenizer, padded_ids, rel_err, tiny_hf_model

pytestmark = pytest.mark.gpu
HD = 128
SCALE = HD ** -0.5


# ---- kernel ------------------------------------------------------------------------------------
def _inputs(dev, B, N, Hq, Hkv, sliced, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    if sliced:   # q / k / v as column slices of one [B*N, (Hq + 2 Hkv)*128] tensor (the fused qkv GEMM's output)
        qkv = torch.randn((B * N, (Hq + 2 * Hkv) * HD), generator=g, device=dev).to(torch.bfloat16)
        return qkv[:, :Hq * HD], qkv[:, Hq * HD:(Hq + Hkv) * HD], qkv[:, (Hq + Hkv) * HD:]
    return [torch.randn((B * N, h * HD), generator=g, device=dev).to(torch.bfloat16) for h in (Hq, Hkv, Hkv)]


def _eager_ref(q, k, v, lens, B, N, Hq, Hkv, scale):
    """Qwen3's eager_attention_forward in fp32: repeat_kv, scale, the causal + key-padding mask, softmax, PV."""
    t = lambda x, h: x.reshape(B, N, h, HD).transpose(1, 2).float()  # noqa: E731
    qq, kk, vv = t(q, Hq), t(k, Hkv).repeat_interleave(Hq // Hkv, 1), t(v, Hkv).repeat_interleave(Hq // Hkv, 1)
    s = qq @ kk.transpose(-1, -2) * scale
    i, j = torch.arange(N, device=q.device)[:, None], torch.arange(N, device=q.device)[None, :]
    keep = (j <= i)[None, None] & (j[None, None] < torch.tensor(lens, device=q.device).view(B, 1, 1, 1))
    p = torch.softmax(s.masked_fill(~keep, float("-inf")), -1)
    return (p @ vv).transpose(1, 2).reshape(B * N, Hq * HD)


@pytest.mark.parametrize("B,N,Hq,Hkv,lens,sliced", [
    (3, 37, 4, 2, [37, 1, 20], False),
    (2, 64, 2, 2, [64, 16], False),
    (2, 65, 8, 2, [65, 33], True),                 # two key blocks, G = 4, qkv read in place
    (1, 1, 2, 1, [1], False),
    (1, 129, 4, 4, [129], False),                  # three key blocks, a one-row last query block
    (2, 300, 8, 2, [129, 299], True),
    (1, 130, 3, 1, [130], False),                  # G = 3
])
def test_causal_attention_vs_eager(dev, B, N, Hq, Hkv, lens, sliced):
    q, k, v = _inputs(dev, B, N, Hq, Hkv, sliced, seed=N * 7 + B)
    ours = K.causal_attention(q, k, v, torch.tensor(lens), B, N, Hq, Hkv, SCALE).float()
    ref = _eager_ref(q, k, v, lens, B, N, Hq, Hkv, SCALE)
    valid = torch.zeros(B, N, dtype=torch.bool, device=dev)
    for b, L in enumerate(lens):
        valid[b, :L] = True
    valid = valid.view(-1)
    o, r = ours[valid], ref[valid]
    rel, mx = rel_err(o, r), float((o - r).abs().max())
    print(f"causal_attention B{B} N{N} H{Hq}/{Hkv} lens{lens}: rel {rel:.3e} max|d| {mx:.3e} "
          f"max|ref| {float(r.abs().max()):.3e}")
    assert rel < 1e-2, rel     # bf16 P (probabilities rounded before the PV MFMA) + bf16 output
    assert mx < 3e-2 * float(r.abs().max())
    assert not ours[~valid].any()                  # query rows >= len[b]: exactly zero


@pytest.mark.parametrize("i0", [62, 63, 64])
def test_causal_attention_causality_bitwise(dev, i0):
    """Keys and values after row i0 do not reach rows <= i0: not one bit (i0 on both sides of a key-block edge)."""
    B, N, Hq, Hkv = 2, 130, 4, 2
    q, k, v = _inputs(dev, B, N, Hq, Hkv, False, seed=11)
    lens = torch.tensor([N, N])
    before = K.causal_attention(q, k, v, lens, B, N, Hq, Hkv, SCALE)
    k2, v2 = k.clone(), v.clone()
    g = torch.Generator(device=dev).manual_seed(12)
    junk = lambda t: (torch.randn(t.shape, generator=g, device=dev) * 300.0).to(torch.bfloat16)  # noqa: E731
    k2[N + i0 + 1:2 * N] = junk(k2[N + i0 + 1:2 * N])      # sequence 1, rows j > i0
    v2[N + i0 + 1:2 * N] = junk(v2[N + i0 + 1:2 * N])
    after = K.causal_attention(q, k2, v2, lens, B, N, Hq, Hkv, SCALE)
    assert torch.equal(after[:N + i0 + 1], before[:N + i0 + 1])
    assert not torch.equal(after[N + i0 + 1:], before[N + i0 + 1:])      # the later rows do see them
    assert bool(torch.isfinite(after.float()).all())


def test_causal_attention_batch_independence_bitwise(dev):
    B, N, Hq, Hkv, lens = 3, 100, 4, 2, [100, 7, 64]
    q, k, v = _inputs(dev, B, N, Hq, Hkv, True, seed=5)
    full = K.causal_attention(q, k, v, torch.tensor(lens), B, N, Hq, Hkv, SCALE)
    for b in range(B):
        s = slice(b * N, (b + 1) * N)
        one = K.causal_attention(q[s], k[s], v[s], torch.tensor(lens[b:b + 1]), 1, N, Hq, Hkv, SCALE)
        assert torch.equal(full[s], one), b


def test_causal_attention_lens_edges_and_host_checks(dev):
    """len 0: the whole sequence is zeros (no NaN); a device-resident lens outside [0, N] is clamped in the
    kernel; a CPU-resident one is refused on the host, like shapes outside the kernel's limits."""
    B, N, Hq, Hkv = 3, 20, 2, 1
    q, k, v = _inputs(dev, B, N, Hq, Hkv, False, seed=9)
    out = K.causal_attention(q, k, v, torch.tensor([0, 20, 3]), B, N, Hq, Hkv, SCALE, out=torch.full(
        (B * N, Hq * HD), float("nan"), dtype=torch.bfloat16, device=dev))
    assert not out[:N].any() and not out[2 * N + 3:].any() and bool(torch.isfinite(out.float()).all())
    assert bool(out[N:2 * N].any())
    clamped = K.causal_attention(q, k, v, torch.tensor([-4, 99, 3], device=dev), B, N, Hq, Hkv, SCALE)
    assert torch.equal(clamped, out)
    with pytest.raises(ValueError):
        K.causal_attention(q, k, v, torch.tensor([0, 21, 3]), B, N, Hq, Hkv, SCALE)
    with pytest.raises(ValueError):
        K.causal_attention(q, k, v, torch.tensor([-1, 20, 3]), B, N, Hq, Hkv, SCALE)
    with pytest.raises(ValueError):
        K.causal_attention(q, k, v, torch.tensor([0, 20, 3]), B, N, 3, 2, SCALE)           # Hq % Hkv != 0
    with pytest.raises(ValueError):
        K.causal_attention(q, k, v, torch.tensor([0, 20, 3]), B, N, Hq, Hkv, SCALE, head_dim=256)
    with pytest.raises(_lib.EggrollError):
        K.causal_attention(q.float(), k, v, torch.tensor([0, 20, 3]), B, N, Hq, Hkv, SCALE)


def test_qk_norm_rope_half_vs_fp32(dev):
    """In place on the q | k heads of a strided view with an 8-column offset (a fused qkv tensor with one head
    of v after them): Qwen3RMSNorm over head_dim with wq / wk, then transformers' rotate_half expression, all in
    fp32, rounded once; the v columns and the offset columns are untouched."""
    B, N, Hq, Hkv, extra, eps = 2, 37, 3, 2, 1, 1e-6
    heads = Hq + Hkv
    g = torch.Generator(device=dev).manual_seed(3)
    big = torch.randn((B * N, 8 + (heads + extra) * HD), generator=g, device=dev).to(torch.bfloat16)
    wq = 1.0 + 0.3 * torch.randn(HD, generator=g, device=dev)
    wk = 1.0 + 0.3 * torch.randn(HD, generator=g, device=dev)
    cos, sin = (t.to(dev) for t in rope_tables(N))

    def reference(w_q, w_k):
        xv = big[:, 8:8 + heads * HD].reshape(B, N, heads, HD).float()
        w = torch.cat([w_q.expand(Hq, HD), w_k.expand(Hkv, HD)])[None, None]
        y = xv * torch.rsqrt(xv.pow(2).mean(-1, keepdim=True) + eps) * w
        c, s = torch.cat([cos, cos], -1)[None, :, None, :], torch.cat([sin, sin], -1)[None, :, None, :]
        rot = torch.cat([-y[..., HD // 2:], y[..., :HD // 2]], -1)
        return (y * c + rot * s).reshape(B * N, heads * HD), y.reshape(B * N, heads * HD)
    ref, normed = reference(wq, wk)
    swapped, _ = reference(wk, wq)
    before = big.clone()
    x = big[:, 8:]                                      # row stride 8 + 6*128, 16-byte aligned start
    K.qk_norm_rope_half_(x, wq, wk, eps, cos, sin, B, N, Hq, Hkv)
    got = x[:, :heads * HD].float()
    mx, rel = float((got - ref).abs().max()), rel_err(got, ref)
    print(f"qk_norm_rope_half: max|d| {mx:.3e} (bar {2.0 ** -8 * float(ref.abs().max()):.3e}) rel {rel:.3e}; "
          f"against wq / wk swapped: rel {rel_err(got, swapped):.3e}")
    assert mx <= 2.0 ** -8 * float(ref.abs().max())     # one bf16 rounding
    assert rel < 2.0 ** -8
    assert torch.equal(big[:, :8], before[:, :8]) and torch.equal(x[:, heads * HD:], before[:, 8 + heads * HD:])
    assert float((got[0] - normed[0]).abs().max()) <= 2.0 ** -8 * float(normed[0].abs().max())   # position 0: the norm
    assert not torch.equal(got[0], before[0, 8:8 + heads * HD].float())
    # wq != wk is visible: the same output against the reference with the two swapped misses the bar
    assert rel_err(got, swapped) > 2.0 ** -8 and float((got - swapped).abs().max()) > 2.0 ** -8 * float(swapped.abs().max())
    with pytest.raises(ValueError):
        K.qk_norm_rope_half_(x, wq, wk, eps, cos[:-1], sin[:-1], B, N, Hq, Hkv)
    with pytest.raises(ValueError):
        K.qk_norm_rope_half_(x, wq[:64], wk, eps, cos, sin, B, N, Hq, Hkv)


# ---- encoder vs transformers -------------------------------------------------------------------
@torch.no_grad()
def _hf_outputs(hf, ids, mask, dev):
    """(fp32 eager oracle, the same model in bf16): hidden_states[-2] on right-padded ids."""
    hf = hf.to(dev)
    ids, mask = ids.to(dev), mask.to(dev)
    ref = hf(input_ids=ids, attention_mask=mask, output_hidden_states=True).hidden_states[-2]
    b16 = copy.deepcopy(hf).to(torch.bfloat16)(input_ids=ids, attention_mask=mask,
                                               output_hidden_states=True).hidden_states[-2].float()
    return ref, b16


@pytest.fixture(scope="module")
def oracle(dev, tmp_path_factory):
    hf = tiny_hf_model(0)                  # hidden 128, 4 heads on 2 KV heads x 128, ffn 256, 3 layers, vocab 512
    root = tmp_path_factory.mktemp("qwen3")
    st, cfg = hf_state(hf), hf_config(hf)
    d = export_dir(root / "tiny", st, cfg)
    # the same weights under a config that claims one layer more: an encoder that runs all 3 layers
    d_all = export_dir(root / "all_layers", st, {**cfg, "num_hidden_layers": cfg["num_hidden_layers"] + 1})
    ids, mask = padded_ids(LENS, 512, 0)
    ref, b16 = _hf_outputs(hf, ids, mask, dev)
    return d, d_all, ids, ref, b16


def test_encoder_vs_transformers(dev, oracle):
    d, d_all, ids, ref, b16 = oracle
    enc = ck.load_qwen3_encoder(d, dev)
    assert len(enc.blocks) == 2
    lens = torch.tensor(LENS)
    ours = enc(ids, lens)
    assert ours.shape == (3, 130, 128) and ours.dtype == torch.bfloat16 and bool(torch.isfinite(ours.float()).all())
    # the same prompts trimmed: a batch whose longest prompt is 40 runs on 40 rows per prompt
    short = enc(ids[:2], lens[:2])
    assert short.shape == (2, 40, 128)
    # what the bar must not pass: every layer run (last_hidden_state before the final norm) ...
    all_layers = ck.load_qwen3_encoder(d_all, dev)
    assert len(all_layers.blocks) == 3
    deep = all_layers(ids, lens)
    # ... and the q / k norm weights forced to 1
    for b in enc.blocks:
        b.q_norm.fill_(1.0)
        b.k_norm.fill_(1.0)
    unit = enc(ids, lens)
    for b, L in enumerate(LENS):
        e_ours, e_ref = rel_err(ours[b, :L], ref[b, :L]), rel_err(b16[b, :L], ref[b, :L])
        e_short = rel_err(short[b, :L], ref[b, :L]) if b < 2 else float("nan")
        e_deep, e_unit = rel_err(deep[b, :L], ref[b, :L]), rel_err(unit[b, :L], ref[b, :L])
        print(f"qwen3 encoder len {L}: ours {e_ours:.3e} trimmed {e_short:.3e} bf16 reference {e_ref:.3e} "
              f"bar {1.5 * e_ref:.3e} all layers {e_deep:.3e} q/k norm weights 1 {e_unit:.3e}")
        assert e_ours <= 1.5 * e_ref, (L, e_ours, e_ref)
        if b < 2:
            assert e_short <= 1.5 * e_ref, (L, e_short, e_ref)
        assert e_deep > 1.5 * e_ref, (L, e_deep, e_ref)
        assert e_unit > 1.5 * e_ref, (L, e_unit, e_ref)


def test_encoder_four_query_heads_on_one_kv_head(dev, tmp_path):
    """G = 4: every query head of a layer reads the one KV head.  The same bar."""
    hf = tiny_hf_model(2, num_attention_heads=4, num_key_value_heads=1)
    enc = ck.load_qwen3_encoder(export_dir(tmp_path / "g4", hf_state(hf), hf_config(hf)), dev)
    assert (enc.arch.num_heads, enc.arch.num_kv_heads) == (4, 1)
    lens = [7, 33]
    ids, mask = padded_ids(lens, 512, 2, seq=64)
    ref, b16 = _hf_outputs(hf, ids, mask, dev)
    ours = enc(ids, torch.tensor(lens))
    assert ours.shape == (2, 33, 128)
    for b, L in enumerate(lens):
        e_ours, e_ref = rel_err(ours[b, :L], ref[b, :L]), rel_err(b16[b, :L], ref[b, :L])
        print(f"qwen3 encoder 4 heads / 1 KV head len {L}: ours {e_ours:.3e} bf16 reference {e_ref:.3e}")
        assert e_ours <= 1.5 * e_ref, (L, e_ours, e_ref)


# ---- end to end --------------------------------------------------------------------------------
TINY_ZIMAGE = ZImageArch(dim=256, n_layers=2, n_refiner_layers=1, n_heads=2, ffn=512, cap_feat_dim=128, t_mid=256,
                         seq_multiple=16)
PX = 64     # the smallest size of tests/test_gpu_zimage.py: 8 x 8 latent, 16 image tokens
PROMPTS = ["A photo of RED cat on the moon", "# an old man reading in the park", "two birds over the sea at night"]


@pytest.fixture(scope="module")
def zimage_dir(tmp_path_factory):
    """A local directory in the diffusers layout, the text side only: text_encoder/ (tiny Qwen3, hidden =
    TINY_ZIMAGE.cap_feat_dim) and tokenizer/, and a prompt .txt with a # line (a prompt here) and a blank line."""
    root = tmp_path_factory.mktemp("e2e")
    hf = tiny_hf_model(1)
    export_dir(root / "model" / "text_encoder", hf_state(hf), hf_config(hf))
    make_tokenizer(root / "model" / "tokenizer")
    txt = root / "prompts.txt"
    txt.write_text(f"{PROMPTS[0]}\n\n  {PROMPTS[1]}\n{PROMPTS[2]}\n", encoding="utf-8")
    return root, root / "model", txt, hf


def test_encode_prompts_end_to_end(dev, zimage_dir, monkeypatch):
    from transformers import AutoTokenizer
    root, model, txt, hf = zimage_dir
    es = ZImageTurboES(str(model), device=str(dev), arch=TINY_ZIMAGE, encode_only=True)
    assert es.transformer is None and es.vae is None
    enc_path = root / "out" / "enc.pt"
    data = es.encode_prompts(txt, enc_path, batch_size=2, drop_text_encoder_after=False)
    assert enc_path.is_file() and data["prompts"] == PROMPTS and es.text_encoder is not None
    assert set(data) == {"prompts", "prompt_embeds"}
    pe = data["prompt_embeds"]
    assert isinstance(pe, list) and len(pe) == 3
    htok = AutoTokenizer.from_pretrained(str(model / "tokenizer"))
    htok.padding_side = "right"
    strings = [htok.apply_chat_template([{"role": "user", "content": p}], tokenize=False, add_generation_prompt=True,
                                        enable_thinking=True) for p in PROMPTS]
    tok = htok(strings, padding="max_length", max_length=64, truncation=True, return_tensors="pt")
    lens = tok.attention_mask.sum(-1).tolist()
    assert lens == [len(s.split()) for s in strings] == [len(p.split()) + 5 for p in PROMPTS]
    ref, b16 = _hf_outputs(hf, tok.input_ids, tok.attention_mask, dev)
    for i, L in enumerate(lens):
        assert pe[i].shape == (L, 128) and pe[i].dtype == torch.bfloat16 and pe[i].device.type == "cpu"
        e_ours, e_ref = rel_err(pe[i].to(dev), ref[i, :L]), rel_err(b16[i, :L], ref[i, :L])
        print(f"encode_prompts prompt {i} len {L}: ours {e_ours:.3e} bf16 reference {e_ref:.3e}")
        assert e_ours <= 1.5 * e_ref, (i, e_ours, e_ref)
    saved = torch.load(enc_path, map_location="cpu", weights_only=True)
    assert saved["prompts"] == PROMPTS and all(torch.equal(a, b) for a, b in zip(saved["prompt_embeds"], pe))
    # a second call without overwrite loads the file: no encoder is built, none is asked to encode
    es.drop_text_encoder()
    assert es.text_encoder is None
    import hyperscalees_t2i_amd.zimage_pipeline as zp

    def boom(*a, **k):
        raise AssertionError("encode_prompts built an encoder although the encoded file exists")
    monkeypatch.setattr(zp, "QwenPromptEncoder", boom)
    again = es.encode_prompts(txt, enc_path, batch_size=2, overwrite=False)
    assert es.text_encoder is None and again["prompts"] == PROMPTS
    assert all(torch.equal(a, b) for a, b in zip(again["prompt_embeds"], pe))


def test_backend_encodes_from_txt_and_generates(dev, zimage_dir):
    root, model, txt, _ = zimage_dir
    enc_path = root / "backend" / "enc.pt"
    cfg = ZImageConfig(model_name=str(model), synthetic_weights=True, arch=TINY_ZIMAGE, vae_widths=(32, 32, 64, 64),
                       width_px=PX, height_px=PX, num_inference_steps=3, prompts_per_gen=2, batches_per_gen=2,
                       prompts_txt_path=str(txt), encoded_prompt_path=str(enc_path), auto_encode_if_missing=True)
    be = ZImageBackend(str(dev), cfg)
    be.init_and_attach_lora()
    assert enc_path.is_file() and be.prompts_list == PROMPTS
    assert len(be.base_prompt_embeds) == 3 and all(e.shape[1] == 128 for e in be.base_prompt_embeds)
    assert be.es_model.text_encoder is None and be.es_model.transformer is not None
    params, shapes = be.collect_lora_params()
    noiser = EggRollNoiser(shapes, sigma=5e-2, lr_scale=0.1, rank=1, use_antithetic=True)
    tp = noiser.perturb(flatten_params(params).to(dev), noiser.epoch_noise(2, seed=4), 2, 0, 2)
    flat = be.step_sampling_info(1)["flat_ids"]
    imgs = be.generate_population(flat, 1, cfg.guidance_scale, tp)
    assert imgs.shape == (2 * len(flat), 3, PX, PX) and bool(torch.isfinite(imgs.float()).all())
