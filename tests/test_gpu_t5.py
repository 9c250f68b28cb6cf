"""T5 prompt encoder on the GPU: eggroll_relbias_attention against fp32 SDPA, the encoder against
transformers' T5EncoderModel (fp32 oracle, the same model in bf16 as the yardstick), and the prompt .txt ->
encoded file -> Infinity population pass path end to end.

Encoder bar: per prompt, our relative Frobenius error against the fp32 oracle over the valid rows is at most
1.5x the error of the reference model itself run in bf16 on the same GPU and inputs.  Measured on an MI355X
(profiles/t5_encoder_vs_transformers.json), lengths 5 / 200 / 512: ours 6.2e-3 / 5.1e-3 / 5.1e-3, the bf16
reference 7.6e-3 / 6.5e-3 / 6.5e-3; with the bias table mirrored (key - query -> query - key) ours is
6.3e-2 / 2.3e-2 / 1.4e-2.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import checkpoints as ck
from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd import t5 as T5
from hyperscalees_t2i_amd.backend import InfinityBackend, InfinityConfig
from hyperscalees_t2i_amd.es import EggRollNoiser, flatten_params
from hyperscalees_t2i_amd.infinity import InfinityArch
from hyperscalees_t2i_amd.infinity_pipeline import InfinityES
from tests.t5_tiny import export_dir, hf_state, make_tokenizer, rel_err, tiny_hf_encoder

pytestmark = pytest.mark.gpu


# ---- kernel ------------------------------------------------------------------------------------
def _inputs(dev, B, N, H, R, sliced, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    if sliced:   # q / k / v as column slices of one [B*N, 3*H*64] tensor (the fused qkv GEMM's output)
        qkv = (torch.randn((B * N, 3 * H * 64), generator=g, device=dev) * 0.5).to(torch.bfloat16)
        q, k, v = qkv[:, :H * 64], qkv[:, H * 64:2 * H * 64], qkv[:, 2 * H * 64:]
    else:
        q, k, v = [(torch.randn((B * N, H * 64), generator=g, device=dev) * 0.5).to(torch.bfloat16) for _ in range(3)]
    # dense random table: one independent value per (head, key - query)
    table = torch.randn((H, 2 * R - 1), generator=g, device=dev)
    return q, k, v, table


def _sdpa_ref(q, k, v, table, lens, B, N, H, R, scale):
    i, j = torch.arange(N, device=q.device)[:, None], torch.arange(N, device=q.device)[None, :]
    mask = torch.zeros((B, 1, 1, N), device=q.device)
    for b, L in enumerate(lens):
        mask[b, ..., L:] = float("-inf")
    attn_mask = table[:, j - i + R - 1][None] + mask                     # [B, H, N, N]
    t = lambda x: x.reshape(B, N, H, 64).transpose(1, 2).float()  # noqa: E731
    return F.scaled_dot_product_attention(t(q), t(k), t(v), attn_mask=attn_mask, scale=scale).transpose(1, 2).reshape(
        B * N, H * 64)


@pytest.mark.parametrize("B,N,H,lens,R,sliced,scale", [
    (3, 37, 3, [37, 1, 20], 37, False, 1.0),
    (2, 64, 1, [64, 16], 70, False, 1.0),
    (2, 65, 2, [65, 33], 65, True, 1.0),              # two query blocks, two key blocks, qkv read in place
    (1, 512, 2, [512], 512, False, 1.0),
    (2, 512, 1, [129, 511], 512, True, 0.125),
])
def test_relbias_attention_vs_sdpa(dev, B, N, H, lens, R, sliced, scale):
    q, k, v, table = _inputs(dev, B, N, H, R, sliced, seed=N * 7 + B)
    ours = K.relbias_attention(q, k, v, table, torch.tensor(lens), B, N, H, scale).float()
    ref = _sdpa_ref(q, k, v, table, lens, B, N, H, R, scale)
    valid = torch.zeros(B, N, dtype=torch.bool, device=dev)
    for b, L in enumerate(lens):
        valid[b, :L] = True
    valid = valid.view(-1)
    o, r = ours[valid], ref[valid]
    rel, mx = rel_err(o, r), float((o - r).abs().max())
    print(f"relbias_attention B{B} N{N} H{H} lens{lens}: rel {rel:.3e} max|d| {mx:.3e} max|ref| {float(r.abs().max()):.3e}")
    assert rel < 1e-2, rel     # bf16 P (probabilities rounded before the PV MFMA) + bf16 output
    assert mx < 3e-2 * float(r.abs().max())
    assert not ours[~valid].any()                     # query rows >= len[b]: exactly zero


def test_relbias_attention_batch_independence_bitwise(dev):
    B, N, H, lens = 3, 100, 2, [100, 7, 64]
    q, k, v, table = _inputs(dev, B, N, H, 128, True, seed=5)
    full = K.relbias_attention(q, k, v, table, torch.tensor(lens), B, N, H)
    for b in range(B):
        s = slice(b * N, (b + 1) * N)
        one = K.relbias_attention(q[s], k[s], v[s], table, torch.tensor(lens[b:b + 1]), 1, N, H)
        assert torch.equal(full[s], one), b


def test_relbias_attention_lens_edges_and_host_checks(dev):
    """len 0: the whole sequence is zeros (no NaN); a device-resident lens outside [0, N] is clamped in the
    kernel; a CPU-resident one is refused on the host, like shapes outside the kernel's limits."""
    B, N, H = 3, 20, 2
    q, k, v, table = _inputs(dev, B, N, H, N, False, seed=9)
    out = K.relbias_attention(q, k, v, table, torch.tensor([0, 20, 3]), B, N, H, out=torch.full(
        (B * N, H * 64), float("nan"), dtype=torch.bfloat16, device=dev))
    assert not out[:N].any() and not out[2 * N + 3:].any() and bool(torch.isfinite(out.float()).all())
    clamped = K.relbias_attention(q, k, v, table, torch.tensor([-4, 99, 3], device=dev), B, N, H)
    assert torch.equal(clamped, out)
    with pytest.raises(ValueError):
        K.relbias_attention(q, k, v, table, torch.tensor([0, 21, 3]), B, N, H)
    with pytest.raises(ValueError):
        K.relbias_attention(q, k, v, table[:, 1:-1].contiguous(), torch.tensor([0, 20, 3]), B, N, H)   # R < N
    with pytest.raises(ValueError):
        K.relbias_attention(q, k, v, table, torch.tensor([1]), 1, 513, H)
    with pytest.raises(_lib.EggrollError):
        K.relbias_attention(q.float(), k, v, table, torch.tensor([0, 20, 3]), B, N, H)


# ---- encoder vs transformers -------------------------------------------------------------------
LENS = [5, 200, 512]


def _padded_ids(lens, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(lens), 512, dtype=torch.long)
    mask = torch.zeros(len(lens), 512, dtype=torch.long)
    for b, L in enumerate(lens):
        ids[b, :L] = torch.randint(3, vocab, (L,), generator=g)
        mask[b, :L] = 1
    return ids, mask


@torch.no_grad()
def _hf_outputs(hf, ids, mask, dev):
    """(fp32 oracle, the same model in bf16) on ids padded to 512, the reference's form."""
    hf = hf.to(dev)
    ids, mask = ids.to(dev), mask.to(dev)
    ref = hf(input_ids=ids, attention_mask=mask).last_hidden_state
    b16 = copy.deepcopy(hf).to(torch.bfloat16)(input_ids=ids, attention_mask=mask).last_hidden_state.float()
    return ref, b16


@pytest.fixture(scope="module")
def oracle(dev, tmp_path_factory):
    hf = tiny_hf_encoder(0)                # d_model 128, 3 heads x 64, d_ff 256, 2 layers, vocab 512
    d = export_dir(tmp_path_factory.mktemp("t5") / "tiny", hf_state(hf), hf.config.to_dict())
    ids, mask = _padded_ids(LENS, 512, 0)
    ref, b16 = _hf_outputs(hf, ids, mask, dev)
    return d, ids, ref, b16


def test_encoder_vs_transformers(dev, oracle, monkeypatch):
    d, ids, ref, b16 = oracle
    enc = ck.load_t5_encoder(d, dev)
    lens = torch.tensor(LENS)
    ours = enc(ids, lens)
    assert ours.shape == (3, 512, 128) and ours.dtype == torch.bfloat16 and bool(torch.isfinite(ours.float()).all())
    # the same prompts trimmed: a batch whose longest prompt is 200 runs on 200 rows per prompt
    short = enc(ids[:2], lens[:2])
    assert short.shape == (2, 200, 128)
    # a mirrored bias table (query - key): what the bar must not pass
    table = T5.rel_bias_table
    monkeypatch.setattr(T5, "rel_bias_table", lambda *a, **kw: table(*a, **kw).flip(1).contiguous())
    wrong = enc(ids, lens)
    monkeypatch.undo()
    for b, L in enumerate(LENS):
        e_ours, e_ref = rel_err(ours[b, :L], ref[b, :L]), rel_err(b16[b, :L], ref[b, :L])
        e_short = rel_err(short[b, :L], ref[b, :L]) if b < 2 else float("nan")
        e_wrong = rel_err(wrong[b, :L], ref[b, :L])
        print(f"t5 encoder len {L}: ours {e_ours:.3e} trimmed {e_short:.3e} bf16 reference {e_ref:.3e} "
              f"bar {1.5 * e_ref:.3e} mirrored bias {e_wrong:.3e}")
        assert e_ours <= 1.5 * e_ref, (L, e_ours, e_ref)
        if b < 2:
            assert e_short <= 1.5 * e_ref, (L, e_short, e_ref)
            # the fp32 oracle with its bias mirrored differs from itself by 6.2e-2 (len 5) and 2.2e-2 (len 200):
            # both more than twice the bar, so a wrong sign cannot pass (at 512 it is 1.3e-2: recorded only)
            assert e_wrong > 1.5 * e_ref, (L, e_wrong, e_ref)


def test_encoder_widths_outside_the_gemm_rule(dev, tmp_path):
    """d_model 96, d_ff 160: q/k/v, wi_0 / wi_1 and the feed-forward wo have K % 64 != 0 and run through
    F.linear with the same op after them, the attention output projection (K = 192) stays on the library's
    GEMM.  The same bar."""
    hf = tiny_hf_encoder(2, d_model=96, d_ff=160)
    enc = ck.load_t5_encoder(export_dir(tmp_path / "odd", hf_state(hf), hf.config.to_dict()), dev)
    lens = [7, 33]
    ids, mask = _padded_ids(lens, 512, 2)
    ref, b16 = _hf_outputs(hf, ids, mask, dev)
    ours = enc(ids, torch.tensor(lens))
    assert ours.shape == (2, 33, 96)
    for b, L in enumerate(lens):
        e_ours, e_ref = rel_err(ours[b, :L], ref[b, :L]), rel_err(b16[b, :L], ref[b, :L])
        print(f"t5 encoder d_model 96 len {L}: ours {e_ours:.3e} bf16 reference {e_ref:.3e}")
        assert e_ours <= 1.5 * e_ref, (L, e_ours, e_ref)


# ---- end to end --------------------------------------------------------------------------------
TINY_INF = InfinityArch(depth=2, embed_dim=256, num_heads=2, block_chunks=2, text_channels=256, codebook_dim=4,
                        spatial_patchify=1, vae_widths=(32, 32, 64, 64))
PROMPTS = ["a photo of red cat on the moon", "an old man reading in the park", "two birds over the sea at night"]


@pytest.fixture(scope="module")
def t5_dir(tmp_path_factory):
    """A local directory as InfinityES wants it: tiny T5 (d_model = TINY_INF.text_channels) + tokenizer files,
    and a 5-line prompt .txt with a comment line and a blank line."""
    root = tmp_path_factory.mktemp("e2e")
    hf = tiny_hf_encoder(1, d_model=256)
    d = export_dir(root / "t5", hf_state(hf), hf.config.to_dict())
    make_tokenizer(d)
    txt = root / "prompts.txt"
    txt.write_text(f"# prompts\n{PROMPTS[0]}\n\n{PROMPTS[1]}\n{PROMPTS[2]}\n", encoding="utf-8")
    return root, d, txt, hf


def test_encode_prompts_end_to_end(dev, t5_dir):
    from transformers import AutoTokenizer
    root, d, txt, hf = t5_dir
    es = InfinityES(model_path="", text_encoder_ckpt=str(d), vae_path="", vae_type=14, pn="0.06M", arch=TINY_INF,
                    synthetic_weights=True, device=str(dev), vae_chunk=8)
    enc_path = root / "out" / "enc.pt"
    data = es.encode_prompts(txt, enc_path, batch_size=2)
    assert enc_path.is_file() and data["prompts"] == PROMPTS and es.text_encoder is not None
    tok = AutoTokenizer.from_pretrained(str(d), legacy=True)(text=PROMPTS, max_length=512, padding="max_length",
                                                              truncation=True, return_tensors="pt")
    lens = tok.attention_mask.sum(-1).tolist()
    assert data["lens_list"] == lens == [len(p.split()) + 1 for p in PROMPTS]
    ref, b16 = _hf_outputs(hf, tok.input_ids, tok.attention_mask, dev)
    for i, L in enumerate(lens):
        kv = data["kv_compact_list"][i]
        assert kv.device.type == "cpu" and kv.dtype == torch.float16 and kv.shape == (L, 256)
        e_ours, e_ref = rel_err(kv.to(dev), ref[i, :L]), rel_err(b16[i, :L], ref[i, :L])
        print(f"encode_prompts prompt {i} len {L}: ours {e_ours:.3e} bf16 reference {e_ref:.3e}")
        assert e_ours <= 1.5 * e_ref, (i, e_ours, e_ref)
    es.drop_text_encoder()
    assert es.text_encoder is None
    again = es.encode_prompts(txt, enc_path, batch_size=2, overwrite=False)       # the file, no encoder built
    assert es.text_encoder is None and again["prompts"] == PROMPTS and again["lens_list"] == lens
    assert all(torch.equal(a, b) for a, b in zip(again["kv_compact_list"], data["kv_compact_list"]))
    f32 = es.encode_prompts(txt, root / "out" / "enc32.pt", batch_size=8, store_dtype="float32")
    assert all(t.dtype == torch.float32 for t in f32["kv_compact_list"])
    es.text_encoder_ckpt = "google/flan-t5-xl"
    es.drop_text_encoder()
    with pytest.raises(FileNotFoundError, match="google/flan-t5-xl"):
        es.encode_prompts(txt, root / "out" / "never.pt")


def test_backend_encodes_from_txt_and_generates(dev, t5_dir):
    root, d, txt, _ = t5_dir
    enc_path = root / "backend" / "enc.pt"
    cfg = InfinityConfig(synthetic_weights=True, arch=TINY_INF, pn="0.06M", prompts_per_gen=2, batches_per_gen=2,
                         micro_batch=0, vae_chunk=8, prompts_txt_path=str(txt), encoded_prompt_path=str(enc_path),
                         auto_encode_if_missing=True, text_encoder_ckpt=str(d), encode_batch_size=2)
    be = InfinityBackend(str(dev), cfg)
    be.init_and_attach_lora()
    assert enc_path.is_file() and be.prompts_list == PROMPTS
    assert be.lens_list == [len(p.split()) + 1 for p in PROMPTS]
    params, shapes = be.collect_lora_params()
    noiser = EggRollNoiser(shapes, sigma=5e-2, lr_scale=0.1, rank=1, use_antithetic=True)
    tp = noiser.perturb(flatten_params(params).to(dev), noiser.epoch_noise(2, seed=4), 2, 0, 2)
    flat = be.step_sampling_info(1)["flat_ids"]
    imgs = be.generate_population(flat, 1, cfg.guidance_scale, tp)
    assert imgs.shape[0] == 2 * len(flat) and imgs.shape[1] == 3 and bool(torch.isfinite(imgs.float()).all())
