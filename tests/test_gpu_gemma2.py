"""Gemma-2 prompt encoder on the GPU: eggroll_softcap_attention against an fp32 torch restatement of
transformers' eager attention, eggroll_rope_half against the rotate_half expression, the encoder against
transformers' Gemma2Model (fp32 eager oracle, the same model in bf16 as the yardstick), and the prompt .txt ->
encoded file -> Sana population pass path end to end.

Encoder bar: per prompt, our relative Frobenius error against the fp32 oracle over the valid rows is at most
1.5x the error of the reference model itself run in bf16 on the same GPU and inputs (the ratio of
tests/test_gpu_t5.py: the same bf16 GEMMs and roundings, summed in another order).  Measured on an MI355X
(profiles/gemma2_encoder_vs_transformers.json), lengths 5 / 40 / 300: ours 7.2e-3 / 1.04e-2 / 8.9e-3, the bf16
reference 9.3e-3 / 1.43e-2 / 2.63e-2; with the soft-cap off ours is 6.7e-2 / 0.18 / 0.33.  With 4 query heads on
one KV head, lengths 7 / 33: ours 8.7e-3 / 1.00e-2, the bf16 reference 1.05e-2 / 1.38e-2.  The kernel against
the fp32 eager restatement: 1.4e-3 to 1.9e-3 (bar 1e-2) with pre-cap logits up to 3.0x (cap 5) and 3.2x (cap 50)
the cap.
"""
import copy
import dataclasses

import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import checkpoints as ck
from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd.backend import SanaBackend, SanaConfig
from hyperscalees_t2i_amd.es import EggRollNoiser, flatten_params
from hyperscalees_t2i_amd.gemma2 import rope_tables
from hyperscalees_t2i_amd.pipeline import GemmaPromptEncoder, SanaOneStep
from hyperscalees_t2i_amd.sana import SanaArch
from tests.gemma2_tiny import LENS, export_dir, hf_config, hf_state, make_tokenizer, padded_ids, rel_err, tiny_hf_model

pytestmark = pytest.mark.gpu
HD = 256


# ---- kernel ------------------------------------------------------------------------------------
def _inputs(dev, B, N, Hq, Hkv, sliced, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    if sliced:   # q / k / v as column slices of one [B*N, (Hq + 2 Hkv)*256] tensor (the fused qkv GEMM's output)
        qkv = torch.randn((B * N, (Hq + 2 * Hkv) * HD), generator=g, device=dev).to(torch.bfloat16)
        return qkv[:, :Hq * HD], qkv[:, Hq * HD:(Hq + Hkv) * HD], qkv[:, (Hq + Hkv) * HD:]
    return [torch.randn((B * N, h * HD), generator=g, device=dev).to(torch.bfloat16) for h in (Hq, Hkv, Hkv)]


def _scale(cap):
    """q . k of unit-variance inputs has std 16 at head dim 256: pre-cap logits of std 0.6 cap reach past +-cap."""
    return 0.6 * cap / 16.0 if cap > 0 else 1.0 / 16.0


def _eager_ref(q, k, v, lens, B, N, Hq, Hkv, scale, cap):
    """Gemma2's eager_attention_forward in fp32: repeat_kv, scale, soft-cap, then the causal + key-padding mask."""
    t = lambda x, h: x.reshape(B, N, h, HD).transpose(1, 2).float()  # noqa: E731
    qq, kk, vv = t(q, Hq), t(k, Hkv).repeat_interleave(Hq // Hkv, 1), t(v, Hkv).repeat_interleave(Hq // Hkv, 1)
    pre = qq @ kk.transpose(-1, -2) * scale
    s = cap * torch.tanh(pre / cap) if cap > 0 else pre
    i, j = torch.arange(N, device=q.device)[:, None], torch.arange(N, device=q.device)[None, :]
    keep = (j <= i)[None, None] & (j[None, None] < torch.tensor(lens, device=q.device).view(B, 1, 1, 1))
    p = torch.softmax(s.masked_fill(~keep, float("-inf")), -1)
    return (p @ vv).transpose(1, 2).reshape(B * N, Hq * HD), float(pre.abs().max())


@pytest.mark.parametrize("B,N,Hq,Hkv,lens,cap,sliced", [
    (3, 37, 4, 2, [37, 1, 20], 5.0, False),
    (2, 64, 2, 2, [64, 16], 5.0, False),
    (2, 65, 8, 4, [65, 33], 50.0, True),               # two query blocks, three key blocks, qkv read in place
    (1, 1, 2, 1, [1], 5.0, False),
    (1, 300, 8, 4, [300], 50.0, False),
    (2, 300, 4, 1, [129, 299], 0.0, False),            # cap = 0: plain causal attention
])
def test_softcap_attention_vs_eager(dev, B, N, Hq, Hkv, lens, cap, sliced):
    q, k, v = _inputs(dev, B, N, Hq, Hkv, sliced, seed=N * 7 + B)
    scale = _scale(cap)
    ours = K.softcap_attention(q, k, v, torch.tensor(lens), B, N, Hq, Hkv, scale, cap).float()
    ref, pre_max = _eager_ref(q, k, v, lens, B, N, Hq, Hkv, scale, cap)
    valid = torch.zeros(B, N, dtype=torch.bool, device=dev)
    for b, L in enumerate(lens):
        valid[b, :L] = True
    valid = valid.view(-1)
    o, r = ours[valid], ref[valid]
    rel, mx = rel_err(o, r), float((o - r).abs().max())
    print(f"softcap_attention B{B} N{N} H{Hq}/{Hkv} lens{lens} cap{cap}: rel {rel:.3e} max|d| {mx:.3e} "
          f"max|ref| {float(r.abs().max()):.3e} max|pre-cap logit| {pre_max:.2f}")
    if cap > 0 and N > 1:
        assert pre_max > cap, pre_max                  # the cap is at work
    assert rel < 1e-2, rel     # bf16 P (probabilities rounded before the PV MFMA) + bf16 output
    assert mx < 3e-2 * float(r.abs().max())
    assert not ours[~valid].any()                      # query rows >= len[b]: exactly zero


def test_softcap_attention_batch_independence_bitwise(dev):
    B, N, Hq, Hkv, lens = 3, 100, 4, 2, [100, 7, 64]
    q, k, v = _inputs(dev, B, N, Hq, Hkv, True, seed=5)
    full = K.softcap_attention(q, k, v, torch.tensor(lens), B, N, Hq, Hkv, _scale(5.0), 5.0)
    for b in range(B):
        s = slice(b * N, (b + 1) * N)
        one = K.softcap_attention(q[s], k[s], v[s], torch.tensor(lens[b:b + 1]), 1, N, Hq, Hkv, _scale(5.0), 5.0)
        assert torch.equal(full[s], one), b


def test_softcap_attention_lens_edges_and_host_checks(dev):
    """len 0: the whole sequence is zeros (no NaN); a device-resident lens outside [0, N] is clamped in the
    kernel; a CPU-resident one is refused on the host, like shapes outside the kernel's limits."""
    B, N, Hq, Hkv = 3, 20, 2, 1
    q, k, v = _inputs(dev, B, N, Hq, Hkv, False, seed=9)
    sc = _scale(5.0)
    out = K.softcap_attention(q, k, v, torch.tensor([0, 20, 3]), B, N, Hq, Hkv, sc, 5.0, out=torch.full(
        (B * N, Hq * HD), float("nan"), dtype=torch.bfloat16, device=dev))
    assert not out[:N].any() and not out[2 * N + 3:].any() and bool(torch.isfinite(out.float()).all())
    assert bool(out[N:2 * N].any())
    clamped = K.softcap_attention(q, k, v, torch.tensor([-4, 99, 3], device=dev), B, N, Hq, Hkv, sc, 5.0)
    assert torch.equal(clamped, out)
    with pytest.raises(ValueError):
        K.softcap_attention(q, k, v, torch.tensor([0, 21, 3]), B, N, Hq, Hkv, sc, 5.0)
    with pytest.raises(ValueError):
        K.softcap_attention(q, k, v, torch.tensor([0, 20, 3]), B, N, 3, 2, sc, 5.0)           # Hq % Hkv != 0
    with pytest.raises(ValueError):
        K.softcap_attention(q, k, v, torch.tensor([0, 20, 3]), B, N, Hq, Hkv, sc, 5.0, head_dim=128)
    with pytest.raises(_lib.EggrollError):
        K.softcap_attention(q.float(), k, v, torch.tensor([0, 20, 3]), B, N, Hq, Hkv, sc, 5.0)


def test_rope_half_vs_rotate_half(dev):
    """In place on the first 3 heads of a strided view (the q | k columns of a fused qkv tensor): the fp32
    rotate_half expression of transformers, rounded once; the v columns and the column before the view are
    untouched."""
    B, N, heads, extra = 2, 37, 3, 2
    g = torch.Generator(device=dev).manual_seed(3)
    big = torch.randn((B * N, 8 + (heads + extra) * HD), generator=g, device=dev).to(torch.bfloat16)
    x = big[:, 8:]                                      # row stride 8 + 5*256, 16-byte aligned start
    before = big.clone()
    cos, sin = (t.to(dev) for t in rope_tables(N))
    v = x[:, :heads * HD].reshape(B, N, heads, HD).float()
    c, s = torch.cat([cos, cos], -1)[None, :, None, :], torch.cat([sin, sin], -1)[None, :, None, :]
    rot = torch.cat([-v[..., HD // 2:], v[..., :HD // 2]], -1)
    ref = (v * c + rot * s).reshape(B * N, heads * HD)
    K.rope_half_(x, cos, sin, B, N, heads)
    got = x[:, :heads * HD].float()
    assert float((got - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max())      # one bf16 rounding
    assert rel_err(got, ref) < 2.0 ** -8
    assert torch.equal(big[:, :8], before[:, :8]) and torch.equal(x[:, heads * HD:], before[:, 8 + heads * HD:])
    assert torch.equal(got[0], before[0, 8:8 + heads * HD].float())                   # position 0: the identity
    with pytest.raises(ValueError):
        K.rope_half_(x, cos[:-1], sin[:-1], B, N, heads)


# ---- encoder vs transformers -------------------------------------------------------------------
@torch.no_grad()
def _hf_outputs(hf, ids, mask, dev):
    """(fp32 eager oracle, the same model in bf16) on right-padded ids, the reference's form."""
    hf = hf.to(dev)
    ids, mask = ids.to(dev), mask.to(dev)
    ref = hf(input_ids=ids, attention_mask=mask).last_hidden_state
    b16 = copy.deepcopy(hf).to(torch.bfloat16)(input_ids=ids, attention_mask=mask).last_hidden_state.float()
    return ref, b16


@pytest.fixture(scope="module")
def oracle(dev, tmp_path_factory):
    hf = tiny_hf_model(0)                  # hidden 128, 2 heads on 1 KV head x 256, ffn 256, 2 layers, vocab 512
    d = export_dir(tmp_path_factory.mktemp("gemma2") / "tiny", hf_state(hf), hf_config(hf))
    ids, mask = padded_ids(LENS, 512, 0)
    ref, b16 = _hf_outputs(hf, ids, mask, dev)
    return d, ids, ref, b16


def test_encoder_vs_transformers(dev, oracle, monkeypatch):
    d, ids, ref, b16 = oracle
    enc = ck.load_gemma2_encoder(d, dev)
    lens = torch.tensor(LENS)
    ours = enc(ids, lens)
    assert ours.shape == (3, 300, 128) and ours.dtype == torch.bfloat16 and bool(torch.isfinite(ours.float()).all())
    # the same prompts trimmed: a batch whose longest prompt is 40 runs on 40 rows per prompt
    short = enc(ids[:2], lens[:2])
    assert short.shape == (2, 40, 128)
    # the soft-cap forced off: what the bar must not pass
    monkeypatch.setattr(enc, "arch", dataclasses.replace(enc.arch, softcap=0.0))
    nocap = enc(ids, lens)
    monkeypatch.undo()
    assert enc.arch.softcap == 5.0
    for b, L in enumerate(LENS):
        e_ours, e_ref = rel_err(ours[b, :L], ref[b, :L]), rel_err(b16[b, :L], ref[b, :L])
        e_short = rel_err(short[b, :L], ref[b, :L]) if b < 2 else float("nan")
        e_nocap = rel_err(nocap[b, :L], ref[b, :L])
        print(f"gemma2 encoder len {L}: ours {e_ours:.3e} trimmed {e_short:.3e} bf16 reference {e_ref:.3e} "
              f"bar {1.5 * e_ref:.3e} soft-cap off {e_nocap:.3e}")
        assert e_ours <= 1.5 * e_ref, (L, e_ours, e_ref)
        if b < 2:
            assert e_short <= 1.5 * e_ref, (L, e_short, e_ref)
        assert e_nocap > 1.5 * e_ref, (L, e_nocap, e_ref)


def test_encoder_four_query_heads_on_one_kv_head(dev, tmp_path):
    """G = 4: every query head of a layer reads the one KV head.  The same bar."""
    hf = tiny_hf_model(2, num_attention_heads=4)
    enc = ck.load_gemma2_encoder(export_dir(tmp_path / "g4", hf_state(hf), hf_config(hf)), dev)
    assert (enc.arch.num_heads, enc.arch.num_kv_heads) == (4, 1)
    lens = [7, 33]
    ids, mask = padded_ids(lens, 512, 2, seq=64)
    ref, b16 = _hf_outputs(hf, ids, mask, dev)
    ours = enc(ids, torch.tensor(lens))
    assert ours.shape == (2, 33, 128)
    for b, L in enumerate(lens):
        e_ours, e_ref = rel_err(ours[b, :L], ref[b, :L]), rel_err(b16[b, :L], ref[b, :L])
        print(f"gemma2 encoder 4 heads / 1 KV head len {L}: ours {e_ours:.3e} bf16 reference {e_ref:.3e}")
        assert e_ours <= 1.5 * e_ref, (L, e_ours, e_ref)


# ---- end to end --------------------------------------------------------------------------------
TINY_SANA = SanaArch(num_attention_heads=4, attention_head_dim=32, num_layers=2, num_cross_attention_heads=2,
                     cross_attention_head_dim=64, caption_channels=128)
PROMPTS = ["A photo of RED cat on the moon", "an old man reading in the park", "two birds over the sea at night"]


@pytest.fixture(scope="module")
def sana_dir(tmp_path_factory):
    """A local directory in the diffusers layout, the text side only: text_encoder/ (tiny Gemma-2, hidden =
    TINY_SANA.caption_channels) and tokenizer/, and a 5-line prompt .txt with a comment line and a blank line."""
    root = tmp_path_factory.mktemp("e2e")
    hf = tiny_hf_model(1)
    export_dir(root / "model" / "text_encoder", hf_state(hf), hf_config(hf))
    make_tokenizer(root / "model" / "tokenizer")
    txt = root / "prompts.txt"
    txt.write_text(f"# prompts\n{PROMPTS[0]}\n\n{PROMPTS[1]}\n{PROMPTS[2]}\n", encoding="utf-8")
    return root, root / "model", txt, hf


def test_encode_prompts_end_to_end(dev, sana_dir):
    from transformers import AutoTokenizer
    root, model, txt, hf = sana_dir
    es = SanaOneStep(str(model), device=str(dev), encode_only=True)
    assert es.transformer is None and es.vae is None
    enc_path = root / "out" / "enc.pt"
    data = es.encode_prompts(txt, enc_path, batch_size=2)
    assert enc_path.is_file() and data["prompts"] == PROMPTS and es.text_encoder is not None
    pe, am = data["prompt_embeds"], data["prompt_attention_mask"]
    assert pe.shape == (3, 300, 128) and pe.dtype == torch.float16 and pe.device.type == "cpu"
    assert am.shape == (3, 300) and am.dtype == torch.int64 and am.device.type == "cpu"
    htok = AutoTokenizer.from_pretrained(str(model / "tokenizer"))
    htok.padding_side = "right"
    tok = htok([p.lower().strip() for p in PROMPTS], padding="max_length", max_length=300, truncation=True,
               add_special_tokens=True, return_tensors="pt")
    assert torch.equal(am, tok.attention_mask)
    lens = am.sum(-1).tolist()
    assert lens == [len(p.split()) + 1 for p in PROMPTS]               # BOS + one token per (lower-cased) word
    ref, b16 = _hf_outputs(hf, tok.input_ids, tok.attention_mask, dev)
    for i, L in enumerate(lens):
        e_ours, e_ref = rel_err(pe[i, :L].to(dev), ref[i, :L]), rel_err(b16[i, :L], ref[i, :L])
        print(f"encode_prompts prompt {i} len {L}: ours {e_ours:.3e} bf16 reference {e_ref:.3e}")
        assert e_ours <= 1.5 * e_ref, (i, e_ours, e_ref)
        assert not pe[i, L:].any()                                      # padded rows: zeros
    # a complex-human-instruction list: position 0, then the last 299 of the longer sequence
    chi = ["given a user prompt generate an enhanced prompt", "user prompt "]
    sel = GemmaPromptEncoder.select_index(300)
    ctok = htok(["\n".join(chi) + p.lower().strip() for p in PROMPTS], padding="max_length", max_length=11 + 298,
                truncation=True, add_special_tokens=True, return_tensors="pt")
    cdata = es.encode_prompts(txt, root / "out" / "enc_chi.pt", batch_size=8, complex_human_instruction=chi)
    assert cdata["prompt_embeds"].shape == (3, 300, 128) and torch.equal(cdata["prompt_attention_mask"], ctok.attention_mask[:, sel])
    cref, cb16 = (t[:, sel] for t in _hf_outputs(hf, ctok.input_ids, ctok.attention_mask, dev))
    for i in range(3):
        m = cdata["prompt_attention_mask"][i].bool()
        e_ours, e_ref = rel_err(cdata["prompt_embeds"][i][m].to(dev), cref[i][m]), rel_err(cb16[i][m], cref[i][m])
        assert e_ours <= 1.5 * e_ref, (i, e_ours, e_ref)
        assert not cdata["prompt_embeds"][i][~m].any()
    es.drop_text_encoder()
    assert es.text_encoder is None
    again = es.encode_prompts(txt, enc_path, batch_size=2, overwrite=False)       # the file, no encoder built
    assert es.text_encoder is None and again["prompts"] == PROMPTS
    assert torch.equal(again["prompt_embeds"], pe) and torch.equal(again["prompt_attention_mask"], am)


def test_backend_encodes_from_txt_and_generates(dev, sana_dir):
    root, model, txt, _ = sana_dir
    enc_path = root / "backend" / "enc.pt"
    cfg = SanaConfig(model_name=str(model), synthetic_weights=True, arch=TINY_SANA, width_latent=4, height_latent=4,
                     prompts_per_gen=2, batches_per_gen=2, vae_widths=(16, 32, 32, 64, 64, 64),
                     vae_layers=(1, 1, 1, 1, 1, 1), prompts_txt_path=str(txt), encoded_prompt_path=str(enc_path),
                     auto_encode_if_missing=True, encode_batch_size=2)
    be = SanaBackend(str(dev), cfg)
    be.init_and_attach_lora()
    assert enc_path.is_file() and be.prompts_list == PROMPTS
    assert be.base_prompt_embeds.shape == (3, 300, 128) and be.es_model.text_encoder is None
    params, shapes = be.collect_lora_params()
    noiser = EggRollNoiser(shapes, sigma=5e-2, lr_scale=0.1, rank=1, use_antithetic=True)
    tp = noiser.perturb(flatten_params(params).to(dev), noiser.epoch_noise(2, seed=4), 2, 0, 2)
    flat = be.step_sampling_info(1)["flat_ids"]
    imgs = be.generate_population(flat, 1, cfg.guidance_scale, tp)
    assert imgs.shape[0] == 2 * len(flat) and imgs.shape[1] == 3 and bool(torch.isfinite(imgs.float()).all())
