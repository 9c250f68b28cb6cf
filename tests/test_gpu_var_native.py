"""VAR's native attention path: eggroll_qk_l2norm_kv against its torch form, the transformer teacher-forced on
tests/golden/g11_var_model.npz with the path on and off (the bars of tests/test_var_model.py: the reference's
own fp32 run judges both), and free-running population generation on the native path.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import kernels as K
from tests.test_var_model import ARCH, FHAT_ABS, IMAGE_ABS, IMAGE_MEAN, LOGIT_REL, _build, _forced

pytestmark = pytest.mark.gpu

# (S, l, H, ltot, row0): a mid-cache append; one token per sequence at row 0 with an odd head count; VAR-d16's
# last scale (256 tokens behind 424 cached ones, 16 heads)
L2_SIZES = [(3, 20, 2, 57, 11), (2, 1, 3, 5, 0), (1, 256, 16, 680, 424)]
PAD = 8   # qkv rows 3C + 8 apart: the row stride is not the width


def _qkv(dev, S, l, H, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed + 17 * S + l)
    C = 64 * H
    x = (torch.randn(S * l, 3 * C + PAD, generator=g, device=dev) * 1.7).bfloat16()
    x[0, 64 * (H - 1):64 * H] = 0          # a zero head in q ...
    x[0, C:C + 64] = 0                     # ... and in k
    qs = (torch.rand(H, generator=g, device=dev) * 8 + 1).contiguous()
    return x, qs, C


def _cache(dev, S, ltot, C, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(2, S, ltot, C, generator=g, device=dev).bfloat16()


def _norm32(x, H):
    """F.normalize(x.float(), dim=-1) per 64-wide head: fp32 [rows, H, 64]."""
    return F.normalize(x.float().view(x.shape[0], H, 64), dim=-1)


def _close(got, ref):
    """Within one bf16 rounding of the fp32 reference (the bar of test_qk_norm_rope_kv_cache_append)."""
    d = (got.float() - ref).abs()
    bar = ref.abs() * 2.0 ** -7 + 1e-6
    assert bool((d <= bar).all()), float((d - bar).max())


@pytest.mark.parametrize("S,l,H,ltot,row0", L2_SIZES)
def test_qk_l2norm_kv_vs_torch(dev, S, l, H, ltot, row0):
    x, qs, C = _qkv(dev, S, l, H)
    x0 = x.clone()
    cache = _cache(dev, S, ltot, C)
    c0 = cache.clone()
    K.qk_l2norm_kv(x[:, :C], x[:, C:2 * C], x[:, 2 * C:3 * C], H, 1e-12, qscale=qs, kout=cache[0], vout=cache[1],
                   rows_per_seq=l, row0=row0)
    torch.cuda.synchronize()
    q_ref = (_norm32(x0[:, :C], H) * qs.view(1, H, 1)).view(-1, C)
    k_ref = _norm32(x0[:, C:2 * C], H).view(S, l, C)
    _close(x[:, :C], q_ref)
    _close(cache[0, :, row0:row0 + l], k_ref)
    assert torch.equal(cache[1, :, row0:row0 + l], x0[:, 2 * C:3 * C].view(S, l, C))         # v: bitwise
    assert torch.equal(x[:, C:], x0[:, C:])                                                  # k, v, pad columns: untouched
    assert torch.equal(cache[:, :, :row0], c0[:, :, :row0]) and torch.equal(cache[:, :, row0 + l:], c0[:, :, row0 + l:])
    assert torch.isfinite(x.float()).all() and torch.isfinite(cache.float()).all()
    assert (x[0, 64 * (H - 1):64 * H] == 0).all() and (cache[0, 0, row0, :64] == 0).all()    # zero heads stay zero
    # unit norm up to the bf16 rounding of 64 values, where the head was not zero
    kn = cache[0, :, row0:row0 + l].float().view(S * l, H, 64).norm(dim=-1)
    kn[0, 0] = 1.0
    assert float((kn - 1).abs().max()) < 2.0 ** -8


@pytest.mark.parametrize("absent", ("q", "k", "v", "kout", "qscale"))
def test_qk_l2norm_kv_parts_absent(dev, absent):
    """Each part absent in turn: the parts present give the bits of the full call, the absent one is untouched."""
    S, l, H, ltot, row0 = L2_SIZES[0]
    x, qs, C = _qkv(dev, S, l, H)
    x0 = x.clone()
    cache = _cache(dev, S, ltot, C)
    c0 = cache.clone()
    full, fcache = x0.clone(), c0.clone()
    K.qk_l2norm_kv(full[:, :C], full[:, C:2 * C], full[:, 2 * C:3 * C], H, 1e-12, qscale=qs, kout=fcache[0],
                   vout=fcache[1], rows_per_seq=l, row0=row0)
    q = None if absent == "q" else x[:, :C]
    k = None if absent == "k" else x[:, C:2 * C]
    v = None if absent == "v" else x[:, 2 * C:3 * C]
    K.qk_l2norm_kv(q, k, v, H, 1e-12, qscale=None if absent in ("q", "qscale") else qs,
                   kout=None if absent in ("k", "kout") else cache[0], vout=None if absent == "v" else cache[1],
                   rows_per_seq=l, row0=row0)
    torch.cuda.synchronize()
    assert torch.equal(x[:, 2 * C:], x0[:, 2 * C:])
    if absent == "q":
        assert torch.equal(x[:, :C], x0[:, :C])
    elif absent == "qscale":
        _close(x[:, :C], _norm32(x0[:, :C], H).view(-1, C))
    else:
        assert torch.equal(x[:, :C], full[:, :C])
    if absent == "k":
        assert torch.equal(x[:, C:2 * C], x0[:, C:2 * C]) and torch.equal(cache[0], c0[0])
    elif absent == "kout":   # k normalised in place, the key cache untouched
        assert torch.equal(cache[0], c0[0])
        assert torch.equal(x[:, C:2 * C].reshape(S, l, C), fcache[0, :, row0:row0 + l])
    else:
        assert torch.equal(x[:, C:2 * C], x0[:, C:2 * C]) and torch.equal(cache[0], fcache[0])
    assert torch.equal(cache[1], c0[1] if absent == "v" else fcache[1])


def test_qk_l2norm_kv_refused_call_writes_nothing(dev):
    S, l, H, ltot, row0 = L2_SIZES[0]
    x, qs, C = _qkv(dev, S, l, H)
    cache = _cache(dev, S, ltot, C)
    x0, c0 = x.clone(), cache.clone()
    ld, ob, ol = x.stride(0), cache.stride(1), cache.stride(2)
    qp, kp, vp = x.data_ptr(), x.data_ptr() + 2 * C, x.data_ptr() + 4 * C
    st = torch.cuda.current_stream(dev).cuda_stream

    def call(q=qp, ldq=ld, k=kp, v=vp, hd=64, kout=cache[0].data_ptr(), vout=cache[1].data_ptr(), ob=ob, ol=ol, rps=l,
             row0=row0, rows=S * l):
        _lib.call("eggroll_qk_l2norm_kv", q, ldq, k, ld, v, ld, rows, H, hd, 1e-12, qs.data_ptr(), kout, vout, ob, ol,
                  rps, row0, st)

    for kw, msg in (({"hd": 128}, "head_dim must be 64"), ({"ldq": ld + 4}, "bad strides"), ({"ldq": C - 8}, "bad strides"),
                    ({"q": qp + 2}, "16-byte aligned"), ({"kout": cache[0].data_ptr() + 8}, "16-byte aligned"),
                    ({"ol": C - 8}, "bad output geometry"), ({"ob": (row0 + l) * ol - 8}, "bad output geometry"),
                    ({"rps": 0}, "bad output geometry"), ({"row0": -1}, "bad output geometry"),
                    ({"vout": None}, "come together"), ({"k": None}, "kout needs k"), ({"rows": -1}, "bad sizes")):
        with pytest.raises(_lib.EggrollError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(cache, c0)
    call(rows=0)                                   # a no-op
    _lib.call("eggroll_qk_l2norm_kv", None, 0, None, 0, None, 0, S * l, H, 64, 1e-12, None, None, None, 0, 0, 1, 0, st)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and torch.equal(cache, c0)
    with pytest.raises(ValueError):                # the wrapper's own shape check: the slice does not fit the cache
        K.qk_l2norm_kv(x[:, :C], x[:, C:2 * C], x[:, 2 * C:3 * C], H, kout=cache[0], vout=cache[1], rows_per_seq=l,
                       row0=ltot - l + 1)
    assert torch.equal(x, x0) and torch.equal(cache, c0)


# ---------------------------------------------------------------------------------------------------
# the transformer
# ---------------------------------------------------------------------------------------------------


def _spies(monkeypatch):
    counts = {"flash": 0, "l2norm": 0, "sdpa": 0}

    def spy(name, fn):
        def wrapped(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(K, "flash_attention", spy("flash", K.flash_attention))
    monkeypatch.setattr(K, "qk_l2norm_kv", spy("l2norm", K.qk_l2norm_kv))
    monkeypatch.setattr(F, "scaled_dot_product_attention", spy("sdpa", F.scaled_dot_product_attention))
    return counts


@pytest.mark.parametrize("use_kernel", (True, False), ids=("native", "torch"))
def test_var_teacher_forced_both_paths(golden, dev, monkeypatch, use_kernel):
    """Teacher-forced on the reference's token maps: both paths within the bars of tests/test_var_model.py, and the
    native one really runs the two kernels: depth x 10 calls each, no SDPA call from the transformer blocks.
    Measured worst per-scale logit error against the reference's fp32 run: DESIGN §3.3."""
    d = golden("g11_var_model.npz")
    cfg, top_k, top_p, g_seed = d["meta"]
    gen, _ = _build(dev, d["theta"])
    assert gen.infer.use_kernel is True            # the default
    gen.infer.use_kernel = use_kernel
    labels = torch.from_numpy(d["labels"]).to(dev)
    counts = _spies(monkeypatch)
    f_hat, _, logits = gen.infer.run(labels, 1, int(g_seed), float(cfg), int(top_k), float(top_p),
                                     force_idx=_forced(d, 1, dev), keep_logits=True)
    calls = ARCH.depth * len(ARCH.patch_nums)
    want = {"flash": calls, "l2norm": calls, "sdpa": 0} if use_kernel else {"flash": 0, "l2norm": 0, "sdpa": calls}
    assert counts == want, counts
    rels = []
    for si in range(len(ARCH.patch_nums)):
        pos = torch.from_numpy(d[f"pos{si}"]).to(dev)
        ref = torch.from_numpy(d[f"logit_sub{si}"].astype(np.float32)).to(dev)
        rels.append(float((logits[si][0][:, pos] - ref).norm() / ref.norm()))
    fh = torch.from_numpy(d["f_hat"]).to(dev)
    img = (gen.vae.fhat_to_img(f_hat).float() + 1) * 0.5
    err = (img.clamp(0, 1) - torch.from_numpy(d["image"].astype(np.float32)).to(dev)).abs()
    print(f"[var parity, {'native' if use_kernel else 'torch'} attention] worst logit rel {max(rels):.4f} per scale "
          f"{[round(r, 4) for r in rels]}  image max {float(err.max()):.4f} mean {float(err.mean()):.5f}")
    assert max(rels) < LOGIT_REL, rels
    assert float((f_hat - fh).abs().max()) < FHAT_ABS
    assert float(err.max()) < IMAGE_ABS and float(err.mean()) < IMAGE_MEAN


def test_var_native_free_generation_deterministic(golden, dev, monkeypatch):
    """Free-running population generation on the native path: bitwise equal run to run, identical theta rows give
    identical images per member."""
    d = golden("g11_var_model.npz")
    gen, theta = _build(dev, d["theta"])
    assert gen.infer.use_kernel
    pop = theta[None].repeat(2, 1).contiguous()
    labels = torch.tensor([3, 980, 3, 980], device=dev)
    counts = _spies(monkeypatch)
    a = gen.generate_population(labels, pop, seed=7, guidance_scale=4.0)
    assert counts["flash"] == counts["l2norm"] == ARCH.depth * len(ARCH.patch_nums)
    b = gen.generate_population(labels, pop, seed=7, guidance_scale=4.0)
    assert a.shape == (8, 3, 256, 256) and torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert torch.equal(a[:4], a[4:])


def test_var_backend_torch_attention_still_generates(dev, monkeypatch):
    """VarConfig.native_attention reaches the generator; with it off the torch path generates."""
    from hyperscalees_t2i_amd.backend import VarBackend, VarConfig
    for flag in (False, True):
        be = VarBackend(str(dev), VarConfig(arch=ARCH, classes_per_gen=2, batches_per_gen=2, ckpt_dir="/nonexistent",
                                            synthetic_if_missing=True, native_attention=flag))
        be.init_and_attach_lora()
        assert be.es_model.infer.use_kernel is flag
    assert VarConfig().native_attention is True
    be = VarBackend(str(dev), VarConfig(arch=ARCH, classes_per_gen=2, batches_per_gen=2, ckpt_dir="/nonexistent",
                                        synthetic_if_missing=True, native_attention=False))
    be.init_and_attach_lora()
    counts = _spies(monkeypatch)
    imgs, _ = be.es_model.generate(seed=3, guidance_scale=4.0, class_ids=[3, 980], output_type="pt")
    assert counts["flash"] == 0 and counts["l2norm"] == 0 and counts["sdpa"] >= ARCH.depth * len(ARCH.patch_nums)
    assert imgs.shape == (2, 3, 256, 256) and torch.isfinite(imgs).all()
