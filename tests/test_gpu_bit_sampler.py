"""eggroll_sample_bits on the GPU: against the float64 oracle of tests/bit_sampler_oracle.py on its recipe (G1), its
CFG logits bit for bit against the torch chain it replaces (G2), bits and generator states against
ChunkedBitSampler (G3), codes against bits_to_codes (G4), invariance over the launch shape (G5), the closed forms
(G6), bad inputs (G7), nothing written outside the outputs or by a refused call (G8), and Infinity generation end to
end with the native sampler against the torch chain (G9)."""
import re

import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd.infinity import (ChunkedBitDraws, ChunkedBitSampler, InfinityArch, bits_to_codes)
from hyperscalees_t2i_amd.var import BAD_PROBS
from tests import bit_sampler_oracle as BO

pytestmark = pytest.mark.gpu

# (n, B, h, w, d_tok, patchify): one bit pair; odd sizes under one tile; d_tok a multiple of 4 with the pixel shuffle;
# several bits per lane stride; more than one token tile (256 tokens of 64) and image; and, past the issue's five,
# more than one 64-bit pass per token (d_tok 72: 64 + 8, d_tok 128) with a ragged last token tile (81 = 64 + 17)
SHAPES = [(1, 1, 1, 1, 4, 0), (2, 3, 2, 2, 14, 0), (2, 3, 3, 3, 16, 1), (3, 2, 4, 4, 56, 1), (2, 3, 16, 16, 56, 1),
          (1, 2, 9, 9, 72, 1), (2, 1, 9, 9, 128, 0)]
DTYPES = [torch.bfloat16, torch.float32]
PADS = [0, 6]
NAN = float("nan")


def arch_of(d_tok, patchify):
    return InfinityArch(codebook_dim=d_tok // 4 if patchify else d_tok, spatial_patchify=patchify)


def make_head(c, u, d_tok, dtype, pad, dev):
    """cond / uncond [n, B, L * d_tok, 2] fp32 (CPU) -> the head output's layout on the device: rows
    [member][cond | uncond][image][token], columns [bit][class], `pad` more columns of NaN behind each row (never
    read: a read would make the bit bad).  Returns the [rows, 2 * d_tok] view."""
    n, B = c.shape[:2]
    t = torch.stack((c, u), dim=1).reshape(n * 2 * B * (c.shape[2] // d_tok), 2 * d_tok)
    full = torch.full((t.shape[0], 2 * d_tok + pad), NAN)
    full[:, :2 * d_tok] = t
    return full.to(dev, dtype)[:, :2 * d_tok]


def launch(head, q, shape, tau, cfg, top_k, top_p, dev, keep=True):
    n, B, h, w, d, p = shape
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    x = torch.full((n, B, h * w * d, 2), NAN, device=dev) if keep else None
    bits, codes = K.sample_bits(head, q, n, B, h, w, d, tau, cfg, top_k, top_p, bool(p), bad, x_out=x)
    return bits, codes, x, int(bad.item())


def recipe_on(shape, s, dtype, pad, dev):
    n, B, h, w, d, p = shape
    c, u = BO.recipe(s, n, B, h * w * d)
    q = BO.draws((B, h * w * d, 2))
    return c, u, q, make_head(c, u, d, dtype, pad, dev)


def oracle_for(x, q, n, top_k, top_p):
    """x [n, B, bits, 2] (any device), q [B, bits, 2] shared by the members -> the oracle over [n, B, bits]."""
    return BO.oracle(x.cpu(), q.cpu()[None].expand(n, -1, -1, -1).contiguous(), top_k, BO.p_cut_of(top_p))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_g1_against_the_oracle_on_the_recipe(shape, dtype, pad, dev):
    """Every bit admissible, the undecided share under the cap, x_out the fp32 chain of the header evaluated on the
    CPU (the reciprocal form), codes those of the bits: the six (s, tau, cfg) cases of the recipe."""
    n, B, h, w, d, p = shape
    for s, tau, cfg in BO.CASES:
        c, u, q, head = recipe_on(shape, s, dtype, pad, dev)
        bits, codes, x, bad = launch(head, q.to(dev), shape, tau, cfg, BO.TOP_K, BO.TOP_P, dev)
        assert bad == 0
        assert torch.equal(x.cpu(), BO.combine(c, u, tau, cfg, reciprocal=True))
        BO.check(oracle_for(x, q, n, BO.TOP_K, BO.TOP_P), bits.view(n, B, -1), f" G1 {shape} s={s} tau={tau} cfg={cfg}")
        assert torch.equal(codes, bits_to_codes(bits, arch_of(d, p), h, w))


@pytest.mark.parametrize("cfg", [3.0, 1.5, 1.0])
@pytest.mark.parametrize("tau", [1.0, 0.7, 1.7])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_g2_cfg_logits_bit_for_bit_torch(dtype, tau, cfg, dev):
    """x_out == the torch chain of InfinityPopulationInfer.run on the GPU, bitwise.  tau = 0.7 and 1.7 fix the form of
    the division (torch multiplies by float32(1.0 / tau), the reciprocal taken in double: at 1.7 that differs from
    1.0f / float32(tau) in the last bit, and both differ from a true division in many elements)."""
    shape = SHAPES[3]
    n, B, h, w, d, p = shape
    c, u, q, head = recipe_on(shape, 2.0, dtype, 6, dev)
    if dtype == torch.float32:      # not only bf16-valued inputs
        head.add_(torch.randn(head.shape, generator=torch.Generator().manual_seed(1)).to(dev) * 1e-3)
    _, _, x, bad = launch(head, q.to(dev), shape, tau, cfg, 0, 0.0, dev)
    lg = head.float().reshape(n, 2, B, h * w * d, 2) / float(tau)
    ref = cfg * lg[:, 0] + (1.0 - cfg) * lg[:, 1]
    differ = int((x != ref).sum())
    print(f"[G2 {dtype} tau={tau} cfg={cfg}] elements off torch's chain: {differ} of {ref.numel()}")
    assert bad == 0 and torch.equal(x, ref)


@pytest.mark.parametrize("mb", [0, 2, 1])
def test_g3_against_chunked_bit_sampler(mb, dev):
    """Same seed, three consecutive scales from one sampler object each, B = 3 (a ragged last chunk at micro_batch
    2): bits equal at every decided position, per-chunk generator states equal after every scale."""
    n, B, d, p, tau, cfg = 2, 3, 16, 1, 0.7, 1.5
    mbe = B if mb <= 0 or mb >= B else mb
    ref = ChunkedBitSampler(torch.Generator(device=dev).manual_seed(11), B, mbe)
    nat = ChunkedBitDraws(torch.Generator(device=dev).manual_seed(11), B, mbe)
    for si, (h, w) in enumerate(((1, 1), (2, 2), (3, 3))):
        shape = (n, B, h, w, d, p)
        g = torch.Generator().manual_seed(20 + si)
        c = (torch.randn(n, B, h * w * d, 2, generator=g) * 2.0).bfloat16().float()
        u = (torch.randn(n, B, h * w * d, 2, generator=g) * 2.0).bfloat16().float()
        head = make_head(c, u, d, torch.bfloat16, 0, dev)
        q = nat.fill(torch.empty((B, h * w * d, 2), dtype=torch.float32, device=dev))
        bits, _, x, bad = launch(head, q, shape, tau, cfg, BO.TOP_K, BO.TOP_P, dev)
        want = ref.sample(x.clone(), BO.TOP_K, BO.TOP_P)
        o = oracle_for(x, q, n, BO.TOP_K, BO.TOP_P)
        got = bits.view(n, B, -1).cpu()
        und = int((~o["decided"]).sum())
        print(f"[G3 mb={mb} scale {si}] bits {got.numel()}; undecided {und}; differ {int((got != want.cpu()).sum())}")
        assert bad == 0 and und <= BO.CAP * got.numel()
        assert torch.equal(got[o["decided"]], want.cpu()[o["decided"]])
        assert bool(BO.admissible(o, got).all()) and bool(BO.admissible(o, want).all())
        assert list(ref.states) == list(nat.states)
        for c0 in ref.states:
            assert torch.equal(ref.states[c0], nat.states[c0]), (si, c0)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_g4_codes_are_bits_to_codes(shape, pad, dev):
    """Both patchify modes, with both classes drawn everywhere (no masking): codes == bits_to_codes(bits)."""
    n, B, h, w, d, p = shape
    c, u, q, head = recipe_on(shape, 0.5, torch.bfloat16, pad, dev)
    bits, codes, _, bad = launch(head, q.to(dev), shape, 1.0, 1.0, 0, 0.0, dev, keep=False)
    assert bad == 0 and 0 <= int(bits.min()) and int(bits.max()) <= 1
    assert n * B * h * w * d < 64 or (0.2 < bits.float().mean().item() < 0.8)
    ref = bits_to_codes(bits, arch_of(d, p), h, w)
    assert codes.shape == ref.shape and torch.equal(codes, ref)


def test_g5_invariance(dev):
    """An n = 3 launch equals three n = 1 launches bitwise; two members given identical logits get identical bits."""
    shape = SHAPES[3]
    n, B, h, w, d, p = shape
    c, u, q, _ = recipe_on(shape, 2.0, torch.bfloat16, 0, dev)
    c, u = c.clone(), u.clone()
    c[2], u[2] = c[0], u[0]
    head = make_head(c, u, d, torch.bfloat16, 6, dev)
    q = q.to(dev)
    bits, codes, x, _ = launch(head, q, shape, 0.7, 1.5, BO.TOP_K, BO.TOP_P, dev)
    rows = 2 * B * h * w
    for k in range(n):
        b1, c1, x1, _ = launch(head[k * rows:(k + 1) * rows], q, (1,) + shape[1:], 0.7, 1.5, BO.TOP_K, BO.TOP_P, dev)
        assert torch.equal(b1, bits[k * B:(k + 1) * B]) and torch.equal(c1, codes[k * B:(k + 1) * B])
        assert torch.equal(x1[0], x[k])
    assert torch.equal(bits[:B], bits[2 * B:]) and torch.equal(codes[:B], codes[2 * B:])
    assert not torch.equal(bits[:B], bits[B:2 * B])
    again = launch(head, q, shape, 0.7, 1.5, BO.TOP_K, BO.TOP_P, dev)
    assert torch.equal(again[0], bits) and torch.equal(again[1], codes)


def test_g6_closed_forms(dev):
    shape = SHAPES[4]
    n, B, h, w, d, p = shape
    c, u, q, head = recipe_on(shape, 2.0, torch.bfloat16, 0, dev)
    q = q.to(dev)
    # top_k = 1 without top-p: the argmax class wherever the two logits differ
    bits, _, x, _ = launch(head, q, shape, 1.0, 3.0, 1, 0.0, dev)
    b, xs = bits.view(n, B, -1), x
    differ = xs[..., 0] != xs[..., 1]
    assert int(differ.sum()) > 0.9 * differ.numel()
    assert torch.equal(b[differ], (xs[..., 1] > xs[..., 0]).long()[differ])
    # top_p = 0.97: every bit whose float64 p_lo < p_cut - 1e-6 gets the larger logit's class
    bits, _, x, _ = launch(head, q, shape, 1.0, 3.0, BO.TOP_K, 0.97, dev)
    xd = x.double()
    p_lo = torch.sigmoid(-(xd[..., 1] - xd[..., 0]).abs())
    sure = (p_lo < BO.p_cut_of(0.97) - 1e-6) & (xd[..., 0] != xd[..., 1])
    print(f"[G6] surely cut by top-p: {int(sure.sum())} of {sure.numel()}")
    assert int(sure.sum()) > 0.3 * sure.numel()
    assert torch.equal(bits.view(n, B, -1)[sure], (xd[..., 1] > xd[..., 0]).long()[sure])
    # equal logits, whatever top_p (and top_k = 1): drawn by q alone, the lower index on a tie of the two quotients
    ce, ue = c.clone(), u.clone()
    ce[..., 1], ue[..., 1] = ce[..., 0], ue[..., 0]
    heade = make_head(ce, ue, d, torch.bfloat16, 0, dev)
    qc = q.cpu()            # IEEE divisions, as the kernel's
    want = ((0.5 / qc[..., 1]) > (0.5 / qc[..., 0])).long()[None].expand(n, -1, -1).to(dev)
    for top_k, top_p in ((BO.TOP_K, 0.97), (1, 0.999), (0, 0.0)):
        bits, _, x, _ = launch(heade, q, shape, 0.7, 1.5, top_k, top_p, dev)
        assert torch.equal(x[..., 0], x[..., 1])
        assert torch.equal(bits.view(n, B, -1), want), (top_k, top_p)
    assert 0.4 < want.float().mean().item() < 0.6


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_g7_bad_inputs(dtype, dev):
    """A NaN, a +inf or a (-inf, -inf) pair planted in one bit: bits = -1 and codes = 0 there, bad = 1, every other
    bit as in the clean run; a single -inf is an ordinary masked entry."""
    shape = SHAPES[2]
    n, B, h, w, d, p = shape
    c, u, q, head = recipe_on(shape, 2.0, dtype, 6, dev)
    q = q.to(dev)
    clean_bits, clean_codes, clean_x, bad = launch(head, q, shape, 1.0, 3.0, BO.TOP_K, BO.TOP_P, dev)
    assert bad == 0
    inf = float("inf")
    spots = [(0, 1, 5, 0), (1, 2, 100, 1), (1, 0, 143, 0)]                  # (member, image, bit of the image, class)
    for (pc0, pc1), is_bad in (((NAN, None), True), ((inf, None), True), ((None, NAN), True), ((-inf, -inf), True),
                               ((-inf, None), False), ((None, -inf), False)):
        for k, j, e, cls in spots:
            cc = c.clone()
            if pc0 is not None:
                cc[k, j, e, cls] = pc0
            if pc1 is not None:
                cc[k, j, e, 1 - cls] = pc1
            bits, codes, x, bad = launch(make_head(cc, u, d, dtype, 6, dev), q, shape, 1.0, 3.0, BO.TOP_K, BO.TOP_P, dev)
            hit = torch.zeros((n, B, h * w * d), dtype=torch.bool, device=dev)
            hit[k, j, e] = True
            hit_codes = bits_to_codes(hit.view(n * B, h * w, d).long(), arch_of(d, p), h, w) > 0
            b = bits.view(n, B, -1)
            assert torch.equal(b[~hit], clean_bits.view(n, B, -1)[~hit])
            assert torch.equal(codes[~hit_codes], clean_codes[~hit_codes])
            assert torch.equal(x[~hit], clean_x[~hit])
            if is_bad:
                assert bad == 1 and int(b[k, j, e]) == -1 and float(codes[hit_codes]) == 0.0
                assert bool(torch.isnan(x[k, j, e]).all())                  # x_out there is not written either
            else:           # cfg 3 on a cond of -inf: x = -inf in that class, the other class is drawn
                want = (1 - cls) if pc0 is not None else cls
                assert bad == 0 and int(b[k, j, e]) == want and float(x[k, j, e, 1 - want]) == -inf
                assert float(codes[hit_codes]) == (2 * want - 1) * float(clean_codes.abs().max())


def _raw(lib, head, ld, shape, q, bits, codes, x, bad, dev):
    n, B, h, w, d, p = shape
    return lib.eggroll_sample_bits(head.data_ptr(), int(head.dtype == torch.bfloat16), ld, n, B, h, w, d, 1.0, 3.0, -2.0,
                                   0, BO.p_cut_of(0.97), q.data_ptr(), bits.data_ptr(), codes.data_ptr(), p, 0.25,
                                   x.data_ptr(), bad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]], ids=str)
def test_g8_nothing_written_outside_the_outputs(shape, dev):
    """Each output sits inside a poisoned buffer: the guards before and behind it are untouched, every element of
    the output is written; a refused call writes nothing at all."""
    lib = _lib.load()
    n, B, h, w, d, p = shape
    c, u, q, head = recipe_on(shape, 2.0, torch.bfloat16, 6, dev)
    q = q.to(dev)
    total, G = n * B * h * w * d, 64
    bits = torch.full((total + 2 * G,), -7, dtype=torch.int64, device=dev)
    codes = torch.full((total + 2 * G,), 7.0, device=dev)
    x = torch.full((2 * total + 2 * G,), 1e30, device=dev)
    bad = torch.full((1 + 2 * G,), -7, dtype=torch.int32, device=dev)
    args = (q, bits[G:], codes[G:], x[G:], bad[G:], dev)
    # refused: odd ld, ld < 2 d_tok, patchify with an odd d_tok, and (with work to do) a null q
    assert _raw(lib, head, 2 * d + 7, shape, *args) == -1
    assert _raw(lib, head, 2 * d - 2, shape, *args) == -1
    assert _raw(lib, head, 2 * d + 6, (n, B, h, w, d + 1, 1), *args) == -1
    assert lib.eggroll_sample_bits(head.data_ptr(), 1, 2 * d + 6, n, B, h, w, d, 1.0, 3.0, -2.0, 0, -1.0, None,
                                   bits[G:].data_ptr(), codes[G:].data_ptr(), p, 0.25, None, bad[G:].data_ptr(),
                                   None) == -1
    assert b"sample_bits" in lib.eggroll_last_error()
    torch.cuda.synchronize(dev)
    assert bool((bits == -7).all()) and bool((codes == 7.0).all()) and bool((x == 1e30).all()) and bool((bad == -7).all())
    assert _raw(lib, head, 2 * d + 6, shape, *args) == 0
    torch.cuda.synchronize(dev)
    for t, fill, m in ((bits, -7, total), (codes, 7.0, total), (x, 1e30, 2 * total)):
        assert bool((t[:G] == fill).all()) and bool((t[G + m:] == fill).all())
        assert not bool((t[G:G + m] == fill).any())
    assert bool((bad == -7).all())                                          # a clean run does not touch the flag
    want = K.sample_bits(head, q, n, B, h, w, d, 1.0, 3.0, 0, 0.97, bool(p), torch.zeros(1, dtype=torch.int32,
                                                                                          device=dev))
    assert torch.equal(bits[G:G + total], want[0].reshape(-1))
    assert torch.equal(codes[G:G + total], torch.sign(want[1]).reshape(-1) * 0.25)


# ---- G9: end to end on the tiny architecture of tests/test_gpu_infinity.py (restated) ----
def tiny_arch(patchify):
    return InfinityArch(depth=2, embed_dim=256, num_heads=2, block_chunks=2, text_channels=256, codebook_dim=4,
                        spatial_patchify=patchify, vae_widths=(32, 32, 64, 64) if patchify else (32, 32, 64, 64, 64))


@pytest.mark.parametrize("patchify", [1, 0])
def test_g9_generation_end_to_end(patchify, dev):
    """generate_population and generate_one_batch_from_compacts with the native sampler against the torch chain:
    n = 2, B = 3, micro_batch 2 (a ragged chunk).  Scale by scale while the bits agree: the CFG logits are equal
    bitwise, the bits equal at every decided position; images equal when no undecided bit differs.  A NaN planted
    through head.bias raises torch.multinomial's RuntimeError, once, after the last scale."""
    from hyperscalees_t2i_amd.backend import InfinityBackend, InfinityConfig
    from hyperscalees_t2i_amd.es import EggRollNoiser, flatten_params
    cfg = InfinityConfig(synthetic_weights=True, arch=tiny_arch(patchify), pn="0.06M", batches_per_gen=1, micro_batch=2,
                         synthetic_prompt_lens=(5, 40), vae_chunk=8)
    assert cfg.native_sampler
    be = InfinityBackend(str(dev), cfg)
    be.init_and_attach_lora()
    es, a = be.es_model, be.es_model.arch
    assert es.native_sampler is True
    params, shapes = be.collect_lora_params()
    noiser = EggRollNoiser(shapes, sigma=5e-2, lr_scale=0.1, rank=1, use_antithetic=True)
    n, B, seed, mb = 2, 3, 5, 2
    tp = noiser.perturb(flatten_params(params).to(dev), noiser.sample_factors(n, dev, seed=2), n, 0, n)
    kv, lens, idx = [be._dev_kv[0], be._dev_kv[1]], [be.lens_list[0], be.lens_list[1]], torch.tensor([0, 1, 0])
    c = be.cfg

    def compare(run, members):
        """run(native) -> images, with es.last_bits / es.last_logits set (logits from the native run)."""
        es.native_sampler = True
        img_n = run(True)
        bits_n, x_n = es.last_bits, es.last_logits
        es.native_sampler = False
        try:
            img_t = run(False)
        finally:
            es.native_sampler = True
        bits_t, x_t = es.last_bits, es.last_logits
        draws = ChunkedBitDraws(torch.Generator(device=dev).manual_seed(seed), B, mb)
        diverged = False
        for si, (_, h, w) in enumerate(es.scale_schedule):
            q = draws.fill(torch.empty((B, h * w * a.d_tok, 2), dtype=torch.float32, device=dev))
            if x_t:
                assert torch.equal(x_n[si], x_t[si]), si
            o = oracle_for(x_n[si].view(members, B, -1, 2), q, members, c.top_k, c.top_p)
            got, want = bits_n[si].view(members, B, -1).cpu(), bits_t[si].view(members, B, -1).cpu()
            assert bool(BO.admissible(o, got).all()) and int(got.min()) >= 0
            assert torch.equal(got[o["decided"]], want[o["decided"]]), si
            if not torch.equal(got, want):      # an undecided bit fell the other way: the runs part here
                diverged = True
                break
        print(f"[G9 patchify={patchify} members={members}] diverged at an undecided bit: {diverged}")
        if not diverged:
            assert torch.equal(img_n, img_t)
        return img_n

    imgs = compare(lambda native: es.generate_population(kv, lens, idx, tp, seed, c.cfg_list, c.tau_list, c.top_k,
                                                         c.top_p, micro_batch=mb, keep_logits=True), n)
    assert imgs.shape == (n * B, 3, 256, 256) and bool(torch.isfinite(imgs).all())

    def one(native):
        img = es.generate_one_batch_from_compacts(kv_compact_list=[kv[i] for i in idx.tolist()],
                                                  lens_list=[lens[i] for i in idx.tolist()], seed=seed,
                                                  guidance_scale=3.0, cfg_list=c.cfg_list, tau_list=c.tau_list,
                                                  output_type="pt", micro_batch=mb)
        bits = es.last_bits
        if native:      # the same pass once more, for the logits the reference API does not keep
            es._generate(kv, lens, idx.to(dev), 1, seed, c.cfg_list, c.tau_list, c.top_k, c.top_p, mb, None,
                         keep_logits=True)
            assert all(torch.equal(x, y) for x, y in zip(bits, es.last_bits))
        return img
    compare(one, 1)

    head = es.transformer.head
    keep = head.bias.clone()
    try:
        with torch.no_grad():
            head.bias[3] = NAN
        with pytest.raises(RuntimeError, match=re.escape(BAD_PROBS)):
            es.generate_population(kv, lens, idx, tp, seed, c.cfg_list, c.tau_list, c.top_k, c.top_p, micro_batch=mb)
    finally:
        with torch.no_grad():
            head.bias.copy_(keep)
    es.generate_population(kv, lens, idx, tp, seed, c.cfg_list, c.tau_list, c.top_k, c.top_p, micro_batch=mb)
