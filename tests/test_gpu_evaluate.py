"""The evaluation path on the GPU: eggroll_images_to_u8 and eggroll_clip_preprocess_u8 against their references,
bit for bit; RewardModels.score_u8 against score; generate_and_score / evaluate_folder end to end on the tiny Sana
stack of tests/test_gpu_sana_pipeline.py (TINY, 4 x 4 latents = 128 px images) in both backend modes.

Every comparison here is bitwise: the kernels restate integer / per-operation-rounded conversions, PNG is lossless,
and candidates evaluated together or alone run the same member-independent kernels.
"""
import warnings

import numpy as np
import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import evaluate as EV
from hyperscalees_t2i_amd import kernels as K
from hyperscalees_t2i_amd.backend import SanaBackend, SanaConfig
from hyperscalees_t2i_amd.es import flatten_params, unflatten_to_params
from hyperscalees_t2i_amd.infinity_pipeline import images_to_uint8
from hyperscalees_t2i_amd.rewards import RewardModels, clip_pixels, clip_pixels_u8, postprocess_uint8
from hyperscalees_t2i_amd.sana import SanaArch
from hyperscalees_t2i_amd.var import quantize_uint8_var

pytestmark = pytest.mark.gpu

TINY = SanaArch(num_attention_heads=4, attention_head_dim=32, num_layers=2, num_cross_attention_heads=2,
                cross_attention_head_dim=64, caption_channels=2304)
# pil_mode -> the torch expression the kernel restates (uint8-valued fp32 [n, 3, H, W])
TO_U8 = {0: postprocess_uint8, 1: quantize_uint8_var, 2: images_to_uint8}


def reference_u8(x_cpu: torch.Tensor, mode: int) -> torch.Tensor:
    """uint8 [n, H, W, 3] of the torch expression, on the CPU."""
    return TO_U8[mode](x_cpu).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------
# images_to_u8
# ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def all_bf16():
    """Every bf16 bit pattern that is not a NaN (65,282 of them, +-inf included), and for each mode the bytes the
    torch expression gives — which is defined on every one of them: the clamp comes before the integer cast."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    is_nan = ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)
    x = bits[~is_nan].to(torch.int16).view(torch.bfloat16)
    assert x.numel() == 65282 and not bool(torch.isnan(x.float()).any()) and int(torch.isinf(x.float()).sum()) == 2
    want = {}
    for mode, fn in TO_U8.items():
        v = fn(x.view(1, 1, 1, -1))
        assert bool(torch.isfinite(v).all()) and float(v.min()) == 0.0 and float(v.max()) == 255.0
        assert torch.equal(v, v.to(torch.uint8).float())
        want[mode] = v.to(torch.uint8).view(-1)
    return x, want


def padded(x: torch.Tensor, total: int) -> torch.Tensor:
    return torch.cat([x, x[: total - x.numel()]])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_images_to_u8_every_bf16_value(dev, all_bf16, mode):
    x, want = all_bf16
    # (shape, strides the call sees): [1,3,64,352] contiguous takes the 16-byte form; [1,3,37,611] (W % 16 != 0)
    # the per-pixel form
    for shape in ((1, 3, 64, 352), (1, 3, 37, 611)):
        total = int(np.prod(shape))
        xs = padded(x, total).view(shape)
        got = K.images_to_u8(xs.to(dev), mode).cpu()
        ref = padded(want[mode], total).view(shape).permute(0, 2, 3, 1)
        assert got.shape == ref.shape and got.dtype == torch.uint8
        bad = (got != ref).nonzero()
        assert bad.numel() == 0, (mode, shape, bad[:4].tolist())


def _image(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 3, H, W, generator=g) * 0.8).clamp(-1.3, 1.3).to(torch.bfloat16)


LAYOUTS = ["2x3x37", "1x2x64", "batch_slice_3x5x48", "offset_slice_2x5x48", "channels_last_2x5x48", "row_slice_2x6x32"]


def _layout(dev, name):
    """(the device view handed to the kernel, whether it can take the 16-byte form)."""
    if name == "2x3x37":
        return _image(2, 3, 37, 1).to(dev), False                      # W % 16 != 0
    if name == "1x2x64":
        return _image(1, 2, 64, 2).to(dev), True
    if name == "batch_slice_3x5x48":
        return _image(5, 5, 48, 3).to(dev)[::2], True                  # n = 3, image stride doubled
    if name == "offset_slice_2x5x48":
        return _image(3, 5, 48, 4).to(dev)[1:], True                   # starts one image into the allocation
    if name == "channels_last_2x5x48":
        return _image(2, 5, 48, 5).to(dev).contiguous(memory_format=torch.channels_last), False    # sw = 3
    if name == "row_slice_2x6x32":
        return _image(2, 6, 40, 6).to(dev)[:, :, :, 4:36], False       # rows start 8 bytes off a 16-byte boundary
    raise KeyError(name)


@pytest.mark.parametrize("name", LAYOUTS)
def test_images_to_u8_layouts_and_sentinels(dev, name):
    xd, vec = _layout(dev, name)
    n, _, H, W = xd.shape
    sn, sc, sh, sw = xd.stride()
    aligned = sw == 1 and W % 16 == 0 and all(s % 8 == 0 for s in (sn, sc, sh)) and xd.data_ptr() % 16 == 0
    assert aligned == vec, "the layout no longer exercises the form it was chosen for"
    nbytes = n * H * W * 3
    for mode in (0, 1, 2):
        ref = reference_u8(xd.cpu(), mode)
        assert torch.equal(K.images_to_u8(xd, mode).cpu(), ref), (name, mode)
        # straight at the C-ABI with 64 sentinel bytes behind the output
        buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
        _lib.call("eggroll_images_to_u8", xd.data_ptr(), n, H, W, sn, sc, sh, sw, mode, buf.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream)
        host = buf.cpu()
        assert torch.equal(host[:nbytes].view(n, H, W, 3), ref), (name, mode)
        assert bool((host[nbytes:] == 0xA5).all()), (name, mode)


def test_images_to_u8_argument_errors(dev):
    x = _image(1, 2, 16, 9)
    xd = x.to(dev)
    for mode in (-1, 3):
        with pytest.raises(_lib.EggrollError, match="mode"):
            K.images_to_u8(xd, mode)
    with pytest.raises(_lib.EggrollError, match="ROCm"):
        K.images_to_u8(x, 0)                                           # a CPU tensor: no fallback
    with pytest.raises(_lib.EggrollError):
        K.images_to_u8(xd.float(), 0)
    with pytest.raises(_lib.EggrollError, match="3, H, W"):
        K.images_to_u8(xd[:, :2], 0)
    lib = _lib.load()
    out = torch.empty(96, dtype=torch.uint8, device=dev)
    assert lib.eggroll_images_to_u8(None, 1, 2, 16, 96, 32, 16, 1, 0, out.data_ptr(), None) == -1
    assert b"NULL" in lib.eggroll_last_error()
    assert lib.eggroll_images_to_u8(xd.data_ptr(), 1, 2, 16, 96, 32, 16, 1, 0, None, None) == -1
    assert b"NULL" in lib.eggroll_last_error()
    assert lib.eggroll_images_to_u8(xd.data_ptr(), 1, 0, 16, 96, 32, 16, 1, 0, out.data_ptr(), None) == -1
    assert b"sizes" in lib.eggroll_last_error()
    assert lib.eggroll_images_to_u8(xd.data_ptr(), 1 << 40, 1 << 20, 1 << 20, 96, 32, 16, 1, 0, out.data_ptr(), None) == -1
    assert b"grid" in lib.eggroll_last_error()
    assert lib.eggroll_images_to_u8(None, 0, 2, 16, 96, 32, 16, 1, 0, None, None) == 0      # no images: a no-op
    assert K.images_to_u8(xd[:0], 0).shape == (0, 2, 16, 3)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# clip_pixels_u8
# ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,H,W", [(2, 224, 224), (2, 128, 128), (2, 300, 200), (2, 40, 56), (1, 1024, 1024)])
def test_clip_pixels_u8_matches_transformers(dev, n, H, W):
    """Random full-range bytes -> PIL images -> transformers' CLIPImageProcessor (PIL backend), against the same
    bytes on the device, in PIL's HWC layout and as a planar CHW tensor: bitwise."""
    from PIL import Image
    from transformers import CLIPImageProcessorPil
    g = torch.Generator().manual_seed(H * 5 + W)
    u8 = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
    ref = CLIPImageProcessorPil()(images=[Image.fromarray(a) for a in u8.numpy()], return_tensors="pt")
    ref = ref["pixel_values"].numpy()
    hwc = u8.to(dev)
    chw = hwc.permute(0, 3, 1, 2).contiguous()                          # planar storage ...
    assert chw.permute(0, 2, 3, 1).stride()[3] == H * W                 # ... seen as [n, H, W, 3]
    for name, t in (("hwc", hwc), ("chw", chw.permute(0, 2, 3, 1))):
        got = clip_pixels_u8(t).cpu().numpy()
        assert got.shape == ref.shape == (n, 3, 224, 224)
        assert np.array_equal(got, ref), (name, float(np.abs(got - ref).max()))


def test_clip_pixels_u8_matches_bf16_path(dev):
    for shape, seed in (((2, 3, 64, 128), 11), ((2, 3, 97, 301), 12), ((1, 3, 256, 256), 13)):
        x = _image(shape[0], shape[2], shape[3], seed).to(dev)
        for mode in (0, 1, 2):
            a = clip_pixels_u8(K.images_to_u8(x, mode))
            b = clip_pixels(x, mode)
            assert torch.equal(a, b), (shape, mode)
    spec = dict(size=96, mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3))      # another processor's numbers
    assert torch.equal(clip_pixels_u8(K.images_to_u8(x, 0), **spec), clip_pixels(x, 0, **spec))


def test_clip_pixels_u8_argument_errors(dev):
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_lib.EggrollError, match="uint8 ROCm"):
        clip_pixels_u8(u8)
    with pytest.raises(_lib.EggrollError, match="uint8 ROCm"):
        clip_pixels_u8(u8.to(dev).float())
    with pytest.raises(ValueError, match="n,H,W,3"):
        clip_pixels_u8(u8.to(dev).permute(0, 3, 1, 2))
    lib = _lib.load()
    p = u8.to(dev).data_ptr()                                           # any non-NULL pointer: nothing is launched
    assert lib.eggroll_clip_preprocess_u8(p, 1, 8, 4097, 3 * 8 * 4097, 1, 3 * 4097, 3, p, p, 4, 4, 224, 224, 224, p, p,
                                          p, p, None) == -1             # the same width limit as the bf16 path
    assert b"W=4097" in lib.eggroll_last_error()
    assert lib.eggroll_clip_preprocess_u8(None, 1, 8, 8, 192, 1, 24, 3, None, None, 1, 1, 224, 224, 224, None, None,
                                          None, None, None) == -1
    assert b"clip_preprocess_u8" in lib.eggroll_last_error() and b"NULL" in lib.eggroll_last_error()


# ---------------------------------------------------------------------------------------
# score_u8
# ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rewards(dev):
    return RewardModels.build(dev, tiny=True)


def test_score_u8_matches_score(dev, rewards):
    x = _image(5, 64, 96, 21).to(dev)
    feats = rewards.prompt_features(["a red fox", "two cats on a sofa"])
    pidx = torch.tensor([0, 1, 1, 0, 1], device=dev)
    for mode in (0, 1, 2):
        want = rewards.score(x, pidx, feats, pil_mode=mode)
        got = rewards.score_u8(K.images_to_u8(x, mode), pidx, feats)
        assert set(got) == set(want) == set(EV.REWARD_KEYS)
        for k in want:
            assert torch.equal(got[k], want[k]), (mode, k)
    old = rewards.image_batch
    rewards.image_batch = 2                                             # three reward batches
    try:
        a, b = rewards.score(x, pidx, feats), rewards.score_u8(K.images_to_u8(x, 0), pidx, feats)
    finally:
        rewards.image_batch = old
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------

N_PROMPTS = 6


@pytest.fixture(scope="module", params=["one_step", "pipeline"])
def e2e(request, dev, rewards, tmp_path_factory):
    """Everything the end-to-end tests compare, computed once per backend mode."""
    mode = request.param
    cfg = SanaConfig(backend_mode=mode, synthetic_weights=True, width_latent=4, height_latent=4, arch=TINY,
                     vae_widths=(16, 32, 32, 64, 64, 64), vae_layers=(1, 1, 1, 1, 1, 1), synthetic_prompts=N_PROMPTS)
    be = SanaBackend(str(dev), cfg)
    be.init_and_attach_lora()
    root = tmp_path_factory.mktemp(f"eval_{mode}")
    params, shapes = be.collect_lora_params()
    theta = flatten_params(params).clone()
    g = torch.Generator(device=dev).manual_seed(5)
    for k in (1, 2):                                                    # two adapters: theta moved by seeded noise
        unflatten_to_params(theta + 0.05 * k * torch.randn(theta.shape, generator=g, device=dev), params, shapes)
        be.save_lora(root / f"adapter_{k}")
    unflatten_to_params(theta, params, shapes)
    specs = ["base", str(root / "adapter_1"), str(root / "adapter_2")]
    cands = EV.load_candidates(be, specs)
    tsv = root / "prompts.tsv"
    cats, chals = ["A", "B", "A", "C", "B", "A"], ["x", "x", "y", "y", "x", "z"]
    tsv.write_text("Prompt\tCategory\tChallenge\n" + "".join(
        f"{p}\t{c}\t{h}\n" for p, c, h in zip(be.prompts_list, cats, chals)), encoding="utf-8")
    both = EV.generate_and_score(be, rewards, cands, prompts_per_pass=3, out_root=root / "out", keep_images=True)
    alone = [EV.generate_and_score(be, rewards, EV.load_candidates(be, [s]), prompts_per_pass=3, keep_images=True)
             for s in specs]
    one_wide = EV.generate_and_score(be, rewards, cands, prompts_per_pass=1, keep_images=True)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", module=EV.__name__)            # a clean folder: nothing is skipped
        folders = {nm: EV.score_folder(root / "out" / nm, EV.read_prompt_table(tsv), rewards) for nm in both.names}
        report = EV.evaluate_folder(root / "out" / "base", tsv, rewards)
    return dict(be=be, root=root, tsv=tsv, both=both, alone=alone, one_wide=one_wide, folders=folders, report=report)


def test_e2e_shapes_and_files(e2e):
    r = e2e["both"]
    assert r.names == ["base", "adapter_1", "adapter_2"] and r.prompt_ids == list(range(N_PROMPTS))
    assert r.prompts == e2e["be"].prompts_list and r.images.shape == (3, N_PROMPTS, 128, 128, 3)
    for k in EV.REWARD_KEYS:
        assert r.rewards[k].shape == (3, N_PROMPTS) and bool(torch.isfinite(r.rewards[k]).all())
    from PIL import Image
    for c, nm in enumerate(r.names):
        files = sorted(p.name for p in (e2e["root"] / "out" / nm).iterdir())
        assert files == [EV.image_filename(i, p) for i, p in enumerate(r.prompts)]
        with Image.open(e2e["root"] / "out" / nm / files[4]) as im:     # the PNG holds the scored bytes
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), r.images[c, 4].numpy())
    # combined: the evaluation mix, not the training default the reward models carry
    w = EV.DEFAULT_MIX_WEIGHTS
    mix = (w[0] * r.rewards["clip_aesthetic"] + w[1] * r.rewards["clip_text"] + w[2] * r.rewards["no_artifacts"]
           + w[3] * r.rewards["pickscore"])
    assert torch.equal(mix, r.rewards["combined"])


def test_e2e_folder_scores_equal_direct_scores(e2e):
    r = e2e["both"]
    for nm in r.names:
        assert e2e["folders"][nm] == r.entries(nm), nm                  # Python floats of the same fp32 values
    table = EV.read_prompt_table(e2e["tsv"])
    rep = e2e["report"]
    assert rep.format() == r.report("base", table).format() and rep.overall.count == N_PROMPTS
    assert rep.overall.sums == r.report("base", table).overall.sums
    assert {k: v.count for k, v in rep.by_category.items()} == {"A": 3, "B": 2, "C": 1}


def test_e2e_candidates_together_equal_candidates_alone(e2e):
    r = e2e["both"]
    for c, single in enumerate(e2e["alone"]):
        assert single.names == [r.names[c]]
        assert torch.equal(single.images[0], r.images[c]), r.names[c]
        for k in EV.REWARD_KEYS:
            assert torch.equal(single.rewards[k][0], r.rewards[k][c]), (r.names[c], k)


def test_e2e_index_seeds_do_not_depend_on_pass_width(e2e):
    assert torch.equal(e2e["one_wide"].images, e2e["both"].images)


def test_e2e_base_differs_and_compare(e2e):
    r = e2e["both"]
    assert not torch.equal(r.images[0], r.images[1]) and not torch.equal(r.images[1], r.images[2])
    assert not torch.equal(r.images[0, 0], r.images[0, 1])             # per-image seeds and prompts
    same = EV.compare(r, "adapter_1", "adapter_1")
    assert all(v == {"mean_diff": 0.0, "win_rate": 0.0} for v in same.values())
    c = EV.compare(r, "base", "adapter_2")
    d = r.rewards["pickscore"][2].double() - r.rewards["pickscore"][0].double()
    assert c["pickscore"] == {"mean_diff": float(d.mean()), "win_rate": float((d > 0).double().mean())}


def test_e2e_batch_seed_mode_is_the_batched_draw(e2e, dev, rewards):
    """seed_mode="batch": prompts [s, s + b) are one b-image draw from seed s, which is what generate_population
    does without per-image seeds."""
    be = e2e["be"]
    cands = EV.load_candidates(be, ["base"])
    r = EV.generate_and_score(be, rewards, cands, seed_mode="batch", reference_batch_size=4, keep_images=True)
    want = torch.cat([K.images_to_u8(be.generate_population(ids, ids[0], be.cfg.guidance_scale, cands[1]), 0).cpu()
                      for ids in ([0, 1, 2, 3], [4, 5])])
    assert torch.equal(r.images[0], want)
    assert not torch.equal(r.images[0], e2e["both"].images[0])          # not the per-index draws
    sub = EV.generate_and_score(be, rewards, cands, prompt_ids=[4, 1], keep_images=True)
    assert sub.prompt_ids == [4, 1] and torch.equal(sub.images[0], e2e["both"].images[0, [4, 1]])
