"""GGUF on the CPU: the numpy dequantiser of every supported ggml type against the packer + closed-form values
of tests/gguf_pack.py (bit-exact), the container round trip and its error cases, the Q8_0 quantiser's error
bound, the Z-Image transformer saved as GGUF and loaded back (both naming schemes, strict), the backend built
from a GGUF file plus a config-only transformer directory, and the C-ABI argument checks of
eggroll_gguf_dequant.  No real GGUF file and no gguf package exist offline: parity with them is unpinned."""
import json
import struct

import numpy as np
import pytest
import torch

from hyperscalees_t2i_amd import _lib
from hyperscalees_t2i_amd import checkpoints as ck
from hyperscalees_t2i_amd import gguf as G
from hyperscalees_t2i_amd.backend import ZImageBackend, ZImageConfig
from hyperscalees_t2i_amd.flux_vae import FluxVAEDecoder
from hyperscalees_t2i_amd.zimage import ZImageArch, ZImageTransformer2DModel
from tests import gguf_pack as P

TINY = ZImageArch(dim=256, n_layers=2, n_refiner_layers=1, n_heads=2, ffn=512, cap_feat_dim=256, t_mid=256,
                  seq_multiple=16)
# what a config.json can say (ffn = int(dim / 3 * 8), t_mid 1024): every inner dimension a multiple of 32
CFG_ARCH = ZImageArch(dim=384, n_layers=2, n_refiner_layers=1, n_heads=3, ffn=1024, cap_feat_dim=256, t_mid=1024)


# ---- per-type dequantisation ---------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 7, 33])
@pytest.mark.parametrize("t", P.ALL_TYPES, ids=[G.type_name(t) for t in P.ALL_TYPES])
def test_dequantize_numpy_equals_formula(t, nb):
    raw, want = P.case(t, nb, seed=1000 * t + nb)
    assert raw.dtype == np.uint8 and raw.size == nb * G.GGML_TYPES[t][2]
    got = G.dequantize_numpy(raw, t, P.n_elems(t, nb))
    assert got.dtype == np.float32 and np.isfinite(want).all()
    assert np.array_equal(got, want)


def test_fields_cover_their_ranges():
    """The 33-block cases hold every value of every 6-bit scale, every Q5 / Q6 quant and every fp16 field."""
    rng = np.random.default_rng(0)
    for t, key, n in ((G.Q3_K, "sc", 64), (G.Q4_K, "sc", 64), (G.Q4_K, "mn", 64), (G.Q5_K, "sc", 64), (G.Q5_K, "q", 32),
                      (G.Q6_K, "q", 64), (G.Q6_K, "sc", 256), (G.Q5_0, "q", 32), (G.Q8_0, "q", 256)):
        assert len(np.unique(P.random_fields(t, 33, rng)[key])) == n, (t, key)
    assert len(np.unique(P.random_fields(G.Q4_K, 33, rng)["d"].view(np.uint16))) == len(P.HALF_VALUES)


def test_q3k_scale_forms_agree():
    """ggml unpacks the sixteen 6-bit Q3_K scales on 32-bit words; the packer uses the per-element form (low
    nibble of byte j or high nibble of byte j - 8, two more bits from byte 8 + j % 4 at 2 (j // 4))."""
    rng = np.random.default_rng(3)
    for _ in range(200):
        b = rng.integers(0, 256, 12).astype(np.uint8)
        per = [((b[j] & 15) if j < 8 else (b[j - 8] >> 4)) | (((b[8 + j % 4] >> (2 * (j // 4))) & 3) << 4)
               for j in range(16)]
        a0, a1, tmp = (int(x) for x in b.view("<u4"))
        k1, k2 = 0x03030303, 0x0F0F0F0F
        words = [(a0 & k2) | (((tmp >> 0) & k1) << 4), (a1 & k2) | (((tmp >> 2) & k1) << 4),
                 ((a0 >> 4) & k2) | (((tmp >> 4) & k1) << 4), ((a1 >> 4) & k2) | (((tmp >> 6) & k1) << 4)]
        assert list(struct.pack("<4I", *words)) == [int(x) for x in per]


def test_dequantize_torch_cpu():
    raw, want = P.case(G.Q4_K, 6, seed=5)
    t = G.dequantize(raw, G.Q4_K, (3, 512), "cpu")
    assert t.dtype == torch.bfloat16 and tuple(t.shape) == (3, 512)
    assert torch.equal(t.reshape(-1), torch.from_numpy(want).to(torch.bfloat16))
    for gt, dt in ((G.F32, torch.float32), (G.F16, torch.float16), (G.BF16, torch.bfloat16)):
        raw, want = P.case(gt, 12, seed=6)
        t = G.dequantize(raw, gt, (3, 4), "cpu")
        assert t.dtype == dt and torch.equal(t.float().reshape(-1), torch.from_numpy(want))
    with pytest.raises(ValueError):
        G.dequantize(raw[:-1], G.BF16, (3, 4), "cpu")
    with pytest.raises(ValueError):
        G.dequantize_numpy(raw, 9, 12)


# ---- container -------------------------------------------------------------------------------------
def _sample_tensors():
    rng = np.random.default_rng(11)
    out = {}
    for name, t, shape in (("blk.0.weight", G.Q4_K, (3, 512)), ("blk.0.bias", G.F32, (7,)), ("emb", G.Q8_0, (2, 5, 64)),
                           ("h", G.F16, (4, 3)), ("b", G.BF16, (5,)), ("w6", G.Q6_K, (1, 256))):
        n = int(np.prod(shape))
        out[name] = (t, shape, P.case(t, n // G.GGML_TYPES[t][1], seed=int(rng.integers(1 << 30)))[0])
    return out


META = {"u8": 200, "i8": -100, "u16": 60000, "i16": -30000, "u32": 4000000000, "i32": -2000000000, "f32": 0.5,
        "flag": True, "general.name": "töst", "names": ["a", "", "βγ"], "ints": [1, -2, 3], "u64": 2 ** 63 + 5,
        "i64": -2 ** 62, "f64": 1.0 / 3.0, "floats": [0.25, -1.5]}
META_TYPES = {"u8": G.U8, "i8": G.I8, "u16": G.U16, "i16": G.I16, "u32": G.U32, "i32": G.I32, "f32": G.FLOAT32,
              "flag": G.BOOL, "general.name": G.STRING, "names": (G.ARRAY, G.STRING), "ints": (G.ARRAY, G.I32),
              "u64": G.U64, "i64": G.I64, "f64": G.FLOAT64, "floats": (G.ARRAY, G.FLOAT32)}


@pytest.mark.parametrize("alignment,version", [(32, 3), (64, 3), (32, 2)])
def test_container_round_trip(tmp_path, alignment, version):
    tensors = _sample_tensors()
    p = tmp_path / "t.gguf"
    G.write_gguf(p, tensors, META, alignment=alignment, metadata_types=META_TYPES, version=version)
    f = G.GGUFFile(p)
    assert f.version == version and f.alignment == alignment and f.data_start % alignment == 0
    meta = dict(META, **({"general.alignment": 64} if alignment == 64 else {}))
    assert f.metadata == meta
    assert {k: v for k, v in f.metadata_types.items() if k != "general.alignment"} == META_TYPES
    assert list(f.tensors) == list(tensors)
    for name, (t, shape, raw) in tensors.items():
        gt, gshape, graw = f.tensors[name]
        assert gt == t and gshape == tuple(shape) and graw.dtype == np.uint8 and np.array_equal(graw, raw)
    assert f.type_counts() == {"BF16": 1, "F16": 1, "F32": 1, "Q4_K": 1, "Q6_K": 1, "Q8_0": 1}


def test_dims_are_stored_innermost_first(tmp_path):
    p = tmp_path / "t.gguf"
    G.write_gguf(p, {"w": (G.F32, (2, 3), np.zeros(24, np.uint8))})
    b = p.read_bytes()
    at = b.index(b"w") + 1                                   # name, then n_dims u32, dims u64 ...
    assert struct.unpack_from("<IQQ", b, at) == (2, 3, 2)


def _info_pos(b: bytes, name: bytes):
    """Byte offsets of (first dim, ggml_type, offset) of a 2-D tensor's info record."""
    at = b.index(struct.pack("<Q", len(name)) + name) + 8 + len(name)
    return at + 4, at + 4 + 16, at + 4 + 16 + 4


def test_container_errors(tmp_path):
    good = tmp_path / "good.gguf"
    G.write_gguf(good, {"a": (G.Q4_K, (2, 256), P.case(G.Q4_K, 2, 1)[0]), "b": (G.Q8_0, (3, 64), P.case(G.Q8_0, 6, 2)[0])})
    G.GGUFFile(good)
    data = good.read_bytes()
    dim_a, type_a, off_a = _info_pos(data, b"a")
    dim_b, type_b, off_b = _info_pos(data, b"b")

    def patched(at, fmt, v, cut=None):
        b = bytearray(data)
        struct.pack_into(fmt, b, at, v)
        p = tmp_path / "bad.gguf"
        p.write_bytes(bytes(b[:cut]))
        return p

    for args, msg in (((0, "<I", 0x46554746), "magic"), ((4, "<I", 1), "version 1"), ((4, "<I", 4), "version 4"),
                      ((type_a, "<I", 9), r"'a' has ggml type 9"),
                      ((type_b, "<I", G.Q4_K), r"'b'.*multiple of the block size 256"),
                      ((off_b, "<Q", 288 + 16), r"'b'.*alignment"), ((off_b, "<Q", 288 + 32), r"'b'.*past the end"),
                      ((0, "<I", G.GGUF_MAGIC, len(data) - 32), r"'b'.*past the end"),
                      ((0, "<I", G.GGUF_MAGIC, 40), "truncated")):
        p = patched(*args)
        with pytest.raises(ValueError, match=msg) as e:
            G.GGUFFile(p)
        assert "bad.gguf" in str(e.value)
    with pytest.raises(ValueError, match="needs 288"):
        G.write_gguf(tmp_path / "x.gguf", {"a": (G.Q4_K, (2, 256), np.zeros(287, np.uint8))})


# ---- Q8_0 quantiser --------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [64, 3840])
def test_q8_0_quantiser_error_bound(cols):
    """Per block |w' - w| <= amax (1/254 + 2^-8): half a step d / 2 = amax / 254, the fp16 rounding of d
    (<= 2^-11 amax on the largest quant), the bf16 rounding of the output (<= 2^-9 amax)."""
    w = torch.randn(5, cols, generator=torch.Generator().manual_seed(cols)).numpy()
    raw = G.quantize_q8_0(w)
    assert raw.size == w.size // 32 * 34
    back = G.dequantize(raw, G.Q8_0, w.shape, "cpu").float().numpy()
    err = np.abs(back - w).reshape(-1, 32).max(1)
    amax = np.abs(w).reshape(-1, 32).max(1)
    print(f"q8_0 cols {cols}: max err / amax {float((err / amax).max()):.3e} (bar {1 / 254 + 2 ** -8:.3e})")
    assert (err <= amax * (1 / 254 + 2.0 ** -8)).all()
    zero = G.quantize_q8_0(np.zeros(32, np.float32))
    assert not zero.any()
    with pytest.raises(ValueError):
        G.quantize_q8_0(np.zeros(33, np.float32))


# ---- the Z-Image transformer through a GGUF file ---------------------------------------------------------
def _expected(p: torch.Tensor) -> torch.Tensor:
    """dequant(quant(p)) computed directly: Q8_0 for a 2-D weight with an inner multiple of 32, else F32."""
    w = p.detach().float().numpy()
    if w.ndim == 2 and w.shape[1] % 32 == 0:
        return torch.from_numpy(G.dequantize_numpy(G.quantize_q8_0(w), G.Q8_0, w.size).reshape(w.shape)).to(p.dtype)
    return p.detach().clone()


@pytest.fixture(scope="module")
def tiny_model():
    m = ZImageTransformer2DModel(TINY)
    m.init_weights(3)
    return m


@pytest.mark.parametrize("single", [False, True])
def test_model_round_trip(tmp_path, tiny_model, single):
    p = tmp_path / "m.gguf"
    ck.save_zimage_gguf(tiny_model, p, single_file_names=single)
    f = G.GGUFFile(p)
    names = list(f.tensors)
    if single:
        assert all(n.startswith("model.diffusion_model.") for n in names)
        assert any(n.endswith(".attention.qkv.weight") for n in names) and not any("to_q" in n for n in names)
        assert "model.diffusion_model.x_embedder.weight" in names and not any("all_" in n for n in names)
        assert any(n.endswith(".attention.q_norm.weight") for n in names)
    else:
        assert set(names) == {n for n, q in tiny_model.named_parameters() if not q.requires_grad}
    counts = f.type_counts()
    assert set(counts) == {"Q8_0", "F32"} and counts["Q8_0"] > 10
    fresh = ZImageTransformer2DModel(TINY)
    ck.load_zimage_transformer_gguf(fresh, p)
    quantised = 0
    for (n, a), (_, b) in zip(tiny_model.named_parameters(), fresh.named_parameters()):
        assert torch.equal(b, _expected(a)), n
        quantised += int(not torch.equal(a, b))
    assert quantised > 10                                   # the Q8_0 tensors really went through the blocks


def test_model_load_is_strict(tmp_path, tiny_model):
    p = tmp_path / "m.gguf"
    ck.save_zimage_gguf(tiny_model, p)
    tensors = dict(G.GGUFFile(p).tensors)
    fresh = ZImageTransformer2DModel(TINY)
    key = "layers.1.feed_forward.w2.weight"

    def write(t):
        G.write_gguf(tmp_path / "bad.gguf", t)
        return tmp_path / "bad.gguf"

    with pytest.raises(ValueError, match="lacks 1 keys"):
        ck.load_zimage_transformer_gguf(fresh, write({k: v for k, v in tensors.items() if k != key}))
    with pytest.raises(ValueError, match="not used"):
        ck.load_zimage_transformer_gguf(fresh, write(dict(tensors, extra=(G.F32, (2,), np.zeros(8, np.uint8)))))
    gt, shape, raw = tensors[key]
    with pytest.raises(ValueError, match="gives"):
        ck.load_zimage_transformer_gguf(fresh, write(dict(tensors, **{key: (gt, (shape[0] // 2, shape[1] * 2), raw)})))


# ---- backend ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gguf_model_dir(tmp_path_factory):
    """(model directory with transformer/config.json only + vae/, GGUF file, the source transformer)."""
    root = tmp_path_factory.mktemp("zimage_gguf")
    src = ZImageTransformer2DModel(CFG_ARCH)
    src.init_weights(5)
    vae = FluxVAEDecoder(widths=(32, 32, 64, 64))
    vae.init_weights(7)
    ck.save_zimage_diffusers(src, vae, root / "model")
    for f in (root / "model" / "transformer").iterdir():
        if f.name != "config.json":
            f.unlink()
    ck.save_zimage_gguf(src, root / "w.gguf", single_file_names=True)
    return root / "model", root / "w.gguf", src


def test_backend_from_gguf(gguf_model_dir):
    model_dir, path, src = gguf_model_dir
    assert [f.name for f in (model_dir / "transformer").iterdir()] == ["config.json"]
    be = ZImageBackend("cpu", ZImageConfig(model_name=str(model_dir), use_gguf=True, gguf_local_path=str(path)))
    be.init_and_attach_lora()
    tr = be.es_model.transformer
    assert json.loads((model_dir / "transformer" / "config.json").read_text())["dim"] == tr.config.dim == 384
    got = {n: p for n, p in tr.named_parameters() if not p.requires_grad}
    want = {n: p for n, p in src.named_parameters() if not p.requires_grad}
    assert set(got) == set(want)
    for n, p in want.items():
        assert torch.equal(got[n], _expected(p)), n
    ws = be.es_model.weights_source
    assert str(path) in ws and "Q8_0×" in ws and "F32×" in ws
    assert len(be.collect_lora_params()[0]) > 0
    # the same file found through gguf_local_dir / gguf_filename
    be2 = ZImageBackend("cpu", ZImageConfig(model_name=str(model_dir), use_gguf=True, gguf_local_dir=str(path.parent),
                                            gguf_filename=path.name))
    be2.init_and_attach_lora()
    assert be2.es_model.gguf_path == path


def test_backend_gguf_errors(gguf_model_dir, tmp_path):
    model_dir, path, _ = gguf_model_dir
    cfg = ZImageConfig(model_name=str(model_dir), use_gguf=True, gguf_local_path=str(tmp_path / "absent.gguf"),
                       gguf_local_dir=str(tmp_path / "cache"), gguf_filename="q.gguf")
    with pytest.raises(FileNotFoundError) as e:
        ZImageBackend("cpu", cfg).init_and_attach_lora()
    assert str(tmp_path / "absent.gguf") in str(e.value) and str(tmp_path / "cache" / "q.gguf") in str(e.value)
    assert "no hub access" in str(e.value)
    cfg = ZImageConfig(model_name=str(model_dir), use_gguf=True, gguf_local_dir=str(tmp_path / "cache"))
    with pytest.raises(FileNotFoundError, match="z_image_turbo-Q3_K_S.gguf"):
        ZImageBackend("cpu", cfg).init_and_attach_lora()
    with pytest.raises(ValueError, match="synthetic_weights"):
        ZImageBackend("cpu", ZImageConfig(use_gguf=True, synthetic_weights=True, gguf_local_path=str(path))).init_and_attach_lora()
    from hyperscalees_t2i_amd.zimage_pipeline import ZImageTurboES
    with pytest.raises(ValueError, match="encode_only"):
        ZImageTurboES(str(model_dir), device="cpu", use_quantize=True, encode_only=True, gguf_local_path=str(path))
    # the flag off: the same directory is what it was before, a transformer directory without weights
    with pytest.raises(FileNotFoundError):
        ZImageBackend("cpu", ZImageConfig(model_name=str(model_dir))).init_and_attach_lora()


def test_config_defaults_follow_the_reference_cli():
    c = ZImageConfig()
    assert (c.use_gguf, c.gguf_repo_id, c.gguf_filename, c.gguf_local_dir, c.gguf_local_path) == \
        (False, "jayn7/Z-Image-Turbo-GGUF", "z_image_turbo-Q3_K_S.gguf", "gguf_cache", None)


# ---- C-ABI ------------------------------------------------------------------------------------------
def test_capi_argument_checks():
    lib = _lib.load()
    p = 4096   # never dereferenced: every call below is refused (or a no-op) before a launch
    for args in ((9, p, 256, p, 0), (0, p, 256, p, 0), (30, p, 256, p, 0), (G.Q4_K, p, 255, p, 0), (G.Q8_0, p, 48, p, 0),
                 (G.Q4_K, p, -256, p, 0), (G.Q4_K, None, 256, p, 0), (G.Q4_K, p, 256, None, 1), (G.Q4_K, p, 256, p, 2)):
        assert lib.eggroll_gguf_dequant(*args, None) == -1, args
        assert b"gguf_dequant" in lib.eggroll_last_error(), args
    assert lib.eggroll_gguf_dequant(G.Q4_K, p, 0, p, 0, None) == 0
    assert lib.eggroll_gguf_dequant(G.Q6_K, None, 0, None, 1, None) == 0
