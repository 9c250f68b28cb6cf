"""GGUF files: the container, ggml block dequantisation, and the one quantiser (Q8_0) the round trips need.

Reference: ZImageTurboES(use_quantize=True, gguf_local_path=...) loads the Z-Image transformer from a GGUF file
through diffusers' `GGUFQuantizationConfig` (models/zImageTurbo.py:76-94,140-193), which keeps the blocks and
dequantises in every forward.  This build dequantises ONCE at load, to the bf16 weights every kernel already
runs on (checkpoints.read_gguf_state): on the GPU by eggroll_gguf_dequant (kernels.gguf_dequant), on the CPU by
`dequantize_numpy`.

Written from the published format (the GGUF container of ggml: little-endian header, metadata key-values,
tensor infos, an aligned data section) and ggml's block layouts and dequantisation expressions for F32, F16,
BF16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K and Q6_K.  Neither the Python `gguf` package nor
llama.cpp nor diffusers is importable here and no real GGUF file exists offline: the reader is pinned only
against this module's own writer and against the independent packer + closed-form values of tests/test_gguf.py
— PARITY WITH REAL GGUF FILES AND WITH DIFFUSERS' GGUFQuantizationConfig PATH IS UNPINNED.

Every multiply / add / subtract of a dequantisation is rounded to fp32 in ggml's written order (no FMA), fp16
fields widen exactly; the GPU kernel produces the same bits.
"""
from __future__ import annotations

import struct
import warnings
from pathlib import Path
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

GGUF_MAGIC = 0x46554747   # "GGUF"
DEFAULT_ALIGNMENT = 32

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 0, 1, 2, 3, 6, 7, 8
Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, BF16 = 10, 11, 12, 13, 14, 30

# ggml type id -> (name, elements per block, bytes per block)
GGML_TYPES: Dict[int, Tuple[str, int, int]] = {
    F32: ("F32", 1, 4), F16: ("F16", 1, 2), Q4_0: ("Q4_0", 32, 18), Q4_1: ("Q4_1", 32, 20), Q5_0: ("Q5_0", 32, 22),
    Q5_1: ("Q5_1", 32, 24), Q8_0: ("Q8_0", 32, 34), Q2_K: ("Q2_K", 256, 84), Q3_K: ("Q3_K", 256, 110),
    Q4_K: ("Q4_K", 256, 144), Q5_K: ("Q5_K", 256, 176), Q6_K: ("Q6_K", 256, 210), BF16: ("BF16", 1, 2),
}
PLAIN_DTYPES = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}

# metadata value types
U8, I8, U16, I16, U32, I32, FLOAT32, BOOL, STRING, ARRAY, U64, I64, FLOAT64 = range(13)
_SCALAR_FMT = {U8: "<B", I8: "<b", U16: "<H", I16: "<h", U32: "<I", I32: "<i", FLOAT32: "<f", BOOL: "<?",
               U64: "<Q", I64: "<q", FLOAT64: "<d"}


def type_name(ggml_type: int) -> str:
    return GGML_TYPES[ggml_type][0] if ggml_type in GGML_TYPES else f"type{ggml_type}"


def tensor_nbytes(ggml_type: int, n_elems: int) -> int:
    _, be, ts = GGML_TYPES[ggml_type]
    if n_elems % be:
        raise ValueError(f"{n_elems} elements are not a multiple of the {type_name(ggml_type)} block size {be}")
    return n_elems // be * ts


# ---------------------------------------------------------------------------------------
# container
# ---------------------------------------------------------------------------------------


class _Cursor:
    def __init__(self, buf, name: str):
        self.buf, self.pos, self.name = buf, 0, name

    def take(self, n: int) -> bytes:
        if n < 0 or self.pos + n > len(self.buf):
            raise ValueError(f"{self.name}: truncated GGUF file (wanted {n} bytes at offset {self.pos} of "
                             f"{len(self.buf)})")
        b = bytes(self.buf[self.pos:self.pos + n])
        self.pos += n
        return b

    def scalar(self, vt: int):
        fmt = _SCALAR_FMT[vt]
        return struct.unpack(fmt, self.take(struct.calcsize(fmt)))[0]

    def string(self) -> str:
        return self.take(self.scalar(U64)).decode("utf-8")

    def value(self, vt: int):
        """(python value, type tag): the tag is vt, or (ARRAY, element type) for an array."""
        if vt == STRING:
            return self.string(), vt
        if vt == ARRAY:
            et, n = self.scalar(U32), self.scalar(U64)
            if et == ARRAY or (et != STRING and et not in _SCALAR_FMT):
                raise ValueError(f"{self.name}: metadata array of element type {et} is not supported")
            return [self.value(et)[0] for _ in range(n)], (ARRAY, et)
        if vt not in _SCALAR_FMT:
            raise ValueError(f"{self.name}: metadata value type {vt} is not a GGUF value type")
        return self.scalar(vt), vt


class GGUFFile:
    """A GGUF v2 / v3 file opened lazily (np.memmap): `.metadata` {key: value}, `.metadata_types` {key: value
    type id, or (ARRAY, element type)}, `.alignment`, and `.tensors` {name: (ggml_type, torch_shape, raw_bytes)}
    with torch_shape the GGUF dims reversed (GGUF lists the contiguous dimension first) and raw_bytes a uint8
    view of the mapping.  Anything malformed raises ValueError naming the file."""

    def __init__(self, path):
        self.path = Path(path)
        name = str(self.path)
        self._mm = np.memmap(self.path, dtype=np.uint8, mode="r")
        c = _Cursor(self._mm, name)
        magic = struct.unpack("<I", c.take(4))[0]
        if magic != GGUF_MAGIC:
            raise ValueError(f"{name}: not a GGUF file (magic 0x{magic:08x}, expected 0x{GGUF_MAGIC:08x})")
        self.version = c.scalar(U32)
        if self.version not in (2, 3):
            raise ValueError(f"{name}: GGUF version {self.version} is not supported (2 or 3)")
        n_tensors, n_kv = c.scalar(U64), c.scalar(U64)
        self.metadata: Dict[str, Any] = {}
        self.metadata_types: Dict[str, Any] = {}
        for _ in range(n_kv):
            key = c.string()
            self.metadata[key], self.metadata_types[key] = c.value(c.scalar(U32))
        self.alignment = int(self.metadata.get("general.alignment", DEFAULT_ALIGNMENT))
        if self.alignment < 1:
            raise ValueError(f"{name}: general.alignment {self.alignment}")
        infos = []
        for _ in range(n_tensors):
            tname = c.string()
            nd = c.scalar(U32)
            dims = [c.scalar(U64) for _ in range(nd)]
            infos.append((tname, dims, c.scalar(U32), c.scalar(U64)))
        self.data_start = -(-c.pos // self.alignment) * self.alignment
        self.tensors: Dict[str, Tuple[int, Tuple[int, ...], np.ndarray]] = {}
        for tname, dims, gt, off in infos:
            if gt not in GGML_TYPES:
                raise ValueError(f"{name}: tensor {tname!r} has ggml type {gt}, which is not supported "
                                 f"({', '.join(f'{v[0]} {k}' for k, v in GGML_TYPES.items())})")
            _, be, ts = GGML_TYPES[gt]
            row = dims[0] if dims else 1
            if row % be:
                raise ValueError(f"{name}: tensor {tname!r} ({type_name(gt)}) has rows of {row} elements, not a "
                                 f"multiple of the block size {be}")
            if off % self.alignment:
                raise ValueError(f"{name}: tensor {tname!r} starts at offset {off}, not a multiple of the alignment "
                                 f"{self.alignment}")
            n = 1
            for d in dims:
                n *= d
            lo = self.data_start + off
            hi = lo + n // be * ts
            if hi > len(self._mm):
                raise ValueError(f"{name}: tensor {tname!r} ends at byte {hi}, past the end of the file "
                                 f"({len(self._mm)} bytes)")
            if tname in self.tensors:
                raise ValueError(f"{name}: tensor {tname!r} is listed twice")
            self.tensors[tname] = (gt, tuple(int(d) for d in reversed(dims)), self._mm[lo:hi])

    def type_counts(self) -> Dict[str, int]:
        """{type name: number of tensors}, most frequent first."""
        out: Dict[str, int] = {}
        for gt, _, _ in self.tensors.values():
            out[type_name(gt)] = out.get(type_name(gt), 0) + 1
        return dict(sorted(out.items(), key=lambda kv: (-kv[1], kv[0])))


def _pack_string(s: str) -> bytes:
    b = s.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


def _infer_value_type(v) -> Any:
    if isinstance(v, bool):
        return BOOL
    if isinstance(v, int):
        return I64 if v < 0 else U32 if v < 2 ** 32 else U64
    if isinstance(v, float):
        return FLOAT32
    if isinstance(v, str):
        return STRING
    if isinstance(v, (list, tuple)):
        if not v:
            raise ValueError("an empty metadata array needs an explicit (ARRAY, element type) tag")
        return (ARRAY, _infer_value_type(v[0]))
    raise ValueError(f"no GGUF value type for {type(v).__name__}")


def _pack_value(v, vt) -> bytes:
    if isinstance(vt, tuple):
        et = vt[1]
        return struct.pack("<IQ", et, len(v)) + b"".join(_pack_value(x, et) for x in v)
    if vt == STRING:
        return _pack_string(v)
    return struct.pack(_SCALAR_FMT[vt], v)


def write_gguf(path, tensors: Dict[str, Tuple[int, Sequence[int], np.ndarray]], metadata: Optional[Dict[str, Any]] = None,
               alignment: int = DEFAULT_ALIGNMENT, metadata_types: Optional[Dict[str, Any]] = None,
               version: int = 3) -> None:
    """The inverse of GGUFFile: name -> (ggml_type, torch_shape, raw uint8 array) and a metadata dict.  A value's
    GGUF type comes from metadata_types[key] (a value type id, or (ARRAY, element type)) when given, else from
    the Python value (bool, u32 / u64 / i64 by range, f32, string, a list of those).  A non-default alignment is
    recorded as general.alignment (u32)."""
    meta = dict(metadata or {})
    types = dict(metadata_types or {})
    if alignment != DEFAULT_ALIGNMENT or "general.alignment" in meta:
        meta["general.alignment"] = int(alignment)
        types["general.alignment"] = U32
    head = struct.pack("<IIQQ", GGUF_MAGIC, version, len(tensors), len(meta))
    for k, v in meta.items():
        vt = types.get(k, None)
        vt = _infer_value_type(v) if vt is None else vt
        head += _pack_string(k) + struct.pack("<I", ARRAY if isinstance(vt, tuple) else vt) + _pack_value(v, vt)
    off, offsets = 0, []
    for name, (gt, shape, raw) in tensors.items():
        n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
        raw = np.asarray(raw)
        if raw.dtype != np.uint8 or raw.size != tensor_nbytes(gt, n):
            raise ValueError(f"write_gguf: {name!r} ({type_name(gt)}, {tuple(shape)}) needs {tensor_nbytes(gt, n)} "
                             f"uint8 bytes, got {raw.size} of {raw.dtype}")
        offsets.append(off)
        off = -(-(off + raw.size) // alignment) * alignment
    for (name, (gt, shape, _)), o in zip(tensors.items(), offsets):
        dims = list(reversed([int(d) for d in shape]))
        head += _pack_string(name) + struct.pack("<I", len(dims)) + b"".join(struct.pack("<Q", d) for d in dims)
        head += struct.pack("<IQ", gt, o)
    with open(path, "wb") as f:
        f.write(head)
        f.write(b"\0" * (-len(head) % alignment))
        for (_, (_, _, raw)), o in zip(tensors.items(), offsets):
            b = np.ascontiguousarray(raw).tobytes()
            f.write(b)
            f.write(b"\0" * (-len(b) % alignment))


# ---------------------------------------------------------------------------------------
# dequantisation on the CPU (numpy, fp32, ggml's order of operations)
# ---------------------------------------------------------------------------------------

_f32 = np.float32


def _half(blk: np.ndarray, off: int) -> np.ndarray:
    """The fp16 field at byte `off` of every block -> fp32 [nb, 1] (exact)."""
    return np.ascontiguousarray(blk[:, off:off + 2]).view("<f2").astype(_f32)


def _k4_scale_min(s: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The eight 6-bit (scale, min) pairs of the 12 packed bytes of Q4_K / Q5_K: [nb, 12] -> 2 x [nb, 8]."""
    sc = np.concatenate([s[:, 0:4] & 63, (s[:, 8:12] & 15) | ((s[:, 0:4] >> 6) << 4)], 1)
    mn = np.concatenate([s[:, 4:8] & 63, (s[:, 8:12] >> 4) | ((s[:, 4:8] >> 6) << 4)], 1)
    return sc, mn


def _crumbs(qs: np.ndarray) -> np.ndarray:
    """Q2_K / Q3_K: [nb, 64] bytes -> the 256 2-bit values in element order (two 128-element halves, each four
    shifts of its 32 bytes)."""
    nb = qs.shape[0]
    sh = np.array([0, 2, 4, 6], dtype=np.uint8).reshape(1, 1, 4, 1)
    return ((qs.reshape(nb, 2, 1, 32) >> sh) & 3).reshape(nb, 256)


def _bit_planes(qh: np.ndarray) -> np.ndarray:
    """[nb, 32] bytes -> bit j of byte l at element 32 j + l: [nb, 256]."""
    nb = qh.shape[0]
    sh = np.arange(8, dtype=np.uint8).reshape(1, 8, 1)
    return ((qh.reshape(nb, 1, 32) >> sh) & 1).reshape(nb, 256)


def _nibbles(qs: np.ndarray, group: int) -> np.ndarray:
    """[nb, n] bytes -> per `group` bytes, their low nibbles then their high nibbles: [nb, 2 n]."""
    nb, n = qs.shape
    sh = np.array([0, 4], dtype=np.uint8).reshape(1, 1, 2, 1)
    return ((qs.reshape(nb, n // group, 1, group) >> sh) & 15).reshape(nb, 2 * n)


def dequantize_numpy(raw, ggml_type: int, n_elems: int) -> np.ndarray:
    """n_elems values of `ggml_type` from their raw bytes -> float32 [n_elems]."""
    if ggml_type not in GGML_TYPES:
        raise ValueError(f"ggml type {ggml_type} is not supported")
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8)).reshape(-1)
    name, be, ts = GGML_TYPES[ggml_type]
    if n_elems < 0 or n_elems % be or raw.size != n_elems // be * ts:
        raise ValueError(f"dequantize_numpy: {raw.size} bytes for {n_elems} {name} elements "
                         f"({be} per {ts}-byte block)")
    if ggml_type == F32:
        return raw.view("<f4").astype(_f32)
    if ggml_type == F16:
        return raw.view("<f2").astype(_f32)
    if ggml_type == BF16:
        return (raw.view("<u2").astype(np.uint32) << 16).view(_f32)
    nb = n_elems // be
    blk = raw.reshape(nb, ts)
    if ggml_type in (Q4_0, Q4_1, Q5_0, Q5_1):
        has_m, has_h = ggml_type in (Q4_1, Q5_1), ggml_type in (Q5_0, Q5_1)
        p = 4 if has_m else 2
        d = _half(blk, 0)
        q = _nibbles(blk[:, p + (4 if has_h else 0):], 16).astype(np.int32)
        if has_h:
            qh = np.ascontiguousarray(blk[:, p:p + 4]).view("<u4")                          # [nb, 1]
            q |= (((qh >> np.arange(32, dtype=np.uint32)[None, :]) & 1) << 4).astype(np.int32)
        if has_m:
            return (q.astype(_f32) * d + _half(blk, 2)).reshape(-1)
        return ((q - (16 if has_h else 8)).astype(_f32) * d).reshape(-1)
    if ggml_type == Q8_0:
        return (blk[:, 2:].view(np.int8).astype(_f32) * _half(blk, 0)).reshape(-1)
    if ggml_type == Q2_K:
        sc = blk[:, 0:16]
        dl = _half(blk, 80) * (sc & 15).astype(_f32)                                        # [nb, 16]
        ml = _half(blk, 82) * (sc >> 4).astype(_f32)
        q = _crumbs(blk[:, 16:80]).reshape(nb, 16, 16).astype(_f32)
        return (dl[:, :, None] * q - ml[:, :, None]).reshape(-1)
    if ggml_type == Q3_K:
        # the sixteen 6-bit scales, unpacked as ggml does on four 32-bit words
        aux = np.ascontiguousarray(blk[:, 96:108]).view("<u4")
        k1, k2 = np.uint32(0x03030303), np.uint32(0x0F0F0F0F)
        a0, a1, tmp = aux[:, 0], aux[:, 1], aux[:, 2]
        words = np.stack([(a0 & k2) | (((tmp >> 0) & k1) << 4), (a1 & k2) | (((tmp >> 2) & k1) << 4),
                          ((a0 >> 4) & k2) | (((tmp >> 4) & k1) << 4), ((a1 >> 4) & k2) | (((tmp >> 6) & k1) << 4)], 1)
        sc = np.ascontiguousarray(words.astype("<u4")).view(np.uint8).astype(np.int32) - 32  # [nb, 16]
        dl = _half(blk, 108) * sc.astype(_f32)
        q = _crumbs(blk[:, 32:96]).astype(np.int32) - np.where(_bit_planes(blk[:, 0:32]) != 0, 0, 4)
        return (dl[:, :, None] * q.reshape(nb, 16, 16).astype(_f32)).reshape(-1)
    if ggml_type in (Q4_K, Q5_K):
        sc, mn = _k4_scale_min(blk[:, 4:16])
        dl = _half(blk, 0) * sc.astype(_f32)                                                # [nb, 8]
        ml = _half(blk, 2) * mn.astype(_f32)
        if ggml_type == Q4_K:
            q = _nibbles(blk[:, 16:144], 32).astype(np.int32)
        else:
            q = _nibbles(blk[:, 48:176], 32).astype(np.int32) + (_bit_planes(blk[:, 16:48]).astype(np.int32) << 4)
        return (dl[:, :, None] * q.reshape(nb, 8, 32).astype(_f32) - ml[:, :, None]).reshape(-1)
    # Q6_K
    ql = _nibbles(blk[:, 0:128], 64).astype(np.int32)
    sh = np.array([0, 2, 4, 6], dtype=np.uint8).reshape(1, 1, 4, 1)
    qh = ((blk[:, 128:192].reshape(nb, 2, 1, 32) >> sh) & 3).reshape(nb, 256).astype(np.int32)
    q = (ql | (qh << 4)) - 32
    dl = _half(blk, 208) * blk[:, 192:208].view(np.int8).astype(_f32)                       # [nb, 16]
    return (dl[:, :, None] * q.reshape(nb, 16, 16).astype(_f32)).reshape(-1)


def quantize_q8_0(x: np.ndarray) -> np.ndarray:
    """float32 [...] (a multiple of 32 elements) -> Q8_0 bytes: per block of 32, d = fp16(amax / 127),
    q = rint(x / f32(d)) clipped to +-127, and q = 0 where d == 0."""
    x = np.ascontiguousarray(x, dtype=_f32).reshape(-1)
    if x.size % 32:
        raise ValueError(f"quantize_q8_0: {x.size} elements are not a multiple of 32")
    x = x.reshape(-1, 32)
    d = (np.abs(x).max(axis=1, keepdims=True) / _f32(127.0)).astype(np.float16)
    df = d.astype(_f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(df == 0, _f32(0), np.rint(x / df))
    out = np.empty((x.shape[0], 34), dtype=np.uint8)
    out[:, 0:2] = d.astype("<f2").view(np.uint8).reshape(-1, 2)
    out[:, 2:] = np.clip(q, -127, 127).astype(np.int8).view(np.uint8)
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------
# torch front end
# ---------------------------------------------------------------------------------------


def _upload(raw: np.ndarray, device) -> torch.Tensor:
    with warnings.catch_warnings():   # a read-only mapping: torch warns about writes that never happen
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(np.asarray(raw)).to(device)


def dequantize(raw, ggml_type: int, shape: Sequence[int], device="cpu") -> torch.Tensor:
    """One tensor: F32 / F16 / BF16 keep their dtype, quantised types come back as bf16 (round-to-nearest-even
    of the fp32 value).  On a CUDA device the blocks are uploaded and decoded by eggroll_gguf_dequant; on the
    CPU by dequantize_numpy."""
    if ggml_type not in GGML_TYPES:
        raise ValueError(f"ggml type {ggml_type} is not supported")
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    dev = torch.device(device)
    raw = np.asarray(raw).reshape(-1) if not isinstance(raw, torch.Tensor) else raw.reshape(-1)
    if raw.dtype not in (np.uint8, torch.uint8) or raw.shape[0] != tensor_nbytes(ggml_type, n):
        raise ValueError(f"dequantize: {raw.shape[0]} bytes of {raw.dtype} for {n} {type_name(ggml_type)} elements")
    if ggml_type in PLAIN_DTYPES:
        t = raw.to(dev) if isinstance(raw, torch.Tensor) else (_upload(raw, dev) if dev.type != "cpu"
                                                               else torch.from_numpy(np.array(raw)))
        return t.view(PLAIN_DTYPES[ggml_type]).reshape(shape)
    if dev.type == "cuda":
        from . import kernels as K
        t = raw.to(dev) if isinstance(raw, torch.Tensor) else _upload(raw, dev)
        return K.gguf_dequant(t, ggml_type, n).reshape(shape)
    host = raw.cpu().numpy() if isinstance(raw, torch.Tensor) else raw
    return torch.from_numpy(dequantize_numpy(host, ggml_type, n)).to(torch.bfloat16).reshape(shape).to(dev)
