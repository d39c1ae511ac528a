"""Numpy restatement of the packed int16 series format (include/nlam_hip.h, "Resident series as PACKED int16").

Everything is float32 arithmetic with one rounding per operation, which numpy gives on float32 arrays:
  decode   x = float32(q) * scale[f] + offset[f]                                  (product rounded, then the sum)
  encode   q = clip(rint((x - offset[f]) / scale[f]), -32767, 32767)              (rint: to nearest even)
  tables   offset = fp32((max + min) / 2), scale = fp32((max - min) / 65534), both computed in float64;
           a constant feature (and a range whose scale underflows fp32): scale = 1, offset = the value
The feature axis is the last one.
"""
import numpy as np

QMAX = 32767


def default_tables(x):
    """(scale, offset), float32 (F,), from the exact per-feature range of ``x`` (..., F)."""
    flat = np.asarray(x, dtype=np.float32).reshape(-1, np.shape(x)[-1])
    lo, hi = flat.min(axis=0).astype(np.float64), flat.max(axis=0).astype(np.float64)
    offset = ((hi + lo) / 2).astype(np.float32)
    scale = ((hi - lo) / (2 * QMAX)).astype(np.float32)
    for f in range(flat.shape[1]):
        if not scale[f] > 0:
            scale[f] = 1.0
            if hi[f] == lo[f]:
                offset[f] = np.float32(lo[f])
    return scale, offset


def encode(x, scale, offset):
    x = np.asarray(x, dtype=np.float32)
    scale, offset = np.asarray(scale, dtype=np.float32), np.asarray(offset, dtype=np.float32)
    q = np.rint((x - offset) / scale)
    assert q.dtype == np.float32
    return np.clip(q, -QMAX, QMAX).astype(np.int16)


def decode(q, scale, offset):
    scale, offset = np.asarray(scale, dtype=np.float32), np.asarray(offset, dtype=np.float32)
    out = np.asarray(q).astype(np.float32) * scale + offset
    assert out.dtype == np.float32
    return out


def roundtrip_bound(x, scale, offset):
    """Per element: half a level, plus the four fp32 roundings (sub, div, mul, add) and the clamp at the ends, with slack."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    scale, offset = np.asarray(scale, dtype=np.float64), np.asarray(offset, dtype=np.float64)
    return 0.5 * scale + 8 * 2.0 ** -24 * (x + np.abs(offset) + QMAX * scale)
