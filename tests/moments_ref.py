"""Shared machinery of test_moments_kernels.py: the case records, the series builders, the float64 restatement of the
nlam_window_moments / nlam_window_moments_q16 contract of include/nlam_hip.h with its first-order error bound, a numpy stand-in of
the kernel pair (moments_partials_kernel<DIFF, T>, moments_finish_kernel of csrc/nlam_stats.inc) with injected defects, and the
guarded float64 device buffers.  A plain module; nothing here is collected by pytest.

The contract.  Flat sample idx = first + i, (s, m) = divmod(idx, members); its rows j = row_begin ... row_begin + nrows - 1 are the
(nodes x nvars) blocks at base + s * stride_sample + m * stride_member + j * stride_step.  A packed series is decoded first
(packed_ref.decode: the product rounded, then the sum).  Per feature:
  values      the terms are x over the nrows rows and the nodes; count = nrows * nodes
  difference  used = (nrows // step) * step; sub-offset k takes the rows k, k + step, ... < used; z = (x - mean) / std in float32
              (one sub, one div), d = z[b] - z[a] in float32 for consecutive pairs: the terms are d over pairs and nodes;
              count = (nrows // step - 1) * nodes; output row i * step + k
  out_mean = (sum of the terms) / count, out_sq = (sum of the squared terms) / count.

The reference is exact: a column of terms is summed with math.fsum (correctly rounded, S1) and once more with -S1 appended (the
residual S2; S1 + S2 is the sum to 2^-105), and the comparison |got - (S1 + S2) / count| <= bound is made in rational arithmetic.
A squared term is exact in float64 (a float32 value has 24 bits), so the second moments are sums of exact terms too.

The bound: depth * 2^-53 * (sum of |term|) / count + 2^-53 |R|.  Every addition of the two kernels is one rounded fp64 operation
(sum[kk] += x; sq[kk] = fma(x, x, sq[kk]) rounds once, on the exact product), so a term carries at most one relative error of 2^-53
per addition it passes through, and `depth` is the longest such chain.  Read off the kernels, a term passes through five
sequential sums, each starting from 0.0; a sequential sum of n items rounds n - 1 times, since 0.0 + t is exact:
  1. the lane's register sum: span_chunks * kMomQuads * rows items (rows = nrows, or nrows // step - 1 pairs)
  2. an LDS segment of moments_partials_kernel: seglen = ceil(R / G) lane sums, R = 4 * lanes / nvars, G = max(1, 256 // (2 nvars))
  3. its segments in order: ceil(R / seglen) of them hold anything; an empty one adds 0.0 exactly
  4. a segment of moments_finish_kernel: fseglen = ceil(nslot / G) partials
  5. its segments in order: ceil(nslot / fseglen) non-empty ones
  depth = sum over the five of (items - 1), and never more than terms - 1: n terms meet in n - 1 rounded additions whatever the
  order, because every other addition has an exact zero on one side.
The last term is the correctly rounded division by count.  Nothing here is measured on a GPU and no constant is fitted."""
import math
from dataclasses import dataclass
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np
import torch

import packed_ref

U64 = 2.0 ** -53            # fp64 unit roundoff
GUARD = 64                  # NaN doubles before and after every output buffer
THREADS, QUADS, SLOTS = 256, 2, 256      # kMomThreads, kMomQuads, kMomSlots
POISON = -32768             # the code between the blocks of a packed series (never produced by the encoder)
OFFSETS = [0.0, 5.0, -3.0, 100.0, 0.5, 2.0, -40.0, 7.0, 1.0, 0.0, 12.0, -1.0, 3.0, 0.0, 9.0, -6.0, 250.0, 1.0, 0.0, 4.0]  # test_standardization_stats.OFFSETS


# ---------------------------------------------------------------------------------------------------------------------------
# geometry: mom_lanes / mom_split and the segment arithmetic of the two kernels
# ---------------------------------------------------------------------------------------------------------------------------
def mom_lanes(nvars):
    return (THREADS // nvars) * nvars


def mom_geometry(nodes, nvars, lanes=None):
    """-> per_row, lanes, W, chunk, span (elements), span_chunks, nslot, G, R, seglen (partials kernel), fseglen (finish)."""
    lanes = mom_lanes(nvars) if lanes is None else lanes
    per_row = nodes * nvars
    W = 4 * lanes
    chunk = W * QUADS
    nchunks = -(-per_row // chunk)
    span_chunks = -(-nchunks // SLOTS)
    span = span_chunks * chunk
    nslot = -(-per_row // span)
    G = max(1, THREADS // (2 * nvars))
    R = W // nvars
    return NS(per_row=per_row, lanes=lanes, W=W, chunk=chunk, span=span, span_chunks=span_chunks, nslot=nslot, G=G, R=R,
              seglen=-(-R // G), fseglen=-(-nslot // G))


def depth_of(c):
    """The longest chain of rounded fp64 additions a term of the case passes through (module docstring)."""
    g = mom_geometry(c.nodes, c.nvars)
    rows = c.nrows if c.step == 0 else c.nrows // c.step - 1
    stages = (g.span_chunks * QUADS * rows, g.seglen, -(-g.R // g.seglen), g.fseglen, -(-g.nslot // g.fseglen))
    chain = sum(n - 1 for n in stages)
    return min(chain, rows * c.nodes - 1)


# ---------------------------------------------------------------------------------------------------------------------------
# cases and problems
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class MomCase:
    name: str
    nodes: int
    nvars: int
    step: int = 0              # 0: values; >= 1: standardized differences with this stride
    nrows: int = 3
    row_begin: int = 0
    layout: str = "analysis"   # analysis: is_forecast = 0, samples one time step apart | forecast: (sample, member, lead) |
    #                            shared: forecast whose members read one series (stride_member = 0)
    nbase: int = 3             # analysis: flat samples; forecast / shared: analysis times
    members: int = 1
    elem: str = "f32"          # f32 | q16
    off: int = 0               # elements between the quad boundary (16 bytes of floats, 8 bytes of codes) and the series base
    odd_step: bool = False     # stride_step odd: the rows of one sample alternate between the quad and the scalar load
    odd_member: bool = False   # stride_member odd
    data: str = "rand"         # rand | ramp (tier b: a ramp in time whose slope depends on the row's parity)

    def __str__(self):
        return self.name

    @property
    def forecast(self):
        return self.layout != "analysis"

    @property
    def nsub(self):
        return self.nrows // max(self.step, 1)

    @property
    def used(self):
        return self.nrows if self.step == 0 else self.nsub * self.step

    @property
    def count(self):
        """the divisor of an output row"""
        return (self.nrows if self.step == 0 else self.nsub - 1) * self.nodes

    def sizes(self):
        """-> n_times, steps (lead times of a forecast series), n_flat"""
        window = self.row_begin + self.nrows
        if self.forecast:
            return self.nbase, window + 1, self.nbase * self.members     # one lead time more than a sample reads
        assert self.members == 1
        return self.nbase + window - 1, 0, self.nbase

    def strides(self):
        """-> stride_sample, stride_step, stride_member, elements of the allocation.  At least one gap element behind every block;
        every stride a multiple of 4 unless asked to be odd, so that `off` alone decides which load a row takes."""
        B = self.nodes * self.nvars
        up4 = lambda n: -(-n // 4) * 4
        odd = lambda n: n if n % 2 else n + 1
        st = odd(B + 1) if self.odd_step else up4(B + 1)
        n_times, steps, _ = self.sizes()
        if not self.forecast:
            return st, st, 0, self.off + n_times * st + 4
        if self.layout == "shared":
            ss = up4(steps * st + 4)
            return ss, st, 0, self.off + self.nbase * ss + 4
        sm = up4(steps * st + 4)
        if self.odd_member:   # odd, and member 1 of an odd base back on a quad boundary
            sm += 3 if self.off % 2 else 1
        ss = up4(self.members * sm + 4)
        return ss, st, sm, self.off + self.nbase * ss + 4


def _blocks(c):
    """(address of the block's first element, index into the logical array) for every block of the series"""
    ss, st, sm, _ = c.strides()
    n_times, steps, _ = c.sizes()
    if not c.forecast:
        return [(c.off + t * st, (t,)) for t in range(n_times)]
    nm = 1 if c.layout == "shared" else c.members
    return [(c.off + s * ss + m * sm + j * st, (s, m, j)) for s in range(c.nbase) for m in range(nm) for j in range(steps)]


def _readable(c, ix):
    """Whether some sample may read the block: every time step of an analysis series, the lead times row_begin ... row_begin + used - 1
    of a forecast series."""
    return not c.forecast or c.row_begin <= ix[2] < c.row_begin + c.used


def mom_problem(c, seed, kind):
    """kind "int" (tier a): integer data in [-8, 8] (packed: integer tables), integer mean, std in {0.5, 1, 2, 4}; "rand" (tier b):
    noise around OFFSETS, or a ramp.  P.X: the decoded logical series, float32, (n_times, nodes, nvars) or (times, members,
    leads, nodes, nvars); P.flat: the allocation as the entry reads it, NaN (POISON codes) wherever no block lies, and in the
    blocks of a forecast series that no sample may read (lead times before row_begin and from row_begin + used on)."""
    rng = np.random.default_rng(seed)
    F, N = c.nvars, c.nodes
    n_times, steps, n_flat = c.sizes()
    nm = 1 if c.layout == "shared" else c.members
    shape = ((n_times,) if not c.forecast else (c.nbase, nm, steps)) + (N, F)
    P = NS(case=c, kind=kind, n_times=n_times, steps=steps, n_flat=n_flat, scale=None, offset=None, mean=None, std=None)
    offs = np.array([OFFSETS[f % len(OFFSETS)] for f in range(F)])
    if kind == "int":
        if c.elem == "q16":
            P.scale = rng.choice([1.0, 2.0], F).astype(np.float32)
            P.offset = rng.integers(-1, 3, F).astype(np.float32)
            codes = rng.integers(-3, 4, shape).astype(np.int16)
        else:
            X = rng.integers(-8, 9, shape).astype(np.float32)
        if c.step:
            P.mean = rng.integers(-2, 3, F).astype(np.float32)
            P.std = rng.choice([0.5, 1.0, 2.0, 4.0], F).astype(np.float32)
    else:
        spread = 2.0 ** rng.integers(-2, 2, F)
        X = rng.standard_normal(shape) * spread + offs
        if c.data == "ramp":   # rows of even and odd time index on lines of different slope: a pair across sub-offsets stands out
            t = np.arange(shape[-3]).reshape((-1, 1, 1))
            X = 0.01 * rng.standard_normal(shape) * spread + offs + np.where(t % 2 == 0, 0.5 * t, -0.25 * t) * spread
        X = X.astype(np.float32)
        if c.elem == "q16":
            P.scale, P.offset = packed_ref.default_tables(X)
            codes = packed_ref.encode(X, P.scale, P.offset)
        if c.step:
            P.mean = (offs + 0.3 * spread * rng.standard_normal(F)).astype(np.float32)
            P.std = (spread * rng.uniform(0.7, 1.4, F)).astype(np.float32)
    if c.elem == "q16":
        X = packed_ref.decode(codes, P.scale, P.offset)
        assert kind != "int" or float(np.abs(X).max()) <= 8
    P.X = X
    ss, st, sm, total = c.strides()
    P.stride_sample, P.stride_step, P.stride_member = ss, st, sm
    src = codes if c.elem == "q16" else X
    P.flat = np.full(total, POISON, np.int16) if c.elem == "q16" else np.full(total, np.nan, np.float32)
    for addr, ix in _blocks(c):
        assert addr + N * F < total
        if _readable(c, ix):
            P.flat[addr: addr + N * F] = src[ix].reshape(-1)
    return P


def decoded_float_problem(P):
    """The fp32 problem that holds the decoded values of a packed one at the same addresses (NaN where POISON stands)."""
    c = P.case
    assert c.elem == "q16"
    Q = NS(**P.__dict__)
    n = c.nodes * c.nvars
    Q.flat = np.full(P.flat.size, np.nan, np.float32)
    for addr, ix in _blocks(c):
        if _readable(c, ix):
            Q.flat[addr: addr + n] = P.X[ix].reshape(-1)
    assert np.array_equal(np.isnan(Q.flat), P.flat == POISON)
    Q.scale = Q.offset = None
    return Q


def sample_rows(c, X, idx):
    """(nrows, nodes, nvars) of flat sample idx"""
    s, m = divmod(idx, c.members)
    if not c.forecast:
        return X[s + c.row_begin: s + c.row_begin + c.nrows]
    return X[s, 0 if c.layout == "shared" else m, c.row_begin: c.row_begin + c.nrows]


def row_terms(c, rows, k, mean, std):
    """The terms of output row (sample, k) as float64, (terms per feature, nvars)."""
    if c.step == 0:
        return rows.astype(np.float64).reshape(-1, c.nvars)
    sub = rows[k: c.used: c.step]
    z = (sub - mean) / std
    d = z[1:] - z[:-1]
    assert z.dtype == np.float32 and d.dtype == np.float32 and len(d) == c.nsub - 1
    return d.astype(np.float64).reshape(-1, c.nvars)


def _dd_sum(T):
    """Column sums of T as (S1, S2), S1 correctly rounded and S1 + S2 exact to 2^-105."""
    hi, lo = np.empty(T.shape[1]), np.empty(T.shape[1])
    for f in range(T.shape[1]):
        col = T[:, f].tolist()
        hi[f] = math.fsum(col)
        col.append(-hi[f])
        lo[f] = math.fsum(col)
    return hi, lo


def moments_math(P, first=0, count=None):
    """-> ref: name ("mean", "sq") -> NS(R: the float64 quotient S1 / count, hi, lo: the exact sum, bound), arrays of
    (count * max(step, 1), nvars)."""
    c = P.case
    count = P.n_flat - first if count is None else count
    S = max(c.step, 1)
    depth = depth_of(c)
    out = {n: NS(hi=[], lo=[], mag=[]) for n in ("mean", "sq")}
    for i in range(count):
        rows = sample_rows(c, P.X, first + i)
        for k in range(S):
            T = row_terms(c, rows, k, P.mean, P.std)
            assert T.shape[0] == c.count
            for n, V in (("mean", T), ("sq", T * T)):
                hi, lo = _dd_sum(V)
                out[n].hi.append(hi), out[n].lo.append(lo), out[n].mag.append(np.abs(V).sum(0))
    cnt = np.float64(c.count)
    for r in out.values():
        r.hi, r.lo, mag = np.array(r.hi), np.array(r.lo), np.array(r.mag)
        r.R = r.hi / cnt
        r.bound = depth * U64 * mag / cnt + U64 * np.abs(r.R)
        r.count = c.count
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def compare_exact(got, ref, names=("mean", "sq")):
    """Tier (a): the sums are exact, so an output is the correctly rounded quotient; -> names of the outputs that are not its bits."""
    bad = []
    for n in names:
        r = ref[n]
        assert not r.lo.any(), "tier (a): the float64 sum itself must be exact"
        if got[n].shape != r.R.shape or not np.array_equal(_bits(got[n]), _bits(r.R)):
            bad.append(n)
    return bad


def compare_bounded(got, ref, names=("mean", "sq"), note=None):
    """Tier (b): |got - (S1 + S2) / count| <= bound element by element, in rational arithmetic; a non-finite output fails.
    note(name, ratio): the largest |got - R| / bound."""
    bad = []
    for n in names:
        r = ref[n]
        g = np.asarray(got[n], dtype=np.float64)
        if g.shape != r.R.shape or not np.isfinite(g).all():
            bad.append(n)
            if note is not None:
                note(n, float("inf"))
            continue
        worst = Fraction(0)
        for gv, hi, lo, b in zip(g.ravel().tolist(), r.hi.ravel().tolist(), r.lo.ravel().tolist(), r.bound.ravel().tolist()):
            err = abs(Fraction(gv) - (Fraction(hi) + Fraction(lo)) / r.count)
            worst = max(worst, err / Fraction(b) if b > 0 else (Fraction(0) if err == 0 else Fraction(10 ** 9)))
        if worst > 1:
            bad.append(n)
        if note is not None:
            note(n, float(worst))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# the stand-in: the two kernels in numpy, on the allocation and its strides, fp64 sums in the kernels' order
# ---------------------------------------------------------------------------------------------------------------------------
MOM_DEFECTS = ("last_partial_quad_dropped", "last_span_skipped", "span_end_not_clamped", "features_of_256_lanes",
               "zp_carried_over_sub_offsets", "first_row_difference_counted", "count_without_minus_one", "finish_one_partial_short",
               "decode_fused")


def _decode(P, raw, feat, fused):
    if P.case.elem != "q16":
        return raw
    sc, of = P.scale[feat], P.offset[feat]
    if fused:   # one fma: the exact product (16 + 24 bits) and the sum rounded once
        return (raw.astype(np.float64) * sc.astype(np.float64) + of.astype(np.float64)).astype(np.float32)
    return packed_ref.decode(raw, sc, of)


def _ordered(items, G, seglen):
    """items (n, C): G segments of seglen items each, summed item by item, then the segments in order (an empty one adds 0.0)."""
    n, C = items.shape
    pad = np.zeros((G * seglen, C))
    pad[: min(n, G * seglen)] = items[: G * seglen]
    pad = pad.reshape(G, seglen, C)
    seg = np.zeros((G, C))
    for r in range(seglen):
        seg = seg + pad[:, r]
    v = np.zeros(C)
    for g in range(G):
        v = v + seg[g]
    return v


def standin(P, first=0, count=None, defect=None):
    """-> {"mean", "sq"}: what the kernel pair computes, or what it would with `defect`."""
    c = P.case
    assert defect is None or defect in MOM_DEFECTS
    F, S = c.nvars, max(c.step, 1)
    count = P.n_flat - first if count is None else count
    g = mom_geometry(c.nodes, F, lanes=THREADS if defect == "features_of_256_lanes" else None)
    flat, last = P.flat, P.flat.size - 1
    tid, kk = np.arange(g.lanes)[:, None], np.arange(4)[None, :]
    feat = (4 * tid + kk) % F
    n_out = count * S
    ws = np.zeros((n_out, g.nslot, 2 * F))
    with np.errstate(all="ignore"):
        for o in range(n_out):
            i, k = divmod(o, S)
            s, m = divmod(first + i, c.members)
            base = c.off + s * P.stride_sample + m * P.stride_member
            if c.step == 0:
                rows, first_counted = [c.row_begin + r for r in range(c.nrows)], 0
            else:
                rows, first_counted = [c.row_begin + k + r * S for r in range(c.nsub)], 1
                if defect == "first_row_difference_counted":
                    first_counted = 0
                if defect == "zp_carried_over_sub_offsets" and k > 0:   # the last row of sub-offset k - 1 is still in zp
                    rows, first_counted = [c.row_begin + k - 1 + (c.nsub - 1) * S] + rows, 1
            for slot in range(g.nslot):
                if defect == "last_span_skipped" and slot == g.nslot - 1:
                    continue
                e0 = slot * g.span
                e1 = e0 + g.span if defect == "span_end_not_clamped" else min(g.per_row, e0 + g.span)
                acc, acc2 = np.zeros((g.lanes, 4)), np.zeros((g.lanes, 4))
                for cc in range(e0, e1, g.W * QUADS):
                    zp = np.zeros((QUADS, g.lanes, 4), np.float32)
                    for ri, j in enumerate(rows):
                        for q in range(QUADS):
                            e = cc + q * g.W + 4 * tid + kk
                            valid = e < e1
                            if defect == "last_partial_quad_dropped":
                                valid = valid & (e[:, :1] + 3 < e1)
                            x = _decode(P, flat[np.minimum(base + j * P.stride_step + e, last)], feat, defect == "decode_fused")
                            x = np.where(e < e1, x, np.float32(0))
                            if c.step:
                                z = (x - P.mean[feat]) / P.std[feat]
                                x, zp[q] = z - zp[q], z
                                assert x.dtype == np.float32
                                if ri < first_counted:
                                    continue
                            x = np.where(valid, x.astype(np.float64), 0.0)
                            acc = acc + x
                            acc2 = acc2 + x * x
                red = np.stack([acc.reshape(-1), acc2.reshape(-1)])[:, : g.R * F].reshape(2, g.R, F)
                items = np.concatenate([red[0], red[1]], axis=1)      # (R, 2 F): column j = q * F + f
                ws[o, slot] = _ordered(items, g.G, g.seglen)
    nsl = g.nslot - 1 if defect == "finish_one_partial_short" else g.nslot
    div = np.float64(c.count if defect != "count_without_minus_one" or c.step == 0 else c.nsub * c.nodes)
    with np.errstate(all="ignore"):
        res = np.array([_ordered(ws[o, :nsl], g.G, -(-g.nslot // g.G)) / div for o in range(n_out)])
    return {"mean": res[:, :F], "sq": res[:, F:]}


def standin_check(c, kind, defect=None, seed=5):
    """The stand-in compared like a kernel -> names of the failing outputs."""
    P = mom_problem(c, seed, kind)
    ref = moments_math(P)
    got = standin(P, defect=defect)
    return compare_exact(got, ref) if kind == "int" else compare_bounded(got, ref)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU side: the series at a chosen alignment, NaN-filled float64 outputs between NaN guards
# ---------------------------------------------------------------------------------------------------------------------------
def put(a, dev="cuda"):
    """a numpy array on the device, on a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    assert t.data_ptr() % 16 == 0
    return t


class Out:
    """A float64 output buffer filled with NaN, GUARD NaN doubles before and after it."""

    def __init__(self, n, dev="cuda"):
        self.n = int(n)
        self.buf = torch.full((2 * GUARD + self.n,), float("nan"), device=dev, dtype=torch.float64)

    def ptr(self):
        return self.buf.data_ptr() + 8 * GUARD

    def read(self):
        full = self.buf.cpu().numpy()
        assert np.isnan(full[:GUARD]).all() and np.isnan(full[GUARD + self.n:]).all(), "a guard was written"
        return full[GUARD: GUARD + self.n].copy()
