"""Kernel-level checks of the weight-gradient C-ABI (nlam_wgrad, nlam_wgrad_group) and of the deterministic reductions behind it
(nlam_reduce_jobs, nlam_reduce_partials), against float64 math.

Every case names the plan code (nlam_wgrad_plan) it is meant to exercise and asserts it before launching, so a case cannot
quietly test another kernel.  Each case is checked in two tiers:
  (a) exact arithmetic: small-integer operands are exact in bf16, and their products and sums are exact in fp32, so every path
      must reproduce float64(A^T S) bit for bit -- a dropped or duplicated row, stage, column, window, gather or slice shows;
  (b) precision: random operands with a different scale per column, elementwise |dW - R| <= tau * (|A|^T |S|) with tau derived
      from the accumulation length (fp32 unit roundoff times the rows one slice sums, plus the slice count, plus a few units for
      the three-term split), R computed in float64 from the operands as the kernel sees them.
The reductions are emulated in numpy float32 in the kernels' documented summation order and compared with torch.equal."""
import ctypes as C
import json
import os
from dataclasses import dataclass, replace

import numpy as np
import pytest
import torch

from neural_lam_amd import _lib as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # fp32 unit roundoff
RED_PARTIALS_WAVES = 4   # waves of reduce_partials_kernel (a literal of the kernel; reduce_jobs' count comes from the library)
TUNE_DEFAULTS = {L.TUNE_WGRAD_LDMA: 3, L.TUNE_WGRAD_LDMA_VAR: 0, L.TUNE_WGRAD_BIG_MIN_ROWS: 0}
MM1, MM3 = 1 << 8, 3 << 8

_RATIOS = {}   # plan code -> (largest |dW - R| / (|A|^T|S|), tau of that case) over the tier-(b) runs


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib = L.load()
    yield lib
    path = os.environ.get("NLAM_WGRAD_REPORT")
    if path and _RATIOS:
        with open(path, "w") as f:
            json.dump({str(k): v for k, v in sorted(_RATIOS.items())}, f, indent=1)


class tuning:
    """Process-wide tuning for one block; the defaults come back in any case."""

    def __init__(self, lib, settings):
        self.lib, self.settings = lib, dict(settings)

    def __enter__(self):
        for k, v in self.settings.items():
            assert self.lib.nlam_set_tuning(k, v) == 0
        return self

    def __exit__(self, *exc):
        for k, v in TUNE_DEFAULTS.items():
            self.lib.nlam_set_tuning(k, v)
        return False


@dataclass(frozen=True)
class Case:
    name: str
    plan: int
    m: int
    widths: tuple
    rows: int
    batch: int = 1
    broadcast: tuple = ()     # sources with bstride = 0 (shared by the batch)
    gather: tuple = ()        # sources read through an index (unsorted, repeated rows)
    mm: int = 0               # NLAM_F_MM_* bits
    silu: bool = False
    solo: bool = False
    abf: bool = False         # A stored as bf16
    sbf: bool = False         # src[0] stored as bf16
    a_off: int = 0            # bytes the A pointer is moved off its allocation's (512-byte aligned) start
    s_off: int = 0            # ... the same for src[0]
    pad_bstride: int = 0      # elements added to src[0]'s batch stride
    tune: tuple = ()          # ((key, value), ..)

    def __str__(self):
        return self.name


def C_(name, plan, m, widths, rows, **kw):
    if kw.get("abf"):
        kw.setdefault("mm", MM1)   # bf16 operands belong to the one-term matrix mode
    return Case(name, plan, m, tuple(widths), rows, **kw)


LDMA, VAR, BIGROWS = L.TUNE_WGRAD_LDMA, L.TUNE_WGRAD_LDMA_VAR, L.TUNE_WGRAD_BIG_MIN_ROWS
CASES = [
    # wgrad_smalln_kernel: one source of <= 8 columns
    C_("smalln_r1", L.WGP_SMALLN, 64, [3], 1),
    C_("smalln_b3_bcast", L.WGP_SMALLN, 132, [8], 33, batch=3, broadcast=(0,)),
    C_("smalln_gather_silu", L.WGP_SMALLN, 20, [5], 3001, gather=(0,), silu=True),
    # wgrad_dma_kernel: m and every width <= 64, % 4
    C_("dma_r15", L.WGP_DMA, 32, [32], 15),
    C_("dma_60_60_12", L.WGP_DMA, 64, [60, 60, 12], 17, batch=3, broadcast=(1,), gather=(0, 2)),
    C_("dma_3src_silu", L.WGP_DMA, 64, [64, 64, 64], 3001, silu=True),
    # wgrad_kernel: m or a width not % 4, and the LDS-DMA shapes whose pointers are not 16-byte aligned
    C_("narrow_256_17", L.WGP_NARROW, 17, [256, 17], 31, batch=3, gather=(1,)),
    C_("narrow_silu", L.WGP_NARROW, 60, [30], 33, silu=True),
    C_("narrow_misaligned_A", L.WGP_NARROW, 64, [64], 100, a_off=4),
    C_("narrow_odd_bstride", L.WGP_NARROW, 32, [32], 40, batch=3, pad_bstride=1),
    # wgrad_wide_kernel: fp32 MFMA
    C_("wide_132", L.WGP_WIDE, 132, [60, 60, 12], 33, batch=3, gather=(2,), broadcast=(1,)),
    C_("wide_384_silu", L.WGP_WIDE, 384, [256], 15, silu=True),
    C_("wide_solo", L.WGP_WIDE, 128, [128], 1000, solo=True),
    # wgrad_wbf_kernel, fp32 operands, 128 x 128 windows
    C_("wbf3_3src", L.WGP_WBF, 128, [128, 128, 128], 1000, mm=MM3, gather=(1,)),
    C_("wbf1_60_60_12", L.WGP_WBF, 96, [60, 60, 12], 17, batch=3, broadcast=(0,), mm=MM1),
    C_("wbf3_256_20_silu", L.WGP_WBF, 68, [256, 20], 3001, mm=MM3, silu=True),
    C_("wbf3_bigminrows", L.WGP_WBF, 260, [256], 200, mm=MM3, tune=((BIGROWS, 1 << 20),)),
    # wgrad_wbf_kernel, fp32 operands, 256 x 256 windows
    C_("wbf3_big_260", L.WGP_WBF_BIG, 260, [256], 1000, mm=MM3),
    C_("wbf3_big_384_silu", L.WGP_WBF_BIG, 384, [132], 31, batch=3, broadcast=(0,), gather=(0,), mm=MM3, silu=True),
    C_("wbf1_big_misaligned_A", L.WGP_WBF_BIG, 256, [256], 500, mm=MM1, a_off=8),
    C_("wbf1_big_ldma_off", L.WGP_WBF_BIG, 256, [256], 500, mm=MM1, silu=True, tune=((LDMA, 1),)),
    C_("wbf1_big_solo", L.WGP_WBF_BIG, 256, [256], 500, mm=MM1, solo=True, tune=((LDMA, 0),)),
    # wgrad_wbf_kernel, bf16 operands
    C_("wbfB_A", L.WGP_WBF_B, 128, [128], 1000, abf=True),
    C_("wbfB_AS_silu", L.WGP_WBF_B, 128, [128], 33, batch=3, abf=True, sbf=True, silu=True),
    C_("wbfB_big_m132", L.WGP_WBF_B_BIG, 132, [256], 1000, abf=True),
    C_("wbfB_big_A_off8", L.WGP_WBF_B_BIG, 256, [256], 500, abf=True, a_off=8),
    C_("wbfB_big_S_w132", L.WGP_WBF_B_BIG, 256, [132], 500, abf=True, sbf=True, silu=True),
    C_("wbfB_big_bit0_off", L.WGP_WBF_B_BIG, 256, [256], 500, abf=True, tune=((LDMA, 2),)),
    C_("wbfB_big_bit0_off_AS", L.WGP_WBF_B_BIG, 384, [256], 500, abf=True, sbf=True, silu=True, tune=((LDMA, 2),)),
    # wgrad_ldma_kernel, bf16 operands, variants 0-3
    *[C_(f"ldmaB_A_v{v}", L.WGP_LDMA_B, 256, [256], 3001, abf=True, tune=((VAR, v),)) for v in range(4)],
    *[C_(f"ldmaB_AS_silu_v{v}", L.WGP_LDMA_B, 384, [256], 1000, abf=True, sbf=True, silu=True, tune=((VAR, v),)) for v in range(4)],
    C_("ldmaB_A_gather", L.WGP_LDMA_B, 264, [128, 64], 17, batch=3, broadcast=(1,), gather=(0, 1), abf=True),
    # wgrad_ldma_kernel, fp32 operands, one term, variants 0-2
    *[C_(f"ldma1_v{v}", L.WGP_LDMA_1, 256, [256], 3001, mm=MM1, tune=((VAR, v),)) for v in range(3)],
    *[C_(f"ldma1_silu_v{v}", L.WGP_LDMA_1, 260, [256, 12], 1000, mm=MM1, silu=True, tune=((VAR, v),)) for v in range(2)],
    C_("ldma1_gather_b3", L.WGP_LDMA_1, 384, [60, 60, 12], 33, batch=3, broadcast=(0,), gather=(1, 2), mm=MM1),
    # wgrad_ldma_kernel, three terms (NLAM_TUNE_WGRAD_LDMA bit 2)
    C_("ldma3", L.WGP_LDMA_3, 256, [256], 1000, mm=MM3, tune=((LDMA, 7),)),
    C_("ldma3_silu_b3", L.WGP_LDMA_3, 260, [132], 31, batch=3, gather=(0,), mm=MM3, silu=True, tune=((LDMA, 7),)),
]


# ---------------------------------------------------------------------------------------------------------------------------
# operands and launch
# ---------------------------------------------------------------------------------------------------------------------------
def _src_rows(case, s):
    return case.rows // 2 + 3 if s in case.gather else case.rows


def _alloc(shape_numel, dtype, off_bytes, dev):
    """A flat buffer with the tensor `off_bytes` past its start (a view: the pointer the kernel gets is moved by that much)."""
    esz = torch.empty((), dtype=dtype).element_size()
    assert off_bytes % esz == 0
    buf = torch.empty(shape_numel + off_bytes // esz + 8, dtype=dtype, device=dev)
    return buf[off_bytes // esz: off_bytes // esz + shape_numel]


def make_operands(case, gen, integer):
    """Host (float64) operands as the kernel reads them, plus their device copies."""
    dev = torch.device("cuda")

    def values(shape, col_axis_len):
        if integer:
            return torch.randint(-8, 9, shape, generator=gen).double()
        scale = 2.0 ** torch.randint(-3, 4, (col_axis_len,), generator=gen).double()   # a different scale per column
        return torch.randn(shape, generator=gen, dtype=torch.float64) * scale

    R = case.batch * case.rows
    A = values((R, case.m), case.m)
    adt = torch.bfloat16 if case.abf else torch.float32
    A = A.to(adt).double()   # what is stored
    Ad = _alloc(A.numel(), adt, case.a_off, dev)
    Ad.copy_(A.reshape(-1).to(adt))
    srcs = []
    for s, w in enumerate(case.widths):
        sdt = torch.bfloat16 if (s == 0 and case.sbf) else torch.float32
        nr = _src_rows(case, s)
        nb = 1 if s in case.broadcast else case.batch
        bstride = 0 if s in case.broadcast else nr * w + (case.pad_bstride if s == 0 else 0)
        S = values((nb, nr, w), w).to(sdt).double()
        numel = max(nb - 1, 0) * bstride + nr * w
        Sd = _alloc(numel, sdt, case.s_off if s == 0 else 0, dev)
        flat = torch.zeros(numel, dtype=torch.float64)
        for b in range(nb):
            flat[b * bstride: b * bstride + nr * w] = S[b].reshape(-1)
        Sd.copy_(flat.to(sdt))
        idx = None
        if s in case.gather:
            idx = torch.randint(0, nr, (case.rows,), generator=gen, dtype=torch.int32)   # unsorted, with repeated rows
            idx[: min(4, case.rows)] = nr - 1
        srcs.append(dict(S=S, Sd=Sd, bstride=bstride, idx=idx, idxd=None if idx is None else idx.to(dev), width=w))
    return A, Ad, srcs


def describe(lib, case, Ad, srcs):
    """The call's nlam_wgrad_t with nparts = nlam_wgrad_nparts and a placeholder partials pointer."""
    q = L.Wgrad()
    q.A, q.m, q.batch, q.rows, q.nsrc = Ad.data_ptr(), case.m, case.batch, case.rows, len(case.widths)
    q.flags = case.mm | (L.F_SILU_B if case.silu else 0) | (L.F_WGRAD_SOLO if case.solo else 0)
    q.flags |= (L.F_A_BF16 if case.abf else 0) | (L.F_S_BF16 if case.sbf else 0)
    q.n = sum(case.widths)
    for k, s in enumerate(srcs):
        q.src[k].ptr = s["Sd"].data_ptr()
        q.src[k].idx = None if s["idxd"] is None else s["idxd"].data_ptr()
        q.src[k].bstride, q.src[k].width = s["bstride"], s["width"]
    q.partials, q.nparts = Ad.data_ptr(), 1
    q.nparts = lib.nlam_wgrad_nparts(C.byref(q))
    return q


def reduce_sum(lib, partials, nparts, m, n):
    """dW from the partials with one nlam_reduce_jobs launch (itself checked by the reduction tests below)."""
    out = torch.empty((m, n), device="cuda", dtype=torch.float32)
    jobs = L.ReduceJobs()
    jobs.njobs = 1
    j = jobs.job[0]
    j.partials, j.out, j.stride, j.nparts, j.n = partials.data_ptr(), out.data_ptr(), m * n, nparts, m * n
    j.accumulate, j.ncols, j.ld = 0, 0, 0
    assert lib.nlam_reduce_jobs(C.byref(jobs), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    return out


def launch(lib, case, Ad, srcs, nparts=None):
    q = describe(lib, case, Ad, srcs)
    assert lib.nlam_wgrad_plan(C.byref(q)) == case.plan, (case.name, lib.nlam_wgrad_plan(C.byref(q)))
    np_ = q.nparts if nparts is None else nparts
    partials = torch.empty((np_, case.m, q.n), device="cuda", dtype=torch.float32)
    q.partials, q.nparts = partials.data_ptr(), np_
    assert lib.nlam_wgrad_plan(C.byref(q)) == case.plan
    assert lib.nlam_wgrad(C.byref(q), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    out = reduce_sum(lib, partials, np_, case.m, q.n)
    torch.cuda.synchronize()
    return partials, out, np_


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    return x.to(torch.float32).to(torch.bfloat16).double()


def near_bf16_tie(x, ulps=256):
    """Elements whose fp32 value lies within `ulps` fp32 units of a bf16 rounding midpoint: there an fp32 SiLU that differs
    from the float64 one by a few units may round to the other bf16 neighbour."""
    b = x.to(torch.float32).view(torch.int32) & 0xFFFF
    return (b - 0x8000).abs() <= ulps


def reference(case, A, srcs):
    """R = sum_b A_b^T B_b in float64, B = [f(S_0[idx_0]), ..], from the operands as the kernel sees them, the elementwise
    scale |A|^T |B|, and the extra bound where the kernel's fp32 SiLU may round to the other bf16 neighbour."""
    one_term = case.mm == MM1 or case.abf
    Ab = bf16_rne(A) if one_term else A
    Bs, Bs_tie = [], []
    for s, src in enumerate(srcs):
        parts, ties = [], []
        for b in range(case.batch):
            S = src["S"][0 if s in case.broadcast else b]
            S = S[src["idx"].long()] if src["idx"] is not None else S
            tie = torch.zeros_like(S)
            if case.silu:
                S = S * torch.sigmoid(S)
                if one_term:
                    tie = near_bf16_tie(S).double() * S.abs()
            if one_term:
                S = bf16_rne(S)
            parts.append(S)
            ties.append(tie)
        Bs.append(torch.stack(parts))
        Bs_tie.append(torch.stack(ties))
    B = torch.cat(Bs, dim=-1)              # (batch, rows, n)
    Bt = torch.cat(Bs_tie, dim=-1)
    A3 = Ab.reshape(case.batch, case.rows, case.m)
    R = torch.einsum("brm,brn->mn", A3, B)
    scale = torch.einsum("brm,brn->mn", A3.abs(), B.abs())
    tie = torch.einsum("brm,brn->mn", A3.abs(), Bt)
    return R, scale, tie


def rows_per_slice(case, nparts):
    """Most rows one workgroup accumulates: its share of the 16- or 32-row stages (rows of a batch item never share a stage)."""
    most = -(-case.batch * case.rows // nparts)
    for st in (16, 32):
        stages = case.batch * -(-case.rows // st)
        most = max(most, -(-stages // nparts) * st)
    return most


def tau(case, nparts):
    t = U * (rows_per_slice(case, nparts) + nparts + 16)
    if case.silu and not (case.mm == MM1 or case.abf):
        t += 2.0 ** -19   # the kernels' fp32 SiLU (v_exp_f32, v_rcp_f32) against the float64 one
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases
# ---------------------------------------------------------------------------------------------------------------------------
def _run(lib, case, integer, seed, nparts=None):
    gen = torch.Generator().manual_seed(seed)
    A, Ad, srcs = make_operands(case, gen, integer)
    with tuning(lib, case.tune):
        p1, o1, np_ = launch(lib, case, Ad, srcs, nparts)
        p2, o2, _ = launch(lib, case, Ad, srcs, nparts)
    assert torch.equal(p1, p2) and torch.equal(o1, o2), f"{case}: two launches differ"
    return A, srcs, p1, o1, np_


@pytest.mark.parametrize("case", [c for c in CASES if not c.silu], ids=str)
def test_wgrad_exact_on_integers(lib, case):
    """Tier (a): integer operands, every path reproduces float64(A^T S) exactly -- the partial slices too."""
    A, srcs, partials, out, np_ = _run(lib, case, True, 1)
    R, _, _ = reference(case, A, srcs)
    assert torch.isfinite(partials).all(), f"{case}: unwritten partials"
    assert torch.equal(partials.double().sum(0).cpu(), R), f"{case}: partials do not sum to the exact product"
    assert torch.equal(out.double().cpu(), R), f"{case}: reduced dW is not the exact product"


@pytest.mark.parametrize("case", CASES, ids=str)
def test_wgrad_elementwise_error_bound(lib, case):
    """Tier (b): |dW - R| <= tau * (|A|^T |S|) element by element (+ one bf16 unit of the SiLU where it may round the
    other way), columns of different scales."""
    A, srcs, partials, out, np_ = _run(lib, case, False, 2)
    R, scale, tie = reference(case, A, srcs)
    t = tau(case, np_)
    err = (out.double().cpu() - R).abs()
    bound = t * scale + 2.0 ** -7 * tie
    bad = err > bound
    ratio = float((err / scale.clamp_min(1e-300)).max())
    prev = _RATIOS.get(case.plan, (0.0, t))
    _RATIOS[case.plan] = (max(prev[0], ratio), max(prev[1], t))
    assert not bad.any(), f"{case}: {int(bad.sum())} elements over the bound; worst err/scale {ratio:.3e}, tau {t:.3e}"


# Every wgrad_ldma_kernel instantiation (NLAM_TUNE_WGRAD_LDMA_VAR 0-3 of each operand form, with and without SiLU) and each
# wgrad_wbf_kernel form at nparts = 2, with enough rows that every workgroup runs its stage ring round at least twice: the
# steady state of the pipeline (ring wrap, requests NBUF - 1 stages ahead, the in-place SiLU of the next stage) is what runs.
RING_MAX = 8         # deepest ring of the wgrad_ldma_kernel instantiations (bf16 A + S, variant 3)
DEEP_NPARTS = 2
DEEP_CASES = [
    *[C_(f"deep_ldmaB_A_v{v}", L.WGP_LDMA_B, 256, [256], 1100, abf=True, tune=((VAR, v),)) for v in range(4)],
    *[C_(f"deep_ldmaB_AS_silu_v{v}", L.WGP_LDMA_B, 256, [256], 380, batch=3, abf=True, sbf=True, silu=True, tune=((VAR, v),))
      for v in range(4)],
    *[C_(f"deep_ldma1_v{v}", L.WGP_LDMA_1, 256, [256], 1100, mm=MM1, gather=(0,), tune=((VAR, v),)) for v in range(3)],
    *[C_(f"deep_ldma1_silu_v{v}", L.WGP_LDMA_1, 256, [256], 380, batch=3, mm=MM1, silu=True, tune=((VAR, v),)) for v in range(2)],
    C_("deep_ldma3", L.WGP_LDMA_3, 256, [256], 1100, mm=MM3, tune=((LDMA, 7),)),
    C_("deep_ldma3_silu", L.WGP_LDMA_3, 256, [256], 380, batch=3, gather=(0,), mm=MM3, silu=True, tune=((LDMA, 7),)),
    C_("deep_wbf3", L.WGP_WBF, 128, [128], 1100, mm=MM3, silu=True),
    C_("deep_wbf3_big", L.WGP_WBF_BIG, 256, [256], 1100, mm=MM3),
    C_("deep_wbfB", L.WGP_WBF_B, 128, [128], 380, batch=3, abf=True, sbf=True, silu=True),
    C_("deep_wbfB_big", L.WGP_WBF_B_BIG, 256, [256], 1100, abf=True, tune=((LDMA, 2),)),
]


@pytest.mark.parametrize("case", DEEP_CASES, ids=str)
def test_wgrad_deep_pipeline(lib, case):
    """Tiers (a) (without SiLU) and (b) where each workgroup takes at least 2 x RING_MAX stages of the taller (32-row) kind."""
    least = case.batch * -(-case.rows // 32) // DEEP_NPARTS
    assert least >= 2 * RING_MAX, f"{case}: only {least} stages per workgroup"
    if not case.silu:
        A, srcs, partials, out, _ = _run(lib, case, True, 5, DEEP_NPARTS)
        R, _, _ = reference(case, A, srcs)
        assert torch.equal(partials.double().sum(0).cpu(), R) and torch.equal(out.double().cpu(), R), f"{case}: tier (a)"
    A, srcs, partials, out, np_ = _run(lib, case, False, 6, DEEP_NPARTS)
    R, scale, tie = reference(case, A, srcs)
    t = tau(case, np_)
    err = (out.double().cpu() - R).abs()
    ratio = float((err / scale.clamp_min(1e-300)).max())
    assert not (err > t * scale + 2.0 ** -7 * tie).any(), f"{case}: tier (b), worst err/scale {ratio:.3e}, tau {t:.3e}"


NPARTS_CASES = [c for c in CASES if c.name in ("smalln_b3_bcast", "dma_60_60_12", "narrow_256_17", "wide_132", "wbf1_60_60_12",
                                                 "wbf3_big_384_silu", "wbfB_AS_silu", "wbfB_big_m132", "ldmaB_A_gather",
                                                 "ldma1_gather_b3", "ldma3_silu_b3")]


@pytest.mark.parametrize("case", NPARTS_CASES, ids=str)
def test_wgrad_any_slice_count(lib, case):
    """Any nparts >= 1 is served: one slice, and more slices than the problem has row stages (the empty ones write zeros)."""
    case = replace(case, silu=case.silu and case.sbf)
    stages = case.batch * -(-case.rows // 16)
    # slices from `empty` on get no rows: a stage apiece for the stage kernels, a row apiece for the streaming one
    empty = case.batch * case.rows if case.plan == L.WGP_SMALLN else stages
    for nparts in (1, case.batch * case.rows + 5):
        A, srcs, partials, out, np_ = _run(lib, case, True, 3, nparts)
        R, scale, tie = reference(case, A, srcs)
        assert np_ == nparts and torch.isfinite(partials).all()
        if not case.silu:
            assert torch.equal(out.double().cpu(), R), f"{case}, nparts {nparts}"
        else:   # bf16 S needs the SiLU: the tier-(b) bound
            err = (out.double().cpu() - R).abs()
            assert not (err > tau(case, nparts) * scale + 2.0 ** -7 * tie).any(), f"{case}, nparts {nparts}"
        if nparts > 1:
            assert torch.count_nonzero(partials[empty:]) == 0, f"{case}: slices without rows must write zeros"


def test_three_term_ldma_matches_wbf(lib):
    """The three-term LDS-DMA kernel keeps wgrad_wbf_kernel's K steps, slices and term order: bit-identical partials without
    SiLU.  With SiLU the two have been observed to differ in the last bits (cause not established); then each must meet the
    tier-(b) bound and the two must agree within it."""
    for silu in (False, True):
        base = C_("ldma3_vs_wbf", L.WGP_LDMA_3, 256, [256], 1000, mm=MM3, silu=silu, tune=((LDMA, 7),))
        gen = torch.Generator().manual_seed(4)
        A, Ad, srcs = make_operands(base, gen, False)
        with tuning(lib, base.tune):
            p_ldma, o_ldma, np_ = launch(lib, base, Ad, srcs)
        p_wbf, o_wbf, _ = launch(lib, replace(base, plan=L.WGP_WBF_BIG, tune=()), Ad, srcs)
        if not silu:
            assert torch.equal(p_ldma, p_wbf) and torch.equal(o_ldma, o_wbf), "three terms without SiLU"
            continue
        R, scale, _ = reference(base, A, srcs)
        t = tau(base, np_)
        for name, o in (("ldma", o_ldma), ("wbf", o_wbf)):
            assert not ((o.double().cpu() - R).abs() > t * scale).any(), f"{name} with SiLU over the tier-(b) bound"
        assert not ((o_ldma.double() - o_wbf.double()).abs().cpu() > 2 * t * scale).any(), "the two kernels disagree with SiLU"


def test_group_members_are_bit_identical_to_solo_launches(lib):
    """nlam_wgrad_group runs wgrad_wbf_kernel's body per member: each member's partials equal its own nlam_wgrad launch."""
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    shapes = [  # (m, widths, mm, silu, rows of each member)
        (128, (128, 60), MM3, True, (33, 1000, 1)),
        (256, (256,), MM1, False, (500, 17)),
    ]
    with tuning(lib, {LDMA: 0}):   # the solo launches on wgrad_wbf_kernel (the LDS-DMA kernel is not part of the group path)
        for m, widths, mm, silu, rows_list in shapes:
            members, qs, solo = [], [], []
            for k, rows in enumerate(rows_list):
                case = C_(f"g{k}", None, m, widths, rows, mm=mm, silu=silu, gather=(0,))
                A, Ad, srcs = make_operands(case, torch.Generator().manual_seed(10 + k), False)
                q = describe(lib, case, Ad, srcs)
                plan = lib.nlam_wgrad_plan(C.byref(q))
                assert plan in (L.WGP_WBF, L.WGP_WBF_BIG)
                solo.append(launch(lib, replace(case, plan=plan), Ad, srcs)[0])
                partials = torch.empty((q.nparts, m, q.n), device="cuda", dtype=torch.float32)
                q.partials = partials.data_ptr()
                members.append((partials, Ad, srcs))
                qs.append(q)
            assert len({lib.nlam_wgrad_plan(C.byref(q)) for q in qs}) == 1, "the members must share one window size"
            arr = (L.Wgrad * len(qs))(*qs)
            assert lib.nlam_wgrad_group(arr, len(qs), stream) == 0
            torch.cuda.synchronize()
            for k, (partials, _, _) in enumerate(members):
                assert torch.equal(partials, solo[k]), f"member {k} of m={m}"


# ---------------------------------------------------------------------------------------------------------------------------
# reductions: the documented summation order, emulated in float32
# ---------------------------------------------------------------------------------------------------------------------------
def emulate_reduce_jobs(P, prev, vec, waves):
    """reduce_jobs_kernel: wave w sums parts [w per, min(nparts, (w + 1) per)), per = ceil(nparts / waves) -- on the vector
    path in groups of 8 as ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)) with the last 1-7 parts added in part order, on the scalar path
    one part after the other; the waves' sums are added in wave order, then the value accumulated onto."""
    nparts = P.shape[0]
    per = -(-nparts // waves)
    t = None
    for w in range(waves):
        q0 = min(nparts, w * per)
        q1 = min(nparts, q0 + per)
        s = np.zeros(P.shape[1], np.float32)
        q = q0
        if vec:
            while q + 8 <= q1:
                v = P[q: q + 8]
                s = s + (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])))
                q += 8
        while q < q1:
            s = s + P[q]
            q += 1
        t = s if t is None else t + s
    return t if prev is None else t + prev


def emulate_reduce_partials(P, prev):
    """reduce_partials_kernel: four waves, parts in order inside a wave, combined as (r0 + r1) + (r2 + r3), then out + t."""
    nparts = P.shape[0]
    per = -(-nparts // RED_PARTIALS_WAVES)
    r = []
    for w in range(RED_PARTIALS_WAVES):
        s = np.zeros(P.shape[1], np.float32)
        for q in range(w * per, min(nparts, w * per + per)):
            s = s + P[q]
        r.append(s)
    t = (r[0] + r[1]) + (r[2] + r[3])
    return t if prev is None else prev + t


def _rand32(gen, shape):
    # mixed magnitudes: the summation order changes the rounded result
    x = torch.randn(shape, generator=gen, dtype=torch.float32) * (2.0 ** torch.randint(-12, 13, shape, generator=gen).float())
    return x


@pytest.mark.parametrize("nparts", [1, 3, 7, 8, 9, 31, 33, 512])
@pytest.mark.parametrize("path", ["vector", "scalar_n", "scalar_ptr", "columns", "accumulate"])
def test_reduce_jobs_order(lib, nparts, path):
    gen = torch.Generator().manual_seed(nparts)
    n = 1000 if path != "scalar_n" else 1001
    stride = n + (4 if path != "scalar_n" else 3)
    P = _rand32(gen, (nparts, stride))
    Pd = _alloc(P.numel(), torch.float32, 4 if path == "scalar_ptr" else 0, "cuda")
    Pd.copy_(P.reshape(-1).cuda())
    ncols, ld = (40, 52) if path == "columns" else (0, 0)
    rows_out = n // ncols if ncols else 1
    out_shape = (rows_out, ld) if ncols else (n,)
    init = _rand32(gen, out_shape)
    out = init.clone().cuda()
    jobs = L.ReduceJobs()
    jobs.njobs = 1
    j = jobs.job[0]
    j.partials, j.out, j.stride, j.nparts, j.n = Pd.data_ptr(), out.data_ptr(), stride, nparts, n
    j.accumulate, j.ncols, j.ld = int(path == "accumulate"), ncols, ld
    assert lib.nlam_reduce_jobs(C.byref(jobs), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    Pn = P[:, :n].numpy()
    prev = init.numpy().reshape(-1)[:n] if path == "accumulate" else None
    want = emulate_reduce_jobs(Pn, prev, vec=path in ("vector", "columns", "accumulate"), waves=lib.nlam_reduce_jobs_waves())
    expect = init.clone()
    if ncols:
        expect[:, :ncols] = torch.from_numpy(want.reshape(rows_out, ncols))   # columns past ncols are left as they were
    else:
        expect = torch.from_numpy(want)
    assert torch.equal(out.cpu(), expect)


def test_reduce_jobs_forty_jobs_in_one_launch(lib):
    gen = torch.Generator().manual_seed(40)
    jobs = L.ReduceJobs()
    jobs.njobs = L.NLAM_MAX_REDUCE_JOBS
    keep, want = [], []
    for k in range(jobs.njobs):
        nparts, n = 1 + (k * 7) % 40, 4 * (1 + (k * 13) % 300) + (k % 3 == 0)   # a third of them on the scalar path
        P = _rand32(gen, (nparts, n))
        init = _rand32(gen, (n,))
        Pd, out = P.cuda(), init.clone().cuda()
        j = jobs.job[k]
        j.partials, j.out, j.stride, j.nparts, j.n = Pd.data_ptr(), out.data_ptr(), n, nparts, n
        j.accumulate, j.ncols, j.ld = k % 2, 0, 0
        keep += [Pd, out]
        want.append((out, emulate_reduce_jobs(P.numpy(), init.numpy() if k % 2 else None, vec=n % 4 == 0, waves=lib.nlam_reduce_jobs_waves())))
    assert lib.nlam_reduce_jobs(C.byref(jobs), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    for k, (out, w) in enumerate(want):
        assert torch.equal(out.cpu(), torch.from_numpy(w)), f"job {k}"


@pytest.mark.parametrize("nparts", [1, 3, 7, 8, 9, 31, 33, 512])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_reduce_partials_order(lib, nparts, accumulate):
    gen = torch.Generator().manual_seed(100 + nparts)
    n, stride = 999, 1003
    P = _rand32(gen, (nparts, stride))
    init = _rand32(gen, (n,))
    Pd, out = P.cuda(), init.clone().cuda()
    assert lib.nlam_reduce_partials(Pd.data_ptr(), nparts, stride, n, out.data_ptr(), accumulate,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    want = emulate_reduce_partials(P[:, :n].numpy(), init.numpy() if accumulate else None)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
