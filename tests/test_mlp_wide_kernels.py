"""Kernel-level checks of the wide fused-MLP families (hid, dout or a source width above 64: nlam_mlp_fwd_family != 0) through the C
ABI, against the float64 math of mlp_kernel_ref.py: mlp_fwd_wide_kernel / mlp_bwd_wide_kernel (fp32 MFMA, nlam_wide.inc) and their
group forms, the split-bf16 super-tile template mlp_fwd_wbf_kernel / mlp_bwd_wbf_kernel and the software-pipelined
mlp_fwd_edge_kernel / mlp_bwd_edge_kernel (nlam_wbf.inc).

Every case names the instantiation (nlam_mlp_fwd_wide_plan / nlam_mlp_bwd_wide_plan: kernel, bf16 terms EXECUTED, plan, <NWV, FB>,
V4, bf16 storage) it is meant to run, under the tuning values it sets, and asserts both codes before it launches --
test_case_table_plans on the CPU, the GPU tests again -- so that none of the dispatch's quiet redirections (one term run as three
for an odd hidden block count, plan 4 for mid-size launches only, the edge kernels from 128 tiles) lets a case test another kernel.
test_every_reachable_plan_has_a_case lists what the dispatch tables can launch and compares it with the table.
Forward and backward run together; the backward once on the z1 / xhat / rstd the forward kernel saved and once on the reference's,
rounded to the storage type.  Every output is NaN-filled with NaN guard rows behind it, `wpack` too.
  (a) exact arithmetic: integer operands in a range chosen per case so that every sum of absolute values stays below 2^24
      (asserted in float64): z1 bit-equal in every executed mode (with bf16 storage: the exact value rounded once, to nearest even),
      the whole chain without activation and LayerNorm (fp32 family);
  (b) precision: |got - R| <= bound element by element, the first-order budget of mlp_kernel_ref.py; a tensor stored as bf16 takes
      one more relative rounding of 2^-8, carried into what reads it;
  (c) low-order probe, exact at any K: W1 = +-(1 + 2^-9 + 2^-18), input rows of at most 16 ones, integer bias -- z1 bit-equal to
      float64 where three terms or fp32 run, the integer count where one term runs (the low terms are dropped by contract).
The comparison functions are tested without a GPU at K = 512 and K = 1536: a stand-in kernel (the same MLP in torch fp32, bf16
rounding where a case stores bf16) passes, each of twelve injected defects is reported in the quantity it corrupts first."""
import ctypes as C
import json
import os
import time
from dataclasses import replace

import pytest
import torch

from neural_lam_amd import _lib as L

from mlp_kernel_ref import (Case, Dev, _combine, _same, _stream, _written, backward_math, build_problem,  # noqa: F401
                            compare_bounded, compare_exact, describe_bwd, describe_fwd, dsrc_rows, exact_headroom, exact_quantities,
                            exact_reference, forward_math, int_problem, low_reference, rand_problem, replace_case, standin_run,
                            to_bf16)

gpu = pytest.mark.gpu

WIDE, WBF, EDGE = L.MLPW_WIDE, L.MLPW_WBF, L.MLPW_EDGE
V4, SBF = L.MLPW_V4, L.MLPW_SBF
MIN_ST, HALF, TV4, TEDGE, CUS = L.TUNE_WBF_MIN_SUPERTILES, L.TUNE_WBF_HALF, L.TUNE_WBF_V4, L.TUNE_WBF_EDGE, L.TUNE_CHAIN_CUS
TUNE_DEFAULTS = {MIN_ST: 192, HALF: 1, TV4: 1, TEDGE: 1, CUS: 256}

_RATIOS = {}    # ("fwd" | "bwd", plan code) -> {quantity: largest |got - R| / bound over the tier-(b) runs}


def _note_ratio(which, code, name, ratio):
    d = _RATIOS.setdefault((which, int(code)), {})
    d[name] = max(d.get(name, 0.0), float(ratio))


def plan_name(which, code):
    if code <= 0:
        return str(code)
    k, ns, plan, nwv, fb, bits = L.mlpw_fields(code)
    d = "fwd" if which == "fwd" else "bwd"
    if k == WIDE:
        return f"mlp_{d}_wide_kernel<{nwv}, {fb}>"
    if k == EDGE:
        return f"mlp_{d}_edge_kernel<{ns}, {512 if ns == 1 else 256}, {'true' if bits & SBF else 'false'}>"
    return f"mlp_{d}_wbf_kernel NS{ns} plan {plan}" + (" SBF" if bits & SBF else "") + (" V4" if bits & V4 else "")


def set_tuning(lib, pairs=()):
    """The five launch-shape values at their defaults, then the case's own."""
    for k, v in {**TUNE_DEFAULTS, **dict(pairs)}.items():
        assert lib.nlam_set_tuning(k, v) == 0, (k, v)


@pytest.fixture
def tuned():
    """nlam_set_tuning is process-wide: whatever a test sets, the defaults are back when it ends."""
    lib = L.load()
    try:
        yield lambda pairs=(): set_tuning(lib, pairs)
    finally:
        set_tuning(lib)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib = L.load()
    t0 = time.time()
    yield lib
    path = os.environ.get("NLAM_MLP_WIDE_REPORT")
    if path and _RATIOS:
        rep = {"wall_seconds": round(time.time() - t0, 2),
               "ratios": [{"which": w, "code": c, "plan": plan_name(w, c), "max_ratio": v} for (w, c), v in sorted(_RATIOS.items())]}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def F32(nwv, fb):
    return L.mlpw_code(WIDE, 0, 0, nwv, fb)


def T(ns, plan, v4=True, sbf=False):
    return L.mlpw_code(WBF, ns, plan, bits=(V4 if v4 else 0) | (SBF if sbf else 0))


def E(ns, sbf=False):
    return L.mlpw_code(EDGE, ns, bits=SBF if sbf else 0)


# the persistent grid on 16 workgroups (two per CU slot for the 4-wave plans) and every launch a super-tile launch: 40 to 70 super
# tiles then make every workgroup walk several, an uneven number among them
BASE = ((MIN_ST, 0), (CUS, 16))
FWD_NRT = {1: 8, 2: 4, 3: 2, 4: 2, 5: 2, 6: 1, 7: 2}   # 32-row tiles per super tile (WbfPlan.nrt)
FWD_HALF = {1: 0, 2: 0, 3: 0, 5: 1, 6: 1, 7: 5}        # NLAM_TUNE_WBF_HALF that gives the forward plan (bit 1 is added for backward plan 5)
FWD_BWD = {1: 1, 2: 2, 3: 3, 4: 2, 5: 2, 6: 3, 7: 3}   # the backward plan of the same widths (8-wave)


def dense_rows(plan, batch, supers):
    """Rows per batch item: `supers` super tiles in all (about), a last super tile of 37 rows (one full tile and 5 rows)."""
    per = max(1, supers // batch)
    return 32 * FWD_NRT[plan] * per + 37


# geometry variants, dealt over the instantiations of each plan in rotation (profiles/mlp_wide_tests/README.md lists which plan
# misses which)
def geo_dense(plan, nsrc):
    return dict(rows=dense_rows(plan, 2, 44 if FWD_NRT[plan] > 1 and plan not in (5, 7) else 70), batch=2, broadcast=(1,), gather=(1,),
                perm=(0,), dmode=(1, 2, 1)[:nsrc], out_perm=True)


def geo_one_row(plan, nsrc):
    return dict(rows=1, batch=3, dmode=(1, 2, 2)[:nsrc])


def geo_mixed(plan, nsrc):
    assert nsrc == 3
    return dict(graph="mixed12", batch=3, aggregate=True, out_perm=True, dmode=(1, 2, 3), g_aggr=True, broadcast=(1,))


def geo_split_atomic(plan, nsrc):
    assert nsrc == 3
    return dict(graph="split9", batch=2, atomic=True, aggregate=True, out_perm=True, dmode=(1, 2, 3), g_aggr=True)


def geo_split_virtual(plan, nsrc):
    assert nsrc == 3
    return dict(graph="split9", batch=3, aggregate=True, want_out=False, dmode=(1, 0, 3), g_out=False, g_aggr=True, mean=True)


GEOS = (geo_dense, geo_mixed, geo_split_atomic, geo_one_row, geo_split_virtual)

# widths at the edges of each width class: (hid, dout, three source widths); hid with an even number of 32-column blocks for the
# one-term kernels (an odd count runs as three terms), hid a multiple of 4 but not of 32, a source of 8 columns, a source wider
# than hid; "R": dout no multiple of 4 (V4 off, dz2 32-padded: the kernel writes the real columns, the padding stays as the caller filled it)
SHAPES = {
    (1, 1): (128, 128, (128, 68, 128)), (1, 3): (68, 128, (128, 8, 128)), (1, "R"): (100, 34, (8, 128, 36)),
    (2, 1): (256, 132, (132, 256, 132)), (2, 3): (132, 256, (256, 8, 256)), (2, "R"): (164, 134, (8, 200, 136)),
    (3, 1): (512, 260, (260, 512, 260)), (3, 3): (260, 512, (512, 8, 512)), (3, "R"): (356, 270, (8, 512, 272)),
}
WCLASS = {1: 1, 2: 2, 3: 3, 4: 2, 5: 2, 6: 3, 7: 3}
SBF_SHAPES = {2: (256, 192, (192, 132, 192)), 3: (512, 320, (320, 260, 320))}


def _template_cases():
    out = []
    slot = {}
    for ns in (1, 3):
        for plan in ((1, 2, 3, 4, 5, 6, 7) if ns == 1 else (1, 2, 3, 4, 5)):
            for v4 in (True, False):
                i = slot[plan] = slot.get(plan, -1) + 1
                geo = GEOS[(i + plan) % len(GEOS)]
                ragged = not v4 and ns == 1   # V4 off through the widths (three terms: through NLAM_TUNE_WBF_V4 = 0)
                if ragged:                    # (no aggregation: with a dout that is no multiple of 4 it runs on the fp32 kernels)
                    geo = geo_one_row if plan in (2, 6) else geo_dense
                hid, dout, w3 = SHAPES[(WCLASS[plan], "R" if ragged else ns)]
                nsrc = 3 if geo in (geo_mixed, geo_split_atomic, geo_split_virtual) else 2
                kw = geo(plan, nsrc)
                widths = w3[:nsrc] if nsrc == 2 else (w3[0], w3[1], w3[2])
                bplan, half = FWD_BWD[plan], FWD_HALF.get(plan, 1)
                if bplan == 2 and ((plan == 2 and not v4) or (plan == 5 and v4) or (plan == 4 and ns == 3)):   # the 4-wave backward of 128 < d <= 256
                    bplan, half = 5, half | 2
                tune = BASE + ((HALF, half),) + (() if v4 or ragged else ((TV4, 0),))
                bwd = T(ns, bplan, v4)
                if plan == 4:   # mid-size launches under the default threshold: 48 .. 767 tiles
                    if i % 2 == 0:   # ~400 tiles: the backward (384 tiles from) is a super-tile launch too
                        kw = dict(rows=32 * 199 + 5, batch=2, dmode=(1, 2), gather=(1,), out_perm=True)
                    else:            # 60 tiles: the backward runs on the fp32 kernel
                        kw = dict(rows=32 * 19 + 5, batch=3, dmode=(1, 2), broadcast=(1,), gather=(1,))
                        bwd = F32(8, 1)
                    widths, nsrc = w3[:2], 2
                    tune = ((CUS, 16), (HALF, half)) + (() if v4 or ragged else ((TV4, 0),))
                add0 = widths[0] == dout and kw.get("want_out", True)
                add1 = nsrc == 3 and widths[1] == dout and not add0
                out.append(Case(f"t{ns}_p{plan}_{'v4' if v4 else ('rag' if ragged else 'nov4')}", T(ns, plan, v4), bwd, widths, hid, dout,
                                mm=(2 if (ns == 3 and i % 2) else ns), ln=(i + plan) % 3 != 2, add0=add0, add1=add1, acc0=(v4 and bwd != F32(8, 1) and not add0),
                                tune=tune, **kw))
    # bf16 storage: one term, whole 32-column blocks, sources above 8 columns
    for plan in (2, 3, 5, 6, 7):
        for v4 in (True, False):
            i = slot[plan] = slot.get(plan, -1) + 1
            geo = GEOS[(i + plan) % len(GEOS)]
            hid, dout, w3 = SBF_SHAPES[WCLASS[plan]]
            nsrc = 3 if geo in (geo_mixed, geo_split_atomic, geo_split_virtual) else 2
            kw = geo(plan, nsrc)
            bplan, half = FWD_BWD[plan], FWD_HALF[plan]
            if (plan == 2 and not v4) or (plan == 5 and v4):
                bplan, half = 5, half | 2
            tune = BASE + ((HALF, half),) + (() if v4 else ((TV4, 0),))
            out.append(Case(f"sbf_p{plan}_{'v4' if v4 else 'nov4'}", T(1, plan, v4, True), T(1, bplan, v4, True), w3[:nsrc], hid, dout, mm=1,
                            ln=i % 2 == 0, add0=kw.get("want_out", True), sbf=True, acc0=not v4 and not kw.get("want_out", True), tune=tune, **kw))
    return out


def _plan_case(name, ns, plan, geo, bwd, half, nsrc=3, threshold=False, **over):
    """One more case of forward plan `plan`: the geometries the rotation of _template_cases does not deal to that plan (three sources
    also for the dense and the one-row geometry: source 2 with dmode 1 and 2)."""
    hid, dout, w3 = SHAPES[(WCLASS[plan], ns)]
    kw = geo(plan, nsrc)
    tune = (((CUS, 16),) if threshold else BASE) + ((HALF, half),)
    return Case(name, T(ns, plan), bwd, w3[:nsrc], hid, dout, mm=ns, tune=tune, **{**kw, **over})


def _gap_cases():
    f41 = dict(widths=(128, 68, 128), hid=96, dout=128, tune=((CUS, 16),))
    f81 = dict(widths=(132, 256, 132), hid=200, dout=132, tune=((CUS, 16),))
    f82 = dict(widths=(260, 512, 260), hid=300, dout=260, tune=((CUS, 16),))
    return [
        _plan_case("p1_split_tiles_acc0", 1, 1, geo_split_atomic, T(1, 1), 0, acc0=True),
        _plan_case("p3_virtual_split", 1, 3, geo_split_virtual, T(1, 3), 0),
        _plan_case("p5_tile_list", 1, 5, geo_mixed, T(1, 5), 3, add0=True),
        _plan_case("p6_dense_three_sources", 1, 6, geo_dense, T(1, 3), 1, add0=True),
        _plan_case("p6_split_tiles", 1, 6, geo_split_atomic, T(1, 3), 1, ln=False),
        _plan_case("p7_one_row_three_sources", 1, 7, geo_one_row, T(1, 3), 5),
        _plan_case("p7_tile_list", 1, 7, geo_mixed, T(1, 3), 5, add0=True),
        # plan 4 exists between 48 and 767 tiles under the default threshold (no single row): tile lists of 129, 130 and 195 tiles; the
        # backward of so few tiles runs on the fp32 kernel
        _plan_case("p4_tile_list", 1, 4, geo_mixed, F32(8, 1), 1, threshold=True, add0=True),
        _plan_case("p4_split_tiles_ns3", 3, 4, geo_split_atomic, F32(8, 1), 1, threshold=True),
        _plan_case("p4_virtual_split", 1, 4, geo_split_virtual, F32(8, 1), 1, threshold=True),
        # the fp32 <4, 1> shape on every geometry
        Case("f32_41_tile_list", F32(4, 1), F32(4, 1), add0=True, **f41, **geo_mixed(0, 3)),
        Case("f32_41_split_tiles", F32(4, 1), F32(4, 1), ln=False, **f41, **geo_split_atomic(0, 3)),
        Case("f32_41_virtual_split", F32(4, 1), F32(4, 1), **f41, **geo_split_virtual(0, 3)),
        Case("f32_41_one_row", F32(4, 1), F32(4, 1), **f41, **{**geo_one_row(0, 3), "dmode": (2, 1, 1)}),
        # ... and what the <8, 1> and <8, 2> cases of the table's head leave out
        Case("f32_81_dense", F32(8, 1), F32(8, 1), add0=True, **f81, **geo_dense(2, 3)),
        Case("f32_81_one_row", F32(8, 1), F32(8, 1), **f81, **geo_one_row(0, 3)),
        Case("f32_81_virtual_split", F32(8, 1), F32(8, 1), **f81, **geo_split_virtual(0, 3)),
        Case("f32_82_split_tiles", F32(8, 2), F32(8, 2), **f82, **geo_split_atomic(0, 3)),
        Case("f32_82_tile_list", F32(8, 2), F32(8, 2), add0=True, **f82, **geo_mixed(0, 3)),
    ]


EDGE_GEO = dict(graph="mixed44", pre=True, aggregate=True, out_perm=True, g_aggr=True, add0=True)
CASES = [
    # ---- mlp_fwd_wide_kernel / mlp_bwd_wide_kernel (fp32 MFMA): matrix mode 0, NLAM_F_NO_ACT, widths that are no multiples of 4, and
    #      split modes below the super-tile threshold; the backward's shape follows the widest source with a data gradient
    Case("f32_41_noact_exact", F32(4, 1), F32(4, 1), (65, 7), 96, 65, rows=32 * 40 + 5, batch=2, ln=False, no_act=True, add0=True, gather=(1,),
         perm=(0,), dmode=(1, 2), out_perm=True, tune=((CUS, 16),)),
    Case("f32_41_hid_narrow", F32(4, 1), F32(8, 1), (200, 12), 48, 17, rows=32 * 33 + 1, broadcast=(1,), dmode=(2, 1), tune=((CUS, 16),)),
    Case("f32_81_mm3_ragged_width", F32(8, 1), F32(8, 1), (100, 38, 136), 200, 136, mm=3, tune=BASE, **{**geo_mixed(0, 3), "batch": 2}),
    Case("f32_81_noact_atomic_exact", F32(8, 1), F32(8, 2), (260, 132, 132), 132, 132, ln=False, no_act=True, add1=True,
         **geo_split_atomic(0, 3), tune=((CUS, 16),)),
    Case("f32_82_ragged_mm1", F32(8, 2), F32(8, 2), (30, 262), 300, 512, rows=32 * 20 + 31, batch=2, mm=1, gather=(0,), dmode=(2, 1), tune=BASE),
    Case("f32_82_virtual_split_mean", F32(8, 2), F32(8, 2), (512, 64, 512), 260, 512, add0=True, **geo_split_virtual(0, 3)),
    Case("f32_82_one_row", F32(8, 2), F32(8, 2), (8, 16), 512, 66, rows=1, batch=3, dmode=(0, 0), tune=((CUS, 16),)),
    *_template_cases(),
    *_gap_cases(),
    # ---- one requested term with an odd number of hidden blocks: the forward runs three terms, the backward one
    Case("odd_hidden_blocks_1_as_3", T(3, 1), T(1, 1), (128, 96), 96, 128, mm=1, add0=True, tune=BASE + ((HALF, 0),), **geo_dense(1, 2)),
    # ---- aggregation with an output width that is no multiple of 4: the super-tile forward reduces whole float4s, so the launch runs on
    #      the fp32 kernel (the backward, whose segment sums are over source widths, stays on the split-bf16 kernel, dz2 padded)
    Case("ragged_dout_aggregated", F32(8, 2), T(1, 3, False), (8, 512, 272), 356, 270, mm=1, tune=BASE + ((HALF, 0),), **geo_mixed(3, 3)),
    # ---- NLAM_F_ADD_SRC1 on the template kernels (msg = mlp + src[1] goes into the aggregate and, with `out`, into the row output)
    Case("add_src1_p2", T(1, 2), T(1, 2), (256, 132, 132), 256, 132, mm=1, add1=True, tune=BASE + ((HALF, 0),), **geo_mixed(2, 3)),
    Case("add_src1_p3_ns3", T(3, 3), T(3, 3), (8, 512, 260), 260, 512, mm=3, add1=True, tune=BASE + ((HALF, 0),), **geo_split_atomic(3, 3)),
    # ---- hid below 64 under a wide source (and a factorised layer on the template kernels: ldw1 beyond the width sum)
    Case("hid64_wide_source", T(1, 1), T(1, 1), (128, 72), 64, 64, mm=1, tune=BASE, **geo_dense(1, 2)),
    Case("pre_template_d512", T(1, 6), T(1, 3), (260, 512, 512), 512, 512, mm=1, pre=True, ldw1_extra=1028, graph="mixed12", batch=3,
         aggregate=True, out_perm=True, dmode=(1, 0, 3), g_aggr=True, tune=BASE + ((TEDGE, 0),)),
    Case("pre_template_d128_ns3", T(3, 1), T(3, 1), (68, 128, 128), 128, 128, mm=3, pre=True, ldw1_extra=300, graph="split9", batch=2,
         aggregate=True, out_perm=True, dmode=(1, 0, 3), g_aggr=True, tune=BASE),
    # ---- mlp_fwd_edge_kernel / mlp_bwd_edge_kernel: three sources of width d, LayerNorm, aggregation, 128 tiles or more
    Case("edge_1_512", E(1), E(1), (512, 512, 512), 512, 512, mm=1, dmode=(1, 0, 3), acc0=True, tune=((CUS, 16),), **EDGE_GEO),   # (acc0: the rollout's shape)
    Case("edge_1_512_sbf_mean", E(1, True), E(1, True), (512, 512, 512), 512, 512, mm=1, sbf=True, mean=True, dmode=(1, 0, 3),
         tune=((CUS, 16),), **EDGE_GEO),
    Case("edge_3_256_no_dsrc0", E(3), E(3), (256, 256, 256), 256, 256, mm=3, dmode=(0, 0, 3), tune=BASE, **EDGE_GEO),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# (int_problem, exact_headroom, rand_problem, low_reference, standin_run and replace_case live in mlp_kernel_ref.py: the tiled-GEMM
# file uses them too)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker's own test: a CPU stand-in for the kernel at K = 512 and K = 1536, and twelve injected defects (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------
STANDIN_1536 = Case("standin_k1536", 0, 0, (512, 512, 512), 512, 512, graph="mixed12", add0=True, aggregate=True, out_perm=True,
                    dmode=(1, 2, 3), g_aggr=True)
STANDIN_512 = Case("standin_k512", 0, 0, (256, 128, 128), 320, 256, graph="split9", add0=True, aggregate=True, out_perm=True,
                   dmode=(1, 2, 3), g_aggr=True, acc0=True)
DEFECTS = ["drop_input_column", "swap_gather_indices", "omit_residual", "tile_last_row_not_aggregated", "rstd_without_eps",
           "sigmoid_for_silu_derivative", "skip_vec_partials_block", "drop_w1_third_term",
           "supertile_last_row_from_neighbour", "drop_dout_block_in_gemm2", "dsrc0_overwritten", "z1_truncated_bf16"]
FIRST = {"drop_input_column": "z1", "swap_gather_indices": "z1", "omit_residual": "out", "tile_last_row_not_aggregated": "aggr",
         "rstd_without_eps": "rstd", "sigmoid_for_silu_derivative": "dz1", "skip_vec_partials_block": "db1", "drop_w1_third_term": "z1",
         "supertile_last_row_from_neighbour": "z1", "drop_dout_block_in_gemm2": "xhat", "dsrc0_overwritten": "dsrc0",
         "z1_truncated_bf16": "z1"}


@pytest.mark.parametrize("case", [STANDIN_512, STANDIN_1536], ids=str)
def test_standin_passes_at_wide_sizes(case):
    for c in (case, replace(case, ln=False, no_act=True, acc0=False), replace(case, ln=False), replace(case, sbf=True),
              replace(case, mean=True, add0=False, add1=case.widths[1] == case.dout)):
        assert standin_run(c, "int") == [], c
        assert standin_run(c, "rand") == [], c
    assert standin_run(case, "low", ns_claimed=3) == []


@pytest.mark.parametrize("defect", DEFECTS)
def test_injected_defect_is_reported(defect):
    """Each defect must fail the comparison at K = 1536 (K = 512 where the defect needs NLAM_F_ACC_DSRC0), in the quantity it
    corrupts first."""
    first = FIRST[defect]
    case = STANDIN_1536
    if defect == "drop_w1_third_term":   # the worst-case budget at K = 1536 would hide it: the exact probe does not
        assert standin_run(case, "low", defect, ns_claimed=3) == ["z1"]
        return
    if defect == "rstd_without_eps":   # rows of nearly equal outputs: eps is then a visible part of the variance
        P = build_problem(case, 7, "rand")
        P.W2, P.b2 = (P.W2 * 2.0 ** -9).float().double(), (P.b2 * 2.0 ** -9).float().double()
        ref_f, bud_f = forward_math(P)
        assert compare_bounded(forward_math(P, torch.float32)[0], ref_f, bud_f) == []
        bad = compare_bounded(forward_math(P, torch.float32, defect=defect)[0], ref_f, bud_f)
        assert first in bad, (defect, bad)
        return
    if defect == "dsrc0_overwritten":
        case = STANDIN_512
    if defect == "z1_truncated_bf16":
        case = replace(case, sbf=True)
    bad_b = standin_run(case, "rand", defect)
    upstream = {"z1": (), "xhat": ("z1",), "out": ("z1", "xhat", "rstd"), "aggr": ("z1", "xhat", "rstd"),
                "dz1": ("z1", "xhat", "rstd", "out", "aggr", "dz2"), "db1": ("z1", "xhat", "rstd", "out", "aggr", "dz2", "dz1"),
                "dsrc0": ("z1", "xhat", "rstd", "out", "aggr", "dz2", "dz1")}[first]
    assert first in bad_b and not set(bad_b) & set(upstream), (defect, bad_b)
    if defect in ("drop_input_column", "swap_gather_indices", "supertile_last_row_from_neighbour", "z1_truncated_bf16"):
        assert "z1" in standin_run(case, "int", defect), defect
    if defect in ("omit_residual", "tile_last_row_not_aggregated", "skip_vec_partials_block"):
        bad_a = standin_run(replace(case, ln=False, no_act=True), "int", defect)
        assert first in bad_a, (defect, bad_a)


# ---------------------------------------------------------------------------------------------------------------------------
# the plan table (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def _fake(P):
    return lambda n: None if ((n.startswith("idx") and P.srcs[int(n[3:])].idx is None) or (n == "tiles" and P.tiles is None)
                              or (n == "out_idx" and P.out_idx is None)) else 4096


def describe_both(lib, P, addr=None):
    """Both descriptors with `wpack` set (placeholder addresses unless addr is given: host logic only)."""
    a = addr if addr is not None else _fake(P)
    pf = describe_fwd(P, a)
    pf.wpack, pf.wpack_floats = 4096, 1 << 40
    pb = describe_bwd(P, a, lib)
    pb.wpack, pb.wpack_floats = 4096, 1 << 40
    return pf, pb


def test_case_table_plans(tuned):
    """Host logic only: under its tuning every case hits the two instantiations it names."""
    lib = L.load()
    for c in CASES:
        tuned(c.tune)
        P = build_problem(c, 1, "int")
        pf, pb = describe_both(lib, P)
        assert lib.nlam_mlp_fwd_family(C.byref(pf)) != 0 and lib.nlam_mlp_bwd_family(C.byref(pb)) != 0, c.name
        assert lib.nlam_mlp_fwd_plan(C.byref(pf)) == L.MLPP_NOT_NARROW and lib.nlam_mlp_bwd_plan(C.byref(pb)) == L.MLPP_NOT_NARROW
        got_f, got_b = lib.nlam_mlp_fwd_wide_plan(C.byref(pf)), lib.nlam_mlp_bwd_wide_plan(C.byref(pb))
        assert got_f == c.fwd, (c.name, plan_name("fwd", got_f), plan_name("fwd", c.fwd))
        assert got_b == c.bwd, (c.name, plan_name("bwd", got_b), plan_name("bwd", c.bwd))
        padded = c.dout % 4 != 0 and L.mlpw_fields(c.bwd)[0] != WIDE
        assert pb.dz2_ld == (32 * -(-c.dout // 32) if padded else 0), c.name
        assert (lib.nlam_mlp_fwd_family(C.byref(pf)) == 1) == (L.mlpw_fields(c.fwd)[0] == WIDE)
        assert (lib.nlam_mlp_bwd_family(C.byref(pb)) == 1) == (L.mlpw_fields(c.bwd)[0] == WIDE)
        if c.sbf:
            assert lib.nlam_store_bf16_supported(C.byref(pf)) == 1
        if "edge" in c.name:   # the geometry the edge kernels' pipeline is tested on
            assert P.ntiles >= 128 and ((P.ntiles + 1) // 2) % 2 == 1, (c.name, P.ntiles)
        if c.graph:
            assert P.ntiles % 2 == 1, (c.name, P.ntiles)   # no multiple of any plan's tiles per super tile


def test_every_reachable_plan_has_a_case():
    """The instantiations fwd_wide / fwd_wbf / bwd_wide / bwd_wbf can launch, listed from their switches, against the case table."""
    fwd = {F32(4, 1), F32(8, 1), F32(8, 2)}                                              # pick_wide
    fwd |= {T(1, p, v) for p in range(1, 8) for v in (True, False)}                      # one term
    fwd |= {T(1, p, v, True) for p in (2, 3, 5, 6, 7) for v in (True, False)}            # one term, bf16 storage
    fwd |= {T(3, p, v) for p in range(1, 6) for v in (True, False)}                      # three terms
    fwd |= {E(1), E(1, True), E(3)}                                                      # mlp_fwd_edge_kernel
    bwd = {F32(4, 1), F32(8, 1), F32(8, 2)}
    bwd |= {T(ns, p, v) for ns in (1, 3) for p in (1, 2, 3, 5) for v in (True, False)}
    bwd |= {T(1, p, v, True) for p in (2, 3, 5) for v in (True, False)}
    bwd |= {E(1), E(1, True), E(3)}
    assert (len(fwd), len(bwd)) == (40, 28)
    hit_f, hit_b = {c.fwd for c in CASES}, {c.bwd for c in CASES}
    assert hit_f <= fwd and hit_b <= bwd, "a case names a code the dispatch cannot produce"
    assert not (fwd - hit_f), sorted(plan_name("fwd", x) for x in fwd - hit_f)
    assert not (bwd - hit_b), sorted(plan_name("bwd", x) for x in bwd - hit_b)


def test_refusals_match_the_launch(tuned):
    """What nlam_mlp_fwd / nlam_mlp_bwd refuse, the plan query refuses with the same code.  Every pair below is (query, launch)
    against the code the header documents.  The descriptors hold placeholder addresses, so the launch entry points are called
    ONLY where no device is visible (a launch that slipped through could then run nothing): there the pair compares the query
    with the launch.  With a device the second element repeats the query, and the test checks the query against the documented
    code alone; query and launch share fwd_check / bwd_check and fwd_wide_plan / bwd_wide_plan."""
    lib = L.load()
    ask_launch = not torch.cuda.is_available()

    def both(pf=None, pb=None):
        r = []
        if pf is not None:
            q = lib.nlam_mlp_fwd_wide_plan(C.byref(pf))
            r.append((q, lib.nlam_mlp_fwd(C.byref(pf), None) if (ask_launch and q < 0) else q))
        if pb is not None:
            q = lib.nlam_mlp_bwd_wide_plan(C.byref(pb))
            r.append((q, lib.nlam_mlp_bwd(C.byref(pb), None) if (ask_launch and q < 0) else q))
        return r

    base = CASE_BY_NAME["t1_p2_v4"]
    tuned(base.tune)
    P = build_problem(base, 1, "int")
    # NLAM_F_PRE_ADD on the fp32 family (matrix mode 0)
    Pp = build_problem(replace(CASE_BY_NAME["pre_template_d128_ns3"], mm=0), 1, "int")
    assert both(*describe_both(lib, Pp)) == [(-2, -2), (-2, -2)]
    # NLAM_F_STORE_BF16 outside nlam_store_bf16_supported (three terms; plan 1; a source of 8 columns)
    for c in (replace(base, sbf=True, mm=3), replace(CASE_BY_NAME["t1_p1_v4"], sbf=True), replace(CASE_BY_NAME["sbf_p2_v4"], widths=(192, 8))):
        Ps = build_problem(replace(c, add0=False, add1=False, acc0=False), 1, "int")
        pf, pb = describe_both(lib, Ps)
        assert lib.nlam_store_bf16_supported(C.byref(pf)) == 0, c
        assert both(pf) == [(-2, -2)], c
    pf, pb = describe_both(lib, build_problem(replace(base, sbf=True, mm=3, acc0=False), 1, "int"))
    assert both(None, pb) == [(-2, -2)]
    # NLAM_F_ACC_DSRC0 on family 1
    Pa = build_problem(replace(CASE_BY_NAME["f32_41_noact_exact"], acc0=True), 1, "int")
    pf, pb = describe_both(lib, Pa)
    assert lib.nlam_mlp_bwd_family(C.byref(pb)) == 1 and both(None, pb) == [(-2, -2)]
    # a too-small wpack, a missing one
    pf, pb = describe_both(lib, P)
    pf.wpack_floats, pb.wpack_floats = lib.nlam_mlp_fwd_wpack_floats(C.byref(pf)) - 1, lib.nlam_mlp_bwd_wpack_floats(C.byref(pb)) - 1
    assert both(pf, pb) == [(-1, -1), (-1, -1)]
    pf, pb = describe_both(lib, P)
    pf.wpack = pb.wpack = None
    assert both(pf, pb) == [(-1, -1), (-1, -1)]
    # a wrong dz2_ld
    pf, pb = describe_both(lib, P)
    pb.dz2_ld = 32 * -(-base.dout // 32)
    assert both(None, pb) == [(-1, -1)]
    pf, pb = describe_both(lib, build_problem(CASE_BY_NAME["t1_p1_rag"], 1, "int"))
    assert pb.dz2_ld == 64
    pb.dz2_ld = 0
    assert both(None, pb) == [(-1, -1)]
    # a width above nlam_max_width()
    assert lib.nlam_max_width() == 512
    pf, pb = describe_both(lib, P)
    pf.hid = pb.hid = 516
    assert both(pf, pb) == [(-2, -2), (-2, -2)]
    # not wide; no rows
    pf, pb = describe_both(lib, build_problem(Case("narrow", 0, 0, (64,), 64, 64, rows=5), 1, "int"))
    assert lib.nlam_mlp_fwd_wide_plan(C.byref(pf)) == L.MLPW_NOT_WIDE and lib.nlam_mlp_bwd_wide_plan(C.byref(pb)) == L.MLPW_NOT_WIDE
    pf, pb = describe_both(lib, P)
    pf.rows = pb.rows = 0
    assert lib.nlam_mlp_fwd_wide_plan(C.byref(pf)) == L.MLPW_EMPTY and lib.nlam_mlp_bwd_wide_plan(C.byref(pb)) == L.MLPW_EMPTY


# ---------------------------------------------------------------------------------------------------------------------------
# GPU side: the launches
# ---------------------------------------------------------------------------------------------------------------------------
def _store_dtype(c):
    return torch.bfloat16 if c.sbf else torch.float32


def prep_forward(lib, P, dev, ready=False):
    """Fresh NaN-filled outputs (and a fresh NaN-filled, guarded wpack unless `ready`: then the image dev.t["wpack_f"] already holds
    is used with NLAM_F_WPACK_READY) -> the filled nlam_mlp_fwd_t, its plan code asserted."""
    c = P.case
    keep_wpack = dev.outs.get("wpack_f") if ready else None
    dev.outs = {}
    if c.want_out:
        dev.out("out", (P.batch, P.out_rows, c.dout))
    if c.aggregate:
        dev.out("aggr", (P.batch, P.nseg_rows, c.dout), zero=P.has_split)
    dev.out("z1", (P.batch, P.rows, c.hid), dtype=_store_dtype(c))
    if c.ln:
        dev.out("xhat", (P.batch, P.rows, c.dout), dtype=_store_dtype(c))
        dev.out("rstd", (P.batch, P.rows))
    p = describe_fwd(P, dev.addr)
    p.wpack, p.wpack_floats = 4096, 1 << 40   # placeholder: the size query below must not depend on it
    need = lib.nlam_mlp_fwd_wpack_floats(C.byref(p))
    assert need > 0
    if ready:
        dev.outs["wpack_f"] = keep_wpack
        p.flags |= L.F_WPACK_READY
    else:
        dev.out("wpack_f", (need,))
    p.wpack, p.wpack_floats = dev.addr("wpack_f"), need
    got = lib.nlam_mlp_fwd_wide_plan(C.byref(p))
    assert got == c.fwd, (c.name, plan_name("fwd", got), plan_name("fwd", c.fwd))
    return p


def collect_forward(lib, P, dev):
    """After the launch: nlam_split_combine where the case has a virtual split, the guards -> host tensors in fp32."""
    c = P.case
    if c.aggregate and P.comb is not None:
        _combine(lib, dev, dev.t["aggr"], c.dout)
    torch.cuda.synchronize()
    assert dev.guards_intact() == [], f"{c.name}: forward wrote behind an output"
    res = {n: dev.t[n].float().cpu() for n in dev.outs if n != "wpack_f"}
    if c.aggregate:
        res["aggr"] = res["aggr"][:, : P.nseg]
    return res


def run_forward(lib, P, dev, ready=False):
    """One nlam_mlp_fwd launch -> host tensors in fp32."""
    p = prep_forward(lib, P, dev, ready)
    assert lib.nlam_mlp_fwd(C.byref(p), _stream()) == 0, P.case.name
    return collect_forward(lib, P, dev)


def prep_backward(lib, P, dev, saved, ready=False):
    """Fresh NaN-filled outputs for a backward on the saved tensors `saved` (device, in the storage type) -> the filled
    nlam_mlp_bwd_t (plan code asserted) and the rows of vec_partials a single launch writes (its capacity)."""
    c = P.case
    keep_wpack = dev.outs.get("wpack_b") if ready else None
    dev.outs = {}
    for n in ("z1", "xhat", "rstd"):
        if n in saved:
            dev.t[n] = saved[n]
    p = describe_bwd(P, dev.addr, lib)   # placeholder outputs: what decides the kernel is set
    ld = p.dz2_ld if p.dz2_ld else c.dout
    dev.out("dz1", (P.batch * P.rows, c.hid), dtype=_store_dtype(c))
    dz2_dev = dev.out("dz2", (P.batch * P.rows, ld), dtype=_store_dtype(c))
    if ld != c.dout:   # the wide kernels write the dout real columns only: the padding is the caller's, zero-filled (nlam_mlp_bwd_t.dz2_ld)
        dz2_dev[:, c.dout:] = 0
    for k in range(P.nsrc):
        if c.dmode[k] != 0:
            t = dev.out(f"dsrc{k}", (P.batch, dsrc_rows(P, k), c.widths[k]), zero=c.dmode[k] == 3 and P.has_split)
            if k == 0 and c.acc0:
                t.copy_(P.dsrc0_init.float())
    p = describe_bwd(P, dev.addr, lib)
    p.wpack, p.wpack_floats = 4096, 1 << 40
    need = lib.nlam_mlp_bwd_wpack_floats(C.byref(p))
    assert need > 0
    if ready:
        dev.outs["wpack_b"] = keep_wpack
        p.flags |= L.F_WPACK_READY
    else:
        dev.out("wpack_b", (need,))
    p.wpack, p.wpack_floats = dev.addr("wpack_b"), need
    nblk = lib.nlam_mlp_bwd_blocks(C.byref(p))
    assert nblk >= 1
    vs = 64 * -(-max(c.hid, c.dout) // 64)
    vec = dev.out("vec", (nblk, 4, vs))
    p.vec_partials, p.vec_partials_rows, p.vec_stride = vec.data_ptr(), nblk, vs
    got = lib.nlam_mlp_bwd_wide_plan(C.byref(p))
    assert got == c.bwd, (c.name, plan_name("bwd", got), plan_name("bwd", c.bwd))
    return p, nblk


def collect_backward(lib, P, dev, nblk, ld):
    """After the launch -> host tensors + the four vectors (the first nblk rows of vec_partials) summed in float64."""
    c = P.case
    for k in range(P.nsrc):
        if c.dmode[k] == 3 and P.comb is not None:
            _combine(lib, dev, dev.t[f"dsrc{k}"], c.widths[k])
    torch.cuda.synchronize()
    assert dev.guards_intact() == [], f"{c.name}: backward wrote behind an output"
    res = {n: dev.t[n].float().cpu() for n in dev.outs if n != "wpack_b"}
    res["dz1"] = res["dz1"].reshape(P.batch, P.rows, c.hid)
    dz2 = res["dz2"].reshape(P.batch, P.rows, ld)
    if ld != c.dout:
        assert torch.count_nonzero(dz2[..., c.dout:]) == 0 and torch.isfinite(dz2).all(), f"{c.name}: the zero-filled padding columns of dz2 must stay zeros"
    res["dz2"] = dz2[..., : c.dout].contiguous()
    for k in range(P.nsrc):
        if c.dmode[k] == 3:
            res[f"dsrc{k}"] = res[f"dsrc{k}"][:, : P.nseg]
    v = res.pop("vec").double()
    assert bool(torch.isnan(v[nblk:]).all()), f"{c.name}: rows of vec_partials behind the launch's workgroups were written"
    v = v[:nblk]
    res["db1"], res["db2"] = v[:, 0, : c.hid].sum(0), v[:, 1, : c.dout].sum(0)
    if c.ln:
        res["dgamma"], res["dbeta"] = v[:, 2, : c.dout].sum(0), v[:, 3, : c.dout].sum(0)
    res["_nblk"] = nblk
    return res


def run_backward(lib, P, dev, saved, ready=False):
    """One nlam_mlp_bwd launch -> host tensors + the four vectors summed in float64."""
    p, nblk = prep_backward(lib, P, dev, saved, ready)
    assert lib.nlam_mlp_bwd(C.byref(p), _stream()) == 0, P.case.name
    return collect_backward(lib, P, dev, nblk, p.dz2_ld if p.dz2_ld else P.case.dout)


def _same_fixed_order(case, a, b):
    """_same over what is summed in a fixed order: the aggregates and dmode-3 gradients of NLAM_TILE_SPLIT tiles are atomic sums
    in no fixed order and are never compared bitwise."""
    loose = {"aggr"} | {f"dsrc{k}" for k, m in enumerate(case.dmode) if m == 3} if case.atomic else set()
    return [n for n in _same(a, b) if n not in loose]


def _saved_dev(c, res):
    return {n: res[n].to(_store_dtype(c) if n != "rstd" else torch.float32).cuda() for n in ("z1", "xhat", "rstd") if n in res}


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_exact_on_integers(lib, tuned, case):
    """Tier (a): integer operands; z1 in every instantiation, and the whole chain where no rounding can occur, bit-equal to float64."""
    tuned(case.tune)
    P = int_problem(case, 11)
    dev = Dev(P)
    got_f = run_forward(lib, P, dev)
    _written(got_f, f"{case} forward")
    ref_f, _ = forward_math(P)
    assert compare_exact(got_f, exact_reference(case, ref_f, True), exact_quantities(case, True)) == [], f"{case}: forward is not the exact result"
    got_b = run_backward(lib, P, dev, _saved_dev(case, got_f))
    _written(got_b, f"{case} backward")
    ref_b, _ = backward_math(P, {k: got_f[k].double() for k in ("z1", "xhat", "rstd") if k in got_f})
    assert compare_exact(got_b, ref_b, exact_quantities(case, False)) == [], f"{case}: backward is not the exact result"
    if case.acc0 and not case.add0:
        # NLAM_F_ACC_DSRC0 adds the gradient to what dsrc[0] holds: one fp32 addition to the gradient the launch without the flag writes
        Q = replace_case(P, acc0=False)
        plain = run_backward(lib, Q, Dev(Q), _saved_dev(case, got_f))
        assert torch.equal(got_b["dsrc0"], plain["dsrc0"] + P.dsrc0_init.float()), f"{case}: dsrc[0] is not what it held plus the gradient"


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_elementwise_error_budget(lib, tuned, case):
    """Tier (b): every output, saved tensor, gradient and vector within its propagated budget; the stages behind GEMM1 also on
    their own (continued from the kernel's z1); the backward on the kernel's saved tensors and on the reference's; two launches of
    a case without atomic adds are bit-equal."""
    tuned(case.tune)
    P = rand_problem(case, 12)
    dev = Dev(P)
    ns_f, ns_b = L.mlpw_fields(case.fwd)[1], L.mlpw_fields(case.bwd)[1]
    got_f = run_forward(lib, P, dev)
    _written(got_f, f"{case} forward")
    keep = _saved_dev(case, got_f)
    if not case.atomic:
        assert _same(got_f, run_forward(lib, P, dev)) == [], f"{case}: two forward launches differ"
    ref_f, bud_f = forward_math(P, ns=ns_f)
    note_f = lambda n, r: _note_ratio("fwd", case.fwd, n, r)
    bad = compare_bounded(got_f, ref_f, bud_f, note=note_f)
    ref_2, bud_2 = forward_math(P, ns=ns_f, z1_given=got_f["z1"].double())
    later = [n for n in ref_2 if n != "z1"]
    bad += [n + "|z1" for n in compare_bounded(got_f, ref_2, bud_2, names=later, note=lambda n, r: note_f(n + "|z1", r))]
    assert bad == [], f"{case}: forward over its budget in {bad}; ratios {_RATIOS[('fwd', case.fwd)]}"
    note_b = lambda n, r: _note_ratio("bwd", case.bwd, n, r)
    got_b = run_backward(lib, P, dev, keep)
    _written(got_b, f"{case} backward")
    if not case.atomic:
        assert _same(got_b, run_backward(lib, P, dev, keep)) == [], f"{case}: two backward launches differ"
    ref_b, bud_b = backward_math(P, {k: got_f[k].double() for k in keep}, ns=ns_b, nblk=got_b["_nblk"])
    bad = compare_bounded(got_b, ref_b, bud_b, note=note_b)
    assert bad == [], f"{case}: backward (on the kernel's saved tensors) over its budget in {bad}; ratios {_RATIOS[('bwd', case.bwd)]}"
    rounded = {k: (to_bf16(ref_f[k].float()) if (case.sbf and k != "rstd") else ref_f[k].float()) for k in keep}   # the reference's, as stored
    got_r = run_backward(lib, P, dev, _saved_dev(case, rounded))
    ref_r, bud_r = backward_math(P, {k: v.double() for k, v in rounded.items()}, ns=ns_b, nblk=got_r["_nblk"])
    bad = compare_bounded(got_r, ref_r, bud_r, note=note_b)
    assert bad == [], f"{case}: backward (on the reference's saved tensors) over its budget in {bad}"


PROBE_CASES = [c for c in CASES if L.mlpw_fields(c.fwd)[1] == 3 or c.name in ("f32_82_ragged_mm1", "t1_p3_v4", "t1_p5_v4", "sbf_p6_v4", "edge_1_512")]


@gpu
@pytest.mark.parametrize("case", PROBE_CASES, ids=str)
def test_gemm1_low_order_terms(lib, tuned, case):
    """Tier (c): every three-term forward code (mlp_fwd_edge_kernel<3, 256> among them) and the fp32 family keep all three bf16
    terms of W1 -- z1 bit-equal to float64; the one-term codes give the integer count (the low terms are dropped by contract)."""
    tuned(case.tune)
    P = build_problem(case, 13, "low")
    got = run_forward(lib, P, Dev(P))
    ns = L.mlpw_fields(case.fwd)[1]
    assert torch.equal(got["z1"].double(), low_reference(P, ns)), f"{case}: z1 of the low-order probe ({ns} terms)"


V4_CASES = ["t1_p1_v4", "t3_p2_v4", "t1_p6_v4", "sbf_p3_v4", "t3_p5_v4"]


@gpu
@pytest.mark.parametrize("name", V4_CASES)
def test_v4_accessors_are_bit_identical(lib, tuned, name):
    """The same launch with NLAM_TUNE_WBF_V4 = 1 and 0: the V4 and the generic accessors give the same bits, forward and backward."""
    case = CASE_BY_NAME[name]
    P = rand_problem(case, 15)
    tuned(case.tune)
    dev = Dev(P)
    on_f = run_forward(lib, P, dev)
    keep = _saved_dev(case, on_f)
    on_b = run_backward(lib, P, dev, keep)
    off = replace(case, fwd=case.fwd & ~V4, bwd=case.bwd & ~V4, tune=case.tune + ((TV4, 0),))
    tuned(off.tune)
    Q = replace_case(P, fwd=off.fwd, bwd=off.bwd)
    off_f = run_forward(lib, Q, dev)
    off_b = run_backward(lib, Q, dev, keep)
    assert _same_fixed_order(case, on_f, off_f) == [] and _same_fixed_order(case, on_b, off_b) == [], name


PACK_CASES = ["f32_81_mm3_ragged_width", "t1_p2_v4", "t3_p3_v4"]   # record kinds 0, 1 and 3


@gpu
@pytest.mark.parametrize("name", PACK_CASES)
def test_pack_records_image_is_bit_identical(lib, tuned, name):
    """A launch with NLAM_F_WPACK_READY on the image nlam_pack_records wrote from nlam_mlp_*_pack_records equals the launch that
    packs its weights itself."""
    case = CASE_BY_NAME[name]
    tuned(case.tune)
    P = rand_problem(case, 14)
    dev = Dev(P)
    plain_f = run_forward(lib, P, dev)
    keep = _saved_dev(case, plain_f)
    plain_b = run_backward(lib, P, dev, keep)
    kinds = []
    for which in ("f", "b"):
        # the launch's own descriptor, with a fresh NaN-filled image of exactly the announced size
        if which == "f":
            run_forward(lib, P, dev)
            p = describe_fwd(P, dev.addr)
            need, fn, key = lib.nlam_mlp_fwd_wpack_floats, lib.nlam_mlp_fwd_pack_records, "wpack_f"
        else:
            run_backward(lib, P, dev, keep)
            p = describe_bwd(P, dev.addr, lib)
            need, fn, key = lib.nlam_mlp_bwd_wpack_floats, lib.nlam_mlp_bwd_pack_records, "wpack_b"
        p.wpack, p.wpack_floats = 4096, 1 << 40
        n = need(C.byref(p))
        buf = dev.outs[key][0]
        buf.fill_(float("nan"))
        p.wpack, p.wpack_floats = buf.data_ptr(), n
        recs, kind = (L.PackRec * 4)(), C.c_int32(-1)
        nrec = fn(C.byref(p), recs, 4, C.byref(kind))
        assert 1 <= nrec <= 4, (name, which, nrec)
        kinds.append(kind.value)
        table = torch.frombuffer(bytearray(bytes(recs)[: 64 * nrec]), dtype=torch.uint8).cuda()
        assert lib.nlam_pack_records(C.c_void_p(table.data_ptr()), nrec, kind.value, _stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[n:]).all()), f"{name}: the pack wrote behind the announced size"
        if which == "f":
            assert _same_fixed_order(case, plain_f, run_forward(lib, P, dev, ready=True)) == [], f"{name}: forward on the packed image differs"
        else:
            assert _same_fixed_order(case, plain_b, run_backward(lib, P, dev, keep, ready=True)) == [], f"{name}: backward on the packed image differs"
    want = {"f32_81_mm3_ragged_width": 0, "t1_p2_v4": 1, "t3_p3_v4": 3}[name]
    assert kinds == [want, want], (name, kinds)


@gpu
def test_zero_rows_launch_nothing(lib, tuned):
    """rows == 0 returns 0 and writes nothing."""
    case = CASE_BY_NAME["t1_p2_v4"]
    tuned(case.tune)
    P = build_problem(case, 1, "int")
    dev = Dev(P)
    for n, shape in (("out", (1, 4, case.dout)), ("z1", (1, 4, case.hid)), ("xhat", (1, 4, case.dout)), ("rstd", (1, 4)), ("dz1", (4, case.hid)),
                     ("dz2", (4, case.dout)), ("dsrc0", (1, 4, case.widths[0])), ("dsrc1", (1, 4, case.widths[1])), ("dsrc2", (1, 4, case.widths[2])), ("vec", (4, 4, 256)),
                     ("wpack", (1 << 16,))):
        dev.out(n, shape)
    pf, pb = describe_both(lib, P, dev.addr)
    pf.wpack = pb.wpack = dev.addr("wpack")
    pf.rows = pf.ntiles = pb.rows = pb.ntiles = 0
    pb.vec_partials, pb.vec_partials_rows, pb.vec_stride = dev.addr("vec"), 4, 256
    assert lib.nlam_mlp_bwd_blocks(C.byref(pb)) <= 4
    assert lib.nlam_mlp_fwd_wide_plan(C.byref(pf)) == L.MLPW_EMPTY and lib.nlam_mlp_fwd(C.byref(pf), _stream()) == 0
    assert lib.nlam_mlp_bwd_wide_plan(C.byref(pb)) == L.MLPW_EMPTY and lib.nlam_mlp_bwd(C.byref(pb), _stream()) == 0
    torch.cuda.synchronize()
    for n, (buf, _, _) in dev.outs.items():
        assert bool(torch.isnan(buf).all()), f"{n} was written by a launch without rows"


# ---------------------------------------------------------------------------------------------------------------------------
# grouped launches of the fp32 wide family
# ---------------------------------------------------------------------------------------------------------------------------
def _member(name, code_f, code_b, widths, hid, dout, **kw):
    return Case(name, code_f, code_b, widths, hid, dout, tune=((CUS, 16),), **kw)


_G41 = dict(hid=96, dout=128, code_f=F32(4, 1), code_b=F32(4, 1))
_G82 = dict(hid=300, dout=260, code_f=F32(8, 2), code_b=F32(8, 2))
_TILE_LIST = dict(aggregate=True, out_perm=True, g_aggr=True, dmode=(1, 2, 3))
GROUPS = {   # members of one kernel shape (hid, dout, flags, LayerNorm or not) with different source counts, widths and tile counts
    # dense members: one row; more tiles than workgroups; three sources, a batch of 3
    "dense_41": [_member("m0", widths=(128, 68), rows=1, dmode=(2, 2), **_G41),
                 _member("m1", widths=(40,), rows=32 * 70 + 7, dmode=(1,), perm=(0,), out_perm=True, **_G41),
                 _member("m2", widths=(8, 100, 12), rows=65, batch=3, dmode=(2, 1, 2), gather=(0,), broadcast=(2,), **_G41)],
    # tile lists without split tiles: aggr, out through out_idx, g_aggr, dmode 1, 2 and 3, NLAM_F_ADD_SRC0 -- the group kernels'
    # member-relative tile and receiver indexing and their aggregation; tiles below 32 rows, empty receivers
    "tile_list_41": [_member("m0", widths=(128, 68, 128), graph="mixed", add0=True, **_TILE_LIST, **_G41),
                     _member("m1", widths=(128, 8, 72), graph="mixed12", batch=2, add0=True, broadcast=(1,), **_TILE_LIST, **_G41),
                     _member("m2", widths=(128, 128, 128), graph="mixed", batch=3, add0=True, **_TILE_LIST, **_G41)],
    # the <8, 2> shape: a tile-list member with NLAM_F_ADD_SRC1 and a mean aggregate beside a larger one
    "tile_list_82": [_member("m0", widths=(132, 260, 260), graph="mixed12", add1=True, mean=True, **_TILE_LIST, **_G82),
                     _member("m1", widths=(8, 260, 300), graph="mixed", batch=2, add1=True, mean=True, **_TILE_LIST, **_G82)],
    "dense_81": [_member("m0", widths=(132,), hid=200, dout=132, code_f=F32(8, 1), code_b=F32(8, 1), rows=33, batch=2, ln=False, dmode=(2,)),
                 _member("m1", widths=(256, 8), hid=200, dout=132, code_f=F32(8, 1), code_b=F32(8, 1), rows=32 * 45 + 31, ln=False, dmode=(2, 2))],
}


@gpu
@pytest.mark.parametrize("group", list(GROUPS), ids=str)
def test_grouped_launch_equals_solo_launches(lib, tuned, group):
    """nlam_mlp_fwd_group / nlam_mlp_bwd_group on mlp_fwd_wide_group_kernel / mlp_bwd_wide_group_kernel: out, aggr, the saved tensors,
    dz1, dz2 and every dsrc (modes 1, 2 and 3) bit-equal to the members launched alone (no split tiles: every sum has a fixed
    order); each member's vec_partials rows (nlam_mlp_bwd_group_blocks of them, the rest of the buffer untouched), summed in
    float64, within the tier-(b) budget."""
    members = GROUPS[group]
    tuned(members[0].tune)
    n = len(members)
    Ps = [rand_problem(c, 20 + k) for k, c in enumerate(members)]
    assert not any(P.has_split or P.comb is not None for P in Ps)
    devs = [Dev(P) for P in Ps]
    solo_f = [run_forward(lib, P, dev) for P, dev in zip(Ps, devs)]
    keep = [_saved_dev(P.case, f) for P, f in zip(Ps, solo_f)]
    solo_b = [run_backward(lib, P, dev, kp) for P, dev, kp in zip(Ps, devs, keep)]
    fa = (L.MlpFwd * n)()
    for k in range(n):
        fa[k] = prep_forward(lib, Ps[k], devs[k])
        assert lib.nlam_mlp_fwd_family(C.byref(fa[k])) == 1
    assert lib.nlam_mlp_fwd_group(fa, n, _stream()) == 0
    for k in range(n):
        got = collect_forward(lib, Ps[k], devs[k])
        assert _same(got, solo_f[k]) == [], f"forward member {k}"
    ba = (L.MlpBwd * n)()
    nblk = [0] * n
    for k in range(n):
        ba[k], nblk[k] = prep_backward(lib, Ps[k], devs[k], keep[k])
    blocks = (C.c_int32 * n)()
    assert lib.nlam_mlp_bwd_group_blocks(ba, n, blocks) == 0
    tiles = [P.ntiles * P.batch for P in Ps]
    # the members are checked as single launches would be: room for nlam_mlp_bwd_blocks rows, blocks[k] of them written
    assert all(1 <= blocks[k] <= min(tiles[k], nblk[k]) for k in range(n)), (list(blocks), tiles, nblk)
    assert any(blocks[k] < tiles[k] for k in range(n)), "one member must have more tiles than workgroups"
    assert lib.nlam_mlp_bwd_group(ba, n, _stream()) == 0
    for k in range(n):
        P = Ps[k]
        got = collect_backward(lib, P, devs[k], int(blocks[k]), P.case.dout)
        exact = [m for m in got if torch.is_tensor(got[m]) and got[m].dim() == 3]
        assert {"dz1", "dz2"} <= set(exact)
        assert [m for m in exact if not torch.equal(got[m], solo_b[k][m])] == [], f"backward member {k}"
        ref, bud = backward_math(P, {m: solo_f[k][m].double() for m in keep[k]}, nblk=int(blocks[k]))
        vecs = [m for m in ("db1", "db2", "dgamma", "dbeta") if m in got]
        assert compare_bounded(got, ref, bud, names=vecs) == [], f"vec_partials of member {k}"
