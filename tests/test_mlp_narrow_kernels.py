"""Kernel-level checks of the narrow fused-MLP family (hid, dout and every source width <= 64: nlam_mlp_fwd_family == 0) through the
C ABI, against float64 math written straight from the contract of include/nlam_hip.h:
mlp_fwd_kernel, mlp_fwd_bf_kernel (RAG / RES / PRE / CAT instantiations), mlp_bwd_kernel, mlp_bwd_fast_kernel, the grouped forms
mlp_fwd_bf_group_kernel / mlp_bwd_fast_group_kernel and the pre-packed weight images of nlam_mlp_pack.

Every case names the instantiation (nlam_mlp_fwd_plan / nlam_mlp_bwd_plan) it is meant to run and asserts both codes before it
launches, so a case cannot quietly test another kernel.  Forward and backward run together: the backward consumes the z1, xhat and
rstd the forward kernel saved (the real contract) and, separately, the float64 reference's saved tensors rounded to fp32, so that
a forward bug cannot hide a backward bug or the reverse.  Every output buffer is NaN-filled and has NaN guard rows behind it.
  (a) exact arithmetic: small-integer operands (|v| <= 4) are exact in bf16 and their products and sums are exact in fp32 at
      these sizes, so z1 must equal the float64 result bit for bit in every matrix mode; without activation and LayerNorm the
      whole chain must (out, aggr, dz2, dz1, every dsrc mode, db1 / db2), with SiLU dz2 and db2 must;
  (b) precision: random operands with a different scale per column, |got - R| <= bound element by element, the bound a
      first-order error budget propagated in float64 next to the reference (forward_math / backward_math);
  (c) low-order probe: operands whose third bf16 term is as large as it can be and of one sign -- a three-term GEMM1 that
      drops its low-order term misses the tier-(b) bound of z1 there (on random operands it would not).
The comparison functions are themselves tested without a GPU: a stand-in kernel (the same MLP in torch fp32 on the CPU) passes,
and each of eight injected defects is reported by name."""
import ctypes as C
import json
import os
import time
from dataclasses import replace

import pytest
import torch

from neural_lam_amd import _lib as L

# the case record, the problem builder, the float64 math with its budget, the comparisons and the device helper: shared with
# test_mlp_wide_kernels.py
from mlp_kernel_ref import (GRID_WAVES, SPLIT_SAFETY, Case, Dev, _combine, _same, _saved_dev, _stream, _written, backward_math,  # noqa: F401
                            block_vectors, build_problem, compare_bounded, compare_exact, describe_bwd, describe_fwd, dsrc_rows,
                            exact_quantities, forward_math)

gpu = pytest.mark.gpu

_RATIOS = {}    # ("fwd" | "bwd", plan code) -> {quantity: largest |got - R| / bound over the tier-(b) runs}


def _note_ratio(which, code, name, ratio):
    d = _RATIOS.setdefault((which, int(code)), {})
    d[name] = max(d.get(name, 0.0), float(ratio))


def plan_name(which, code):
    k, hb, ob, ns, bits = L.mlpp_fields(code)
    kern = ({1: "mlp_fwd_kernel generic", 2: "mlp_fwd_kernel fast", 3: "mlp_fwd_bf_kernel"} if which == "fwd"
            else {1: "mlp_bwd_kernel", 2: "mlp_bwd_fast_kernel"})[k]
    tags = [t for b, t in ((L.MLPP_RAG, "RAG" if which == "fwd" else "RO"), (L.MLPP_RES, "RES"), (L.MLPP_PRE, "PRE"), (L.MLPP_CAT, "CAT")) if bits & b]
    return f"{kern} HB{hb} OB{ob} NS{ns}" + ("".join(" " + t for t in tags))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib = L.load()
    t0 = time.time()
    yield lib
    path = os.environ.get("NLAM_MLP_NARROW_REPORT")
    if path and _RATIOS:
        rep = {"wall_seconds": round(time.time() - t0, 2), "split_safety": SPLIT_SAFETY,
               "ratios": [{"which": w, "code": c, "plan": plan_name(w, c), "max_ratio": v} for (w, c), v in sorted(_RATIOS.items())]}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
FG, FF, FB = L.MLPP_FWD_GENERIC, L.MLPP_FWD_FAST, L.MLPP_FWD_BF
BG, BF_ = L.MLPP_BWD_GENERIC, L.MLPP_BWD_FAST
RAG, RES, PRE, CAT = L.MLPP_RAG, L.MLPP_RES, L.MLPP_PRE, L.MLPP_CAT
P_ = L.mlpp_code
ROWS = (1, 31, 32, 33, 65)
BIG_ROWS = 32 * (GRID_WAVES + 37) + 5   # more tiles than waves: every wave walks at least two tiles, the next-tile prefetch runs

CASES = [
    # ---- mlp_fwd_kernel generic: hid or dout no multiple of 32, 2-3 sources of ragged widths; a requested split mode falls back to fp32
    Case("gen_7_12_5", P_(FG, 1, 1, 0), P_(BG, 1, 1, 0), (7, 12, 5), 24, 17, rows=33, gather=(1,), dmode=(1, 2, 1)),
    Case("gen_7_12_5_mm3_fallback", P_(FG, 2, 2, 0), P_(BG, 2, 2, 0), (7, 12, 5), 40, 33, rows=65, batch=3, mm=3, broadcast=(2,),
         perm=(0,), dmode=(1, 0, 1)),
    Case("gen_24_24_17", P_(FG, 1, 1, 0), P_(BG, 1, 1, 0), (24, 24, 17), 32, 32, rows=31, ln=False, gather=(0, 2), dmode=(2, 1, 0)),
    Case("gen_noact_exact", P_(FG, 1, 2, 0), P_(BG, 1, 2, 0), (12, 20), 24, 40, rows=65, batch=3, ln=False, no_act=True, gather=(1,),
         dmode=(1, 2), out_perm=True),
    # ---- mlp_fwd_kernel fast (fp32 MFMA, widths % 8, whole 32-column blocks)
    Case("fast_64_32_add1", P_(FF, 2, 1, 0), P_(BF_, 2, 1, 0), (64, 32), 64, 32, rows=65, add1=True),
    Case("fast_8_16", P_(FF, 1, 2, 0), P_(BG, 1, 2, 0), (8, 16), 32, 64, rows=32, batch=3, broadcast=(0,), dmode=(1, 1)),
    Case("fast_noact_exact", P_(FF, 2, 2, 0), P_(BG, 2, 2, 0), (64, 64, 64), 64, 64, rows=33, ln=False, no_act=True, add0=True,
         gather=(1, 2), perm=(0,), dmode=(1, 2, 2), out_perm=True),
    Case("fast_noact_ln", P_(FF, 1, 1, 0), P_(BG, 1, 1, 0), (32,), 32, 32, rows=1, no_act=True),
    # ---- mlp_fwd_bf_kernel, NS = 1, 2, 3 for (HB, OB) in {1, 2}^2; the backward on mlp_bwd_fast_kernel in the same mode
    *[Case(f"bf_ns{ns}_hb{hb}_ob{ob}", P_(FB, hb, ob, ns), P_(BF_, hb, ob, ns), (32, 64) if (hb + ob) % 2 else (64,), 32 * hb, 32 * ob,
           rows=ROWS[(2 * hb + ob + ns) % 5], batch=1 + 2 * (ns == 2), mm=ns, ln=(hb + ns) % 2 == 0,
           gather=(0,) if ns == 3 else (), dmode=(2, 1) if ns == 3 else (1, 1))
      for ns in (1, 2, 3) for hb in (1, 2) for ob in (1, 2)],
    Case("fast_f32_h32", P_(FF, 1, 1, 0), P_(BF_, 1, 1, 0), (32,), 32, 32, rows=33, batch=3),
    Case("fast_f32_h32_o64", P_(FF, 1, 2, 0), P_(BF_, 1, 2, 0), (64,), 32, 64, rows=31, ln=False, perm=(0,)),
    # ---- RAG: a single source of width 3, 20 or 56 (the embedders: no data gradient; with one, the generic backward)
    *[Case(f"rag_ns{ns}_hb{hb}_ob{ob}", P_(FB, hb, ob, ns, RAG), P_(BF_, hb, ob, ns), ((3, 20, 56)[(ns + hb + ob) % 3],), 32 * hb, 32 * ob,
           rows=ROWS[(hb + 2 * ob + ns) % 5], batch=1 + 2 * (ns == 1), mm=ns, ln=(ob + ns) % 2 == 0, broadcast=(0,) if hb == ob else (),
           dmode=(0,))
      for ns in (1, 2, 3) for hb in (1, 2) for ob in (1, 2)],
    Case("rag_w56_dx", P_(FB, 2, 1, 1, RAG), P_(BG, 2, 1, 0), (56,), 64, 32, rows=31, mm=1, gather=(0,), dmode=(2,)),
    # ---- ragged output width (output_map): no LayerNorm, dz2 32-padded with zero columns
    *[Case(f"rout_ns{ns}_hb{hb}", P_(FB, hb, 1, ns, RAG), P_(BF_, hb, 1, ns, RAG), (32 * hb,), 32 * hb, (5, 17, 31)[(ns + hb) % 3],
           rows=ROWS[(ns + 3 * hb) % 5], batch=1 + 2 * (ns == 2), mm=ns, ln=False, dmode=((ns + hb) % 2,))
      for ns in (1, 2, 3) for hb in (1, 2)],
    Case("rout_17_f32", P_(FG, 2, 1, 0), P_(BG, 2, 1, 0), (64,), 64, 17, rows=33, ln=False),
    # ---- RES: NLAM_F_ADD_SRC0, NLAM_F_ADD_SRC1, both
    *[Case(f"res_ns{ns}_hb{hb}_ob{ob}", P_(FB, hb, ob, ns, RES), P_(BF_, hb, ob, ns),
           ((32 * ob, 32), (32, 32 * ob), (32 * ob, 32 * ob))[(ns + hb + ob) % 3], 32 * hb, 32 * ob,
           rows=ROWS[(3 * hb + ob + ns) % 5], batch=1 + 2 * (ns == 3), mm=ns, ln=(hb + ob + ns) % 2 == 1,
           add0=(ns + hb + ob) % 3 != 1, add1=(ns + hb + ob) % 3 != 0, broadcast=(1,) if ns == 3 else ())
      for ns in (1, 2, 3) for hb in (1, 2) for ob in (1, 2)],
    Case("res_add01_gather", P_(FB, 2, 2, 1, RES), P_(BF_, 2, 2, 1), (64, 64, 32), 64, 64, rows=31, mm=1, add0=True, add1=True, ln=False,
         gather=(2,), dmode=(1, 1, 2)),
    # ---- PRE without a tile schedule: src0 through GEMM1, gathered addends of width hid, ldw1 larger than src0's width
    *[Case(f"pre_ns{ns}_hb{hb}_res{res}", P_(FB, hb, hb, ns, PRE | (RES if res else 0)), P_(BF_, hb, hb, ns), (32 * hb,) * (1 + hb), 32 * hb, 32 * hb,
           rows=ROWS[(hb + ns + res) % 5], batch=1 + 2 * (ns == 2), mm=ns, pre=True, ldw1_extra=32 * hb * hb, add0=bool(res),
           ln=(ns + res) % 2 == 0, gather=(1, 2)[:hb], dmode=(1, 0, 0)[: 1 + hb])
      for ns in (1, 2, 3) for hb in (1, 2) for res in (0, 1)],
    # ---- CAT: 2 and 4 pieces, a piece shared by the batch, cat_out written
    *[Case(f"cat_ns{ns}_hb{hb}", P_(FB, hb, hb, ns, RAG | CAT), P_(BF_, hb, hb, ns), ((32,), (56,))[hb - 1], 32 * hb, 32 * hb,
           rows=ROWS[(ns + hb) % 5 or 1], batch=3, mm=ns, cat=((12, 20), (8, 8, 24, 16))[hb - 1], cat_shared=((1,), (3,))[hb - 1],
           ln=ns != 2, dmode=(0,))
      for ns in (1, 2, 3) for hb in (1, 2)],
    Case("cat4_h64_dx", P_(FB, 2, 2, 1, RAG | CAT), P_(BG, 2, 2, 0), (56,), 64, 64, rows=33, batch=3, mm=1, cat=(8, 8, 24, 16), cat_shared=(3,), dmode=(1,)),
    # ---- more tiles than waves (batch 1 and 3): the default benchmark line's node MLP shape
    Case("big_b1", P_(FB, 2, 2, 3, RES), P_(BF_, 2, 2, 3), (64, 64), 64, 64, rows=BIG_ROWS, mm=3, add0=True),
    Case("big_b3", P_(FB, 1, 1, 3), P_(BF_, 1, 1, 3), (32,), 32, 32, rows=BIG_ROWS, batch=3, mm=3),
    # ---- edge geometry over a tile schedule: three gathered sources, out through the CSR permutation and aggr together
    Case("edge_mixed_add0", P_(FB, 2, 2, 3, RES), P_(BF_, 2, 2, 3), (64, 64, 64), 64, 64, batch=3, mm=3, graph="mixed", add0=True,
         aggregate=True, out_perm=True, dmode=(1, 2, 3), g_aggr=True, broadcast=(1,)),
    Case("edge_split_mean_add1", P_(FB, 1, 1, 2, RES), P_(BF_, 1, 1, 2), (32, 32, 32), 32, 32, mm=2, graph="split", add1=True, mean=True,
         want_out=False, aggregate=True, dmode=(1, 2, 3), g_out=False, g_aggr=True),
    Case("edge_split_atomic_exact", P_(FF, 1, 1, 0), P_(BG, 1, 1, 0), (32, 32, 32), 32, 32, batch=3, graph="split", atomic=True, ln=False,
         no_act=True, aggregate=True, out_perm=True, dmode=(1, 2, 3), g_aggr=True),
    Case("edge_split_virtual_exact", P_(FF, 1, 1, 0), P_(BG, 1, 1, 0), (32, 32, 32), 32, 32, graph="split", ln=False, no_act=True,
         aggregate=True, out_perm=True, dmode=(1, 0, 3), g_aggr=True),
    Case("edge_mixed_generic", P_(FG, 1, 1, 0), P_(BG, 1, 1, 0), (12, 20, 8), 24, 17, graph="mixed", aggregate=True, out_perm=True,
         dmode=(1, 0, 3), g_aggr=True),
    Case("edge_mixed_mean_f32", P_(FF, 2, 2, 0), P_(BF_, 2, 2, 0), (64, 64, 64), 64, 64, graph="mixed", mean=True, aggregate=True,
         want_out=False, dmode=(0, 2, 3), g_out=False, g_aggr=True),
    Case("edge_mixed_silu_sum", P_(FB, 1, 2, 3), P_(BF_, 1, 2, 3), (32, 32, 64), 32, 64, graph="mixed", mm=3, ln=False, aggregate=True,
         out_perm=True, dmode=(1, 2, 3), g_aggr=True),
    # ---- PRE over a tile schedule: the receiver-gathered addend's gradient is segment-summed in the kernel (dmode 3)
    Case("edge_pre3_split", P_(FB, 2, 2, 3, PRE | RES), P_(BF_, 2, 2, 3), (64, 64, 64), 64, 64, mm=3, graph="split", pre=True, ldw1_extra=128,
         add0=True, aggregate=True, out_perm=True, dmode=(1, 0, 3), g_aggr=True),
    Case("edge_pre2_mixed", P_(FB, 1, 1, 1, PRE), P_(BF_, 1, 1, 1), (32, 32), 32, 32, batch=3, mm=1, graph="mixed", roles="er", pre=True,
         ldw1_extra=64, aggregate=True, want_out=False, dmode=(1, 3), g_out=False, g_aggr=True),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# the checker's own test: a CPU stand-in for the kernel, and eight injected defects (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------
STANDIN_CASE = Case("standin", 0, 0, (32, 32, 32), 32, 32, graph="mixed", add0=True, aggregate=True, out_perm=True, dmode=(1, 2, 3),
                    g_aggr=True)
STANDIN_NBLK = 4
DEFECTS = ["drop_input_column", "swap_gather_indices", "omit_residual", "tile_last_row_not_aggregated", "rstd_without_eps",
           "sigmoid_for_silu_derivative", "skip_vec_partials_block", "drop_third_term"]


def standin_run(case, kind, defect=None, ns_claimed=0):
    """The MLP in torch fp32 on the CPU with an optional defect, compared like a kernel -> names of the failing quantities."""
    P = build_problem(case, 7, kind)
    ref_f, bud_f = forward_math(P, ns=ns_claimed)
    got_f, _ = forward_math(P, torch.float32, defect=defect)
    saved = {k: got_f[k] for k in ("z1", "xhat", "rstd") if k in got_f}
    ref_b, bud_b = backward_math(P, saved, ns=ns_claimed, nblk=STANDIN_NBLK)
    got_b, _ = backward_math(P, saved, torch.float32, defect=defect)
    # the four vectors as a kernel leaves them: per-workgroup partial sums, summed in float64
    c = case
    go = P.g_out[:, P.out_idx] if P.out_idx is not None else P.g_out
    dm = (go + (P.g_aggr * P.scale[None, :, None])[:, P.seg_of_row]).float()
    rows = {"db1": got_b["dz1"], "db2": got_b["dz2"]}
    if c.ln:
        rows.update(dgamma=dm * saved["xhat"], dbeta=dm)
    got_b.update(block_vectors(P, rows, STANDIN_NBLK, skip=1 if defect == "skip_vec_partials_block" else None))
    if kind == "int":
        return compare_exact(got_f, ref_f, exact_quantities(c, True)) + compare_exact(got_b, ref_b, exact_quantities(c, False))
    return compare_bounded(got_f, ref_f, bud_f) + compare_bounded(got_b, ref_b, bud_b)


def test_standin_passes_with_the_fp32_constants():
    for case in (STANDIN_CASE, replace(STANDIN_CASE, ln=False, no_act=True), replace(STANDIN_CASE, ln=False),
                 replace(STANDIN_CASE, mean=True, add0=False, add1=True)):
        assert standin_run(case, "int") == [], case
        assert standin_run(case, "rand") == [], case
    assert standin_run(replace(STANDIN_CASE, name="probe"), "probe", ns_claimed=3) == []


@pytest.mark.parametrize("defect", DEFECTS)
def test_injected_defect_is_reported(defect):
    """Each defect must fail the comparison, in the quantity it corrupts first."""
    first = {"drop_input_column": "z1", "swap_gather_indices": "z1", "omit_residual": "out", "tile_last_row_not_aggregated": "aggr",
             "rstd_without_eps": "rstd", "sigmoid_for_silu_derivative": "dz1", "skip_vec_partials_block": "db1", "drop_third_term": "z1"}[defect]
    if defect == "drop_third_term":
        # the stand-in claims the three-term bound (2^-24 class) but rounds one GEMM1 operand to bf16 + bf16
        assert first in standin_run(STANDIN_CASE, "probe", defect, ns_claimed=3), defect
        return
    if defect == "rstd_without_eps":   # rows of nearly equal outputs: eps is then a visible part of the variance
        case = replace(STANDIN_CASE, name="tiny_variance")
        bad = _standin_tiny_variance(case, defect)
        assert first in bad, (defect, bad)
        return
    bad_b = standin_run(STANDIN_CASE, "rand", defect)
    assert first in bad_b, (defect, bad_b)
    if defect in ("drop_input_column", "swap_gather_indices"):
        assert "z1" in standin_run(STANDIN_CASE, "int", defect), defect
    if defect in ("omit_residual", "tile_last_row_not_aggregated", "skip_vec_partials_block"):
        exact = replace(STANDIN_CASE, ln=False, no_act=True)
        bad_a = standin_run(exact, "int", defect)
        assert first in bad_a, (defect, bad_a)


def _standin_tiny_variance(case, defect):
    P = build_problem(case, 7, "rand")
    P.W2 = (P.W2 * 2.0 ** -9).float().double()   # outputs of ~1e-3: a variance of ~1e-6 next to eps = 1e-5
    P.b2 = (P.b2 * 2.0 ** -9).float().double()
    ref_f, bud_f = forward_math(P)
    got_f, _ = forward_math(P, torch.float32, defect=defect)
    return compare_bounded(got_f, ref_f, bud_f)


def test_tiny_variance_standin_passes():
    assert _standin_tiny_variance(replace(STANDIN_CASE, name="tiny_variance"), None) == []


def test_case_table_plans():
    """Host logic only: every case hits the instantiation it names; wide and empty launches are told apart; the fallbacks."""
    lib = L.load()
    for c in CASES:
        P = build_problem(replace(c, rows=min(c.rows, 65)) if not c.graph else c, 1, "int")
        pf = describe_fwd(P, lambda n: None if (n.startswith("idx") and P.srcs[int(n[3:])].idx is None)
                          or (n == "tiles" and P.tiles is None) or (n == "out_idx" and P.out_idx is None) else 4096)
        pb = describe_bwd(P, lambda n: None if (n.startswith("idx") and P.srcs[int(n[3:])].idx is None)
                          or (n == "tiles" and P.tiles is None) or (n == "out_idx" and P.out_idx is None) else 4096, lib)
        assert lib.nlam_mlp_fwd_family(C.byref(pf)) == 0 and lib.nlam_mlp_bwd_family(C.byref(pb)) == 0, c.name
        got_f, got_b = lib.nlam_mlp_fwd_plan(C.byref(pf)), lib.nlam_mlp_bwd_plan(C.byref(pb))
        assert got_f == c.fwd, (c.name, plan_name("fwd", got_f) if got_f > 0 else got_f, plan_name("fwd", c.fwd))
        assert got_b == c.bwd, (c.name, plan_name("bwd", got_b) if got_b > 0 else got_b, plan_name("bwd", c.bwd))
        ro = bool(c.bwd & RAG)
        assert pb.dz2_ld == (32 if ro else 0), c.name
    # rows == 0: nothing is launched; a width above 64: not narrow; what the launch refuses, the query refuses the same way
    P = build_problem(CASE_BY_NAME["bf_ns3_hb2_ob2"], 1, "int")
    a = lambda n: None if n in ("tiles", "out_idx") or (n.startswith("idx") and P.srcs[int(n[3:])].idx is None) else 4096
    pf, pb = describe_fwd(P, a), describe_bwd(P, a, lib)
    pf.rows = pb.rows = 0
    assert lib.nlam_mlp_fwd_plan(C.byref(pf)) == L.MLPP_EMPTY and lib.nlam_mlp_bwd_plan(C.byref(pb)) == L.MLPP_EMPTY
    pf, pb = describe_fwd(P, a), describe_bwd(P, a, lib)
    pf.hid = pb.hid = 128
    pf.wpack = pb.wpack = 4096
    pf.wpack_floats = pb.wpack_floats = 1 << 30
    assert lib.nlam_mlp_fwd_family(C.byref(pf)) != 0
    assert lib.nlam_mlp_fwd_plan(C.byref(pf)) == L.MLPP_NOT_NARROW and lib.nlam_mlp_bwd_plan(C.byref(pb)) == L.MLPP_NOT_NARROW
    pf, pb = describe_fwd(P, a), describe_bwd(P, a, lib)
    pf.W1 = pb.W1 = None
    assert lib.nlam_mlp_fwd_plan(C.byref(pf)) == -1 and lib.nlam_mlp_bwd_plan(C.byref(pb)) == -1
    pf, pb = describe_fwd(P, a), describe_bwd(P, a, lib)
    pf.flags |= L.F_NO_ACT
    pb.flags |= L.F_ACC_DSRC0
    assert lib.nlam_mlp_fwd_plan(C.byref(pf)) == -2 and lib.nlam_mlp_bwd_plan(C.byref(pb)) == -2
    pb = describe_bwd(P, a, lib)
    pb.dz2_ld = 32   # not what nlam_mlp_bwd_dz2_ld gives for this shape
    assert lib.nlam_mlp_bwd_plan(C.byref(pb)) == -1
    # concatenated pieces and the factorised form have no fp32 instantiation
    Pc = build_problem(replace(CASE_BY_NAME["cat_ns3_hb1"], mm=0), 1, "int")
    ac = lambda n: None if n in ("tiles", "out_idx", "idx0") else 4096
    assert lib.nlam_mlp_fwd_plan(C.byref(describe_fwd(Pc, ac))) == -2
    Pp = build_problem(replace(CASE_BY_NAME["pre_ns3_hb1_res0"], mm=0), 1, "int")
    ap = lambda n: None if n in ("tiles", "out_idx", "idx0") else 4096
    assert lib.nlam_mlp_fwd_plan(C.byref(describe_fwd(Pp, ap))) == -2
    assert lib.nlam_mlp_bwd_plan(C.byref(describe_bwd(Pp, ap, lib))) == -2


def test_every_reachable_plan_has_a_case():
    """The instantiations fwd_narrow / bwd_narrow can launch, listed from their dispatch (the launcher's pick<> ladders), against
    the case table: every reachable code has a case, and no case names a code the dispatch cannot produce."""
    fwd = {P_(k, hb, ob, 0) for k in (FG, FF) for hb in (1, 2) for ob in (1, 2)}                 # mlp_fwd_kernel<hb, ob, fast, 0>
    fwd |= {P_(FB, hb, ob, ns, bits) for hb in (1, 2) for ob in (1, 2) for ns in (1, 2, 3) for bits in (0, RAG, RES)}
    fwd |= {P_(FB, hb, hb, ns, RAG | CAT) for hb in (1, 2) for ns in (1, 2, 3)}                  # <hb, hb, ns, true, false, false, true>
    fwd |= {P_(FB, hb, hb, ns, PRE | res) for hb in (1, 2) for ns in (1, 2, 3) for res in (0, RES)}   # <hb, hb, ns, false, res, true>
    bwd = {P_(BG, hb, ob, 0) for hb in (1, 2) for ob in (1, 2)}                                   # mlp_bwd_kernel<hb, ob>
    bwd |= {P_(BF_, hb, ob, ns) for hb in (1, 2) for ob in (1, 2) for ns in (0, 1, 2, 3)}        # mlp_bwd_fast_kernel<hb, ob, ns>
    bwd |= {P_(BF_, hb, 1, ns, RAG) for hb in (1, 2) for ns in (1, 2, 3)}                        # <hb, 1, ns, true>
    hit_f, hit_b = {c.fwd for c in CASES}, {c.bwd for c in CASES}
    assert hit_f <= fwd and hit_b <= bwd, "a case names a code the dispatch cannot produce"
    assert not (fwd - hit_f), sorted(plan_name("fwd", x) for x in fwd - hit_f)
    assert not (bwd - hit_b), sorted(plan_name("bwd", x) for x in bwd - hit_b)


def run_forward(lib, P, dev, wpack=None):
    """One nlam_mlp_fwd launch into fresh outputs -> host tensors (aggr: the real receivers' rows, after nlam_split_combine)."""
    c = P.case
    dev.outs = {}
    if c.want_out:
        dev.out("out", (P.batch, P.out_rows, c.dout))
    if c.aggregate:
        dev.out("aggr", (P.batch, P.nseg_rows, c.dout), zero=P.has_split)
    dev.out("z1", (P.batch, P.rows, c.hid))
    if c.ln:
        dev.out("xhat", (P.batch, P.rows, c.dout))
        dev.out("rstd", (P.batch, P.rows))
    if c.cat:
        dev.out("cat_out", (P.batch, P.rows, c.widths[0]))
    p = describe_fwd(P, dev.addr)
    if wpack is not None:
        p.wpack, p.wpack_floats = wpack.data_ptr(), wpack.numel()
    got = lib.nlam_mlp_fwd_plan(C.byref(p))
    assert got == c.fwd, (c.name, got, plan_name("fwd", c.fwd))
    assert lib.nlam_mlp_fwd_family(C.byref(p)) == 0
    assert lib.nlam_mlp_fwd(C.byref(p), _stream()) == 0, c.name
    if c.aggregate and P.comb is not None:
        _combine(lib, dev, dev.t["aggr"], c.dout)
    torch.cuda.synchronize()
    assert dev.guards_intact() == [], f"{c.name}: forward wrote behind an output"
    res = {n: dev.t[n].cpu() for n in dev.outs}
    if c.aggregate:
        res["aggr"] = res["aggr"][:, : P.nseg]
    return res


def run_backward(lib, P, dev, saved, wpack=None):
    """One nlam_mlp_bwd launch on the saved tensors `saved` (device) -> host tensors + the four vectors summed in float64."""
    c = P.case
    dev.outs = {}
    for n in ("z1", "xhat", "rstd"):
        if n in saved:
            dev.t[n] = saved[n]
    p = describe_bwd(P, dev.addr, lib)   # placeholder outputs: what decides the kernel is set
    ld = p.dz2_ld if p.dz2_ld else c.dout
    dev.out("dz1", (P.batch * P.rows, c.hid))
    dev.out("dz2", (P.batch * P.rows, ld))
    for k in range(P.nsrc):
        if c.dmode[k] != 0:
            dev.out(f"dsrc{k}", (P.batch, dsrc_rows(P, k), c.widths[k]), zero=c.dmode[k] == 3 and P.has_split)
    p = describe_bwd(P, dev.addr, lib)
    nblk = lib.nlam_mlp_bwd_blocks(C.byref(p))
    assert nblk == lib.nlam_num_blocks(P.ntiles * P.batch)
    vec = dev.out("vec", (nblk, 4, 64))
    p.vec_partials, p.vec_partials_rows, p.vec_stride = vec.data_ptr(), nblk, 64
    if wpack is not None:
        p.wpack, p.wpack_floats = wpack.data_ptr(), wpack.numel()
    got = lib.nlam_mlp_bwd_plan(C.byref(p))
    assert got == c.bwd, (c.name, got, plan_name("bwd", c.bwd))
    assert (p.dz2_ld == 32) == bool(c.bwd & RAG)
    assert lib.nlam_mlp_bwd(C.byref(p), _stream()) == 0, c.name
    for k in range(P.nsrc):
        if c.dmode[k] == 3 and P.comb is not None:
            _combine(lib, dev, dev.t[f"dsrc{k}"], c.widths[k])
    torch.cuda.synchronize()
    assert dev.guards_intact() == [], f"{c.name}: backward wrote behind an output"
    res = {n: dev.t[n].cpu() for n in dev.outs}
    res["dz1"] = res["dz1"].reshape(P.batch, P.rows, c.hid)
    dz2 = res["dz2"].reshape(P.batch, P.rows, ld)
    if ld != c.dout:
        assert torch.count_nonzero(dz2[..., c.dout:]) == 0 and torch.isfinite(dz2).all(), f"{c.name}: the padding columns of dz2 must be written as zeros"
    res["dz2"] = dz2[..., : c.dout].contiguous()
    for k in range(P.nsrc):
        if c.dmode[k] == 3:
            res[f"dsrc{k}"] = res[f"dsrc{k}"][:, : P.nseg]
    v = res.pop("vec").double()
    res["db1"], res["db2"] = v[:, 0, : c.hid].sum(0), v[:, 1, : c.dout].sum(0)
    if c.ln:
        res["dgamma"], res["dbeta"] = v[:, 2, : c.dout].sum(0), v[:, 3, : c.dout].sum(0)
    res["_vec"], res["_nblk"] = v, nblk
    return res


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_exact_on_integers(lib, case):
    """Tier (a): integer operands; z1 in every instantiation, and the whole chain where no rounding can occur, bit-equal to float64."""
    assert lib.nlam_grid_waves() == GRID_WAVES
    P = build_problem(case, 11, "int")
    dev = Dev(P)
    got_f = run_forward(lib, P, dev)
    _written(got_f, f"{case} forward")
    ref_f, _ = forward_math(P)
    assert compare_exact(got_f, ref_f, exact_quantities(case, True)) == [], f"{case}: forward is not the exact result"
    if case.cat:
        assert torch.equal(got_f["cat_out"].double(), P.srcs[0].S.expand(P.batch, -1, -1)), f"{case}: cat_out"
    got_b = run_backward(lib, P, dev, _saved_dev(got_f))
    _written(got_b, f"{case} backward")
    ref_b, _ = backward_math(P, {k: got_f[k].double() for k in ("z1", "xhat", "rstd") if k in got_f})
    assert compare_exact(got_b, ref_b, exact_quantities(case, False)) == [], f"{case}: backward is not the exact result"


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_elementwise_error_budget(lib, case):
    """Tier (b): every output, saved tensor, gradient and vector within its propagated budget; the stages behind GEMM1 also on
    their own (continued from the kernel's z1); the backward on the kernel's saved tensors and on the reference's; two launches of
    a non-atomic case are bit-equal."""
    P = build_problem(case, 12, "rand")
    dev = Dev(P)
    ns_f, ns_b = L.mlpp_fields(case.fwd)[3], L.mlpp_fields(case.bwd)[3]
    got_f = run_forward(lib, P, dev)
    _written(got_f, f"{case} forward")
    keep = _saved_dev(got_f)
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
    rounded = {k: ref_f[k].float() for k in keep}   # the reference's saved tensors, rounded to fp32
    got_r = run_backward(lib, P, dev, {k: v.cuda() for k, v in rounded.items()})
    ref_r, bud_r = backward_math(P, {k: v.double() for k, v in rounded.items()}, ns=ns_b, nblk=got_r["_nblk"])
    bad = compare_bounded(got_r, ref_r, bud_r, note=note_b)
    assert bad == [], f"{case}: backward (on the reference's saved tensors) over its budget in {bad}"


PROBE_CASES = [c for c in CASES if L.mlpp_fields(c.fwd)[3] == 3 and not c.graph and c.rows <= 65]


@gpu
@pytest.mark.parametrize("case", PROBE_CASES, ids=str)
def test_three_term_gemm1_keeps_its_low_order_term(lib, case):
    """Tier (c): every GEMM1 operand has a third bf16 term of 0.98 * 2^-17 of its value, all of one sign; z1 within the
    three-term budget means the term took part (test_injected_defect_is_reported[drop_third_term] shows the bound tells)."""
    P = build_problem(case, 13, "probe")
    got = run_forward(lib, P, Dev(P))
    ref, bud = forward_math(P, ns=3)
    assert compare_bounded(got, ref, bud, names=["z1"], note=lambda n, r: _note_ratio("fwd", case.fwd, "z1 (probe)", r)) == [], case


@gpu
def test_zero_rows_launch_nothing(lib):
    """rows == 0 returns 0 and writes nothing."""
    case = CASE_BY_NAME["bf_ns3_hb2_ob2"]
    P = build_problem(case, 1, "int")
    dev = Dev(P)
    for n, shape in (("out", (1, 4, 64)), ("z1", (1, 4, 64)), ("xhat", (1, 4, 64)), ("rstd", (1, 4)), ("dz1", (4, 64)), ("dz2", (4, 64)),
                     ("dsrc0", (1, 4, 64)), ("vec", (1, 4, 64))):
        dev.out(n, shape)
    pf = describe_fwd(P, dev.addr)
    pf.rows = pf.ntiles = 0
    assert lib.nlam_mlp_fwd_plan(C.byref(pf)) == L.MLPP_EMPTY and lib.nlam_mlp_fwd(C.byref(pf), _stream()) == 0
    pb = describe_bwd(P, dev.addr, lib)
    pb.rows = pb.ntiles = 0
    pb.vec_partials, pb.vec_partials_rows, pb.vec_stride = dev.addr("vec"), 1, 64
    assert lib.nlam_mlp_bwd_plan(C.byref(pb)) == L.MLPP_EMPTY and lib.nlam_mlp_bwd(C.byref(pb), _stream()) == 0
    torch.cuda.synchronize()
    for n, (buf, _, _) in dev.outs.items():
        assert bool(torch.isnan(buf).all()), f"{n} was written by a launch without rows"


# ---------------------------------------------------------------------------------------------------------------------------
# bit identity: pre-packed weight images, grouped launches
# ---------------------------------------------------------------------------------------------------------------------------
PACK_CASES = ["bf_ns1_hb2_ob1", "bf_ns2_hb1_ob2", "bf_ns3_hb2_ob2", "res_ns3_hb2_ob2", "pre_ns3_hb2_res1", "rag_ns2_hb1_ob1"]


@gpu
@pytest.mark.parametrize("name", PACK_CASES)
def test_packed_weight_image_is_bit_identical(lib, name):
    """A launch that fetches the nlam_mlp_pack image equals the launch that stages its weights itself, forward and backward."""
    case = CASE_BY_NAME[name]
    P = build_problem(case, 14, "rand")
    dev = Dev(P)
    job = L.PackJob()
    job.W1, job.W2, job.hid, job.dout, job.nsrc = dev.addr("W1"), dev.addr("W2"), case.hid, case.dout, P.nsrc
    job.ldw1 = P.ldw1 if case.pre else 0
    for k, w in enumerate(case.widths):
        job.width[k] = w
    job.flags = (case.mm << 8) | (L.F_PRE_ADD if case.pre else 0)
    nf, nb = lib.nlam_mlp_pack_floats(C.byref(job), 0), lib.nlam_mlp_pack_floats(C.byref(job), 1)
    assert nf > 0 and nb > 0 and nf % 256 == 0 and nb % 256 == 0, (nf, nb)   # whole 1 KiB LDS-DMA pieces
    fimg, bimg = dev.out("fwd_image", (nf,)), dev.out("bwd_image", (nb,))
    images = dict(dev.outs)
    job.fwd_image, job.bwd_image = fimg.data_ptr(), bimg.data_ptr()
    table = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).cuda()
    assert lib.nlam_mlp_pack(C.c_void_p(table.data_ptr()), 1, _stream()) == 0
    torch.cuda.synchronize()
    for n, (buf, k, _) in images.items():
        assert bool(torch.isfinite(buf[:k]).all()) and bool(torch.isnan(buf[k:]).all()), f"{name}: {n} is not exactly its announced size"
    plain_f = run_forward(lib, P, dev)
    keep = _saved_dev(plain_f)
    packed_f = run_forward(lib, P, dev, wpack=fimg)
    assert _same(plain_f, packed_f) == [], f"{name}: forward with the packed image differs"
    plain_b = run_backward(lib, P, dev, keep)
    packed_b = run_backward(lib, P, dev, keep, wpack=bimg)
    assert _same(plain_b, packed_b) == [], f"{name}: backward with the packed image differs"


GROUPS = [   # (hid = dout, mm, LayerNorm, (width, rows, batch) per member): a member of one row, one with more tiles than workgroups
    (64, 3, True, ((3, 1, 1), (20, 32 * 300 + 7, 1))),
    (32, 2, False, ((3, 1, 1), (20, 33, 3), (32, 65, 1), (64, 32 * 300 + 7, 1), (56, 100, 2), (2, 31, 1), (64, 32, 1), (8, 640, 1))),
]


@gpu
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"n{len(g[3])}_h{g[0]}_ns{g[1]}")
def test_grouped_launch_equals_solo_launches(lib, group):
    """nlam_mlp_fwd_group / nlam_mlp_bwd_group: outputs, saved tensors, dz1 and dz2 bit-equal to the members launched alone; each
    member's vec_partials rows (nlam_mlp_bwd_group_blocks of them), summed in float64, within the tier-(b) budget."""
    d, mm, ln, members = group
    n = len(members)
    Ps, devs, solo_f, solo_b = [], [], [], []
    for k, (w, rows, batch) in enumerate(members):
        rag = w % 32 != 0
        case = Case(f"member{k}", P_(FB, d // 32, d // 32, mm, RAG if rag else 0), P_(BF_, d // 32, d // 32, mm), (w,), d, d, rows=rows,
                    batch=batch, mm=mm, ln=ln, dmode=(0,))
        P = build_problem(case, 20 + k, "rand")
        dev = Dev(P)
        f = run_forward(lib, P, dev)
        solo_f.append(f)
        solo_b.append(run_backward(lib, P, dev, _saved_dev(f)))
        Ps.append(P)
        devs.append(dev)
    fa = (L.MlpFwd * n)()
    for k in range(n):
        P, dev, c = Ps[k], devs[k], Ps[k].case
        dev.outs = {}
        dev.out("out", (P.batch, P.rows, d))
        dev.out("z1", (P.batch, P.rows, d))
        if ln:
            dev.out("xhat", (P.batch, P.rows, d))
            dev.out("rstd", (P.batch, P.rows))
        fa[k] = describe_fwd(P, dev.addr)
    assert lib.nlam_mlp_fwd_group(fa, n, _stream()) == 0
    torch.cuda.synchronize()
    saved = []
    for k in range(n):
        assert devs[k].guards_intact() == []
        got = {m: devs[k].t[m].cpu() for m in devs[k].outs}
        assert _same(got, solo_f[k]) == [], f"forward member {k}"
        saved.append({m: devs[k].t[m] for m in ("z1", "xhat", "rstd") if m in devs[k].outs})
    ba = (L.MlpBwd * n)()
    for k in range(n):
        P, dev = Ps[k], devs[k]
        dev.outs = {}
        dev.t.update(saved[k])
        dev.out("dz1", (P.batch * P.rows, d))
        dev.out("dz2", (P.batch * P.rows, d))
        ba[k] = describe_bwd(P, dev.addr, lib)
    blocks = (C.c_int32 * n)()
    assert lib.nlam_mlp_bwd_group_blocks(ba, n, blocks) == 0
    tiles = [Ps[k].ntiles * Ps[k].batch for k in range(n)]
    assert all(1 <= blocks[k] <= tiles[k] for k in range(n)) and sum(blocks) <= 256
    assert any(blocks[k] < tiles[k] for k in range(n)), "one member must have more tiles than workgroups"
    for k in range(n):
        vec = devs[k].out("vec", (blocks[k], 4, 64))
        ba[k].vec_partials, ba[k].vec_partials_rows, ba[k].vec_stride = vec.data_ptr(), blocks[k], 64
    assert lib.nlam_mlp_bwd_group(ba, n, _stream()) == 0
    torch.cuda.synchronize()
    for k in range(n):
        P, dev = Ps[k], devs[k]
        assert dev.guards_intact() == []
        assert torch.equal(dev.t["dz1"].cpu().reshape(P.batch, P.rows, d), solo_b[k]["dz1"]), f"dz1 of member {k}"
        assert torch.equal(dev.t["dz2"].cpu().reshape(P.batch, P.rows, d), solo_b[k]["dz2"]), f"dz2 of member {k}"
        v = dev.t["vec"].cpu().double()
        got = {"db1": v[:, 0, :d].sum(0), "db2": v[:, 1, :d].sum(0)}
        if ln:
            got.update(dgamma=v[:, 2, :d].sum(0), dbeta=v[:, 3, :d].sum(0))
        ref, bud = backward_math(P, {m: solo_f[k][m].double() for m in ("z1", "xhat", "rstd") if m in solo_f[k]}, ns=mm, nblk=int(blocks[k]))
        assert compare_bounded(got, ref, bud, names=list(got)) == [], f"vec_partials of member {k}"
