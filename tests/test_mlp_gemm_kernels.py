"""Kernel-level checks of the tiled-GEMM MLP family (neural_lam_amd/csrc/nlam_gemm.inc: gemm_kernel<NS, NN>, ln_fwd_rows_kernel,
ln_bwd_rows_kernel, tile_segsum_kernel, colsum_partials_kernel) through nlam_mlp_fwd_gemm / nlam_mlp_bwd_gemm with hand-filled
structs, against the float64 math of mlp_kernel_ref.py.  The family serves every MLP with a width above 512; the kernels take any
width, so the cases name the SMALLEST shapes at which each edge of the 128 x 128 x 32 tiling exists: one row, 127 / 129 / 133 rows
(a row tile that straddles two batch items), ragged last column tiles (513, 520, 528, 1000 columns; a single output column), K of
one step (3) and of 96 steps (3072), source boundaries inside a K step and inside a column tile of the scatter epilogue.

Forward and backward run together; the backward once on the z1 / xhat / rstd the forward saved and once on the reference's.  Every
output is NaN-filled with NaN guard floats behind it; the workspace is a guarded buffer of exactly the floats the query answers;
vec_partials has more rows than nlam_mlp_bwd_gemm_blocks: the 256 rows must be written (blocks without rows: zeros), the rest
must keep its NaN fill.
  (a) exact on integers (range chosen by exact_headroom): z1 bit-equal to float64 in every case; without activation, LayerNorm
      and mean the whole chain.  A one-term (bf16x1) chain is exact only if the operands of the second and third GEMM fit in 8
      bits: ONE_TERM_CHAIN states it per case, test_one_term_chain_condition derives it on the CPU;
  (b) |got - R| <= bound element by element, the first-order budget of mlp_kernel_ref.py with the mode term of the terms
      EXECUTED (three for requested f32, bf16x2, bf16x3; one for bf16x1) and nblk = 256;
  (c) low-order probe: W1 = +-(1 + 2^-9 + 2^-18): z1 bit-equal to float64 on three terms, the integer count on one.
Identities, bit for bit: requested modes 0, 2, 3; a forward that saves nothing (z1 in the workspace); two launches; rows == 0.
Without a GPU: the stand-in kernel (torch fp32) passes the tiers on the table's shape families, six injected defects of this
family's kind are reported in the quantity they corrupt first, the workspace queries refuse what the launches refuse."""
import ctypes as C
import json
import os
import time
from dataclasses import replace

import pytest
import torch

from neural_lam_amd import _lib as L
from neural_lam_amd import graph as G_

from mlp_kernel_ref import (GUARD, Case, Dev, _combine, _same, _saved_dev, _stream, _written, backward_math, build_problem,
                            compare_bounded, compare_exact, describe_bwd, describe_fwd, dsrc_rows, exact_headroom, exact_quantities,
                            forward_math, int_problem, low_reference, rand_problem, standin_run, to_bf16)

gpu = pytest.mark.gpu

NBLK = 256        # kGemmPartBlocks: the rows of vec_partials every backward launch writes
VEC_EXTRA = 3     # rows of vec_partials behind them: must keep their NaN fill
EINVAL, EUNSUP = -1, -2

_RATIOS = {}      # (terms executed, quantity) -> largest |got - R| / bound over the tier-(b) runs


def terms(case):
    """bf16 terms the family EXECUTES for the requested mode: it has no fp32 and no two-term kernel."""
    return 1 if case.mm == 1 else 3


def _note(case, name, ratio):
    if name.startswith("dsrc") and "|" not in name:
        name = f"dsrc mode {case.dmode[int(name[4])]}"
    key = (terms(case), name)
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib = L.load()
    t0 = time.time()
    yield lib
    path = os.environ.get("NLAM_MLP_GEMM_REPORT")
    if path and _RATIOS:
        rep = {"wall_seconds": round(time.time() - t0, 2),
               "ratios": [{"terms": ns, "quantity": q, "max_ratio": v} for (ns, q), v in sorted(_RATIOS.items())]}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def K(name, widths, hid, dout, mm=3, **kw):
    """A case of this family: it has no plan codes, so `fwd` and `bwd` hold the bf16 terms the launch executes."""
    ns = 1 if mm == 1 else 3
    return Case(name, ns, ns, widths, hid, dout, mm=mm, **kw)


EDGES = dict(aggregate=True, out_perm=True, g_aggr=True)
ONE_ROW = dict(widths=(3,), hid=513, dout=1, rows=1, ln=False, no_act=True, dmode=(2,))
STRADDLE = dict(widths=(3, 700, 5), hid=528, dout=520, rows=133, batch=2, gather=(1,), perm=(0,), broadcast=(2,), dmode=(1, 2, 1), out_perm=True)
MIXED_CHAIN = dict(widths=(3, 520, 5), hid=528, dout=520, graph="mixed", batch=2, ln=False, no_act=True, add1=True, dmode=(1, 2, 3), **EDGES)
SPLIT_CHAIN = dict(widths=(3, 70, 5), hid=160, dout=130, graph="split", batch=2, ln=False, no_act=True, dmode=(1, 2, 3), **EDGES)
K3072 = dict(widths=(1024, 1024, 1024), hid=640, dout=1000, graph="mixed12", dmode=(1, 0, 3), **EDGES)
CASES = [
    # ---- dense rows: M = 1 (one K step of 3 columns, N = 513: four column tiles and one column, one output column), 127, 129,
    #      2 x 133 (three row tiles, the second one straddles the batch items; K = 708: no multiple of 32, above hid and dout)
    K("one_row_k3_dout1", **ONE_ROW),
    K("one_row_k3_dout1_x1", mm=1, **ONE_ROW),
    K("rows127_k3_f32", (3,), 640, 520, mm=0, rows=127, ln_beta=False, perm=(0,), dmode=(1,)),            # kin below hid and dout
    K("straddle_133x2", **STRADDLE),
    K("straddle_133x2_x1", mm=1, **STRADDLE),
    K("rows129_add0_bf16x2", (520, 9), 576, 520, mm=2, rows=129, add0=True, dmode=(2, 0)),                # kin between dout and hid
    K("no_data_gradient", (70, 5), 513, 130, rows=33, batch=3, ln=False, dmode=(0, 0)),                    # the dX GEMM is skipped
    K("w1_row_stride", (3, 70, 5), 160, 130, rows=65, ldw1_pad=9, perm=(1,), dmode=(2, 1, 2)),             # ldw1 > kin without NLAM_F_PRE_ADD
    K("one_kstep_two_boundaries", (3, 7, 5), 513, 17, rows=40, batch=2, perm=(0, 2), gather=(1,), dmode=(1, 2, 1)),   # K = 15
    K("rows_are_segments", (130, 130), 200, 130, rows=70, batch=2, rowseg=True, add1=True, aggregate=True, g_aggr=True, dmode=(2, 3)),
    # ---- tile lists: tiles below 32 rows, empty receivers at the start, in the middle and at the end
    K("mixed_chain", **MIXED_CHAIN),
    K("mixed_chain_x1", mm=1, **MIXED_CHAIN),
    K("mixed_add0_aggr_gradient_only", (520, 3, 5), 528, 520, graph="mixed", roles="rse", add0=True, mean=True, aggregate=True, g_out=False,
      g_aggr=True, dmode=(3, 0, 1)),                                     # the residual gradient of source 0 is zero
    K("mixed_out_gradient_only", (5, 520, 3), 528, 520, graph="mixed", roles="ser", batch=3, add1=True, ln_beta=False, aggregate=True,
      out_perm=True, dmode=(2, 1, 3)),
    K("mixed12_chain_add01", (130, 130, 130), 200, 130, graph="mixed12", ln=False, no_act=True, add0=True, add1=True, dmode=(1, 2, 3), **EDGES),
    # ---- receivers above 32 in-edges: NLAM_TILE_SPLIT tiles (atomic adds into zeroed destinations), and the virtual split
    K("split_atomic_chain", atomic=True, **SPLIT_CHAIN),
    K("split_atomic_chain_x1", mm=1, atomic=True, **SPLIT_CHAIN),
    K("split_virtual_chain", **SPLIT_CHAIN),
    K("split9_virtual_ln_mean", (520, 520, 520), 640, 520, graph="split9", batch=2, mean=True, add0=True, add1=True, dmode=(1, 2, 0), **EDGES),
    K("split9_atomic_aggr_only", (520, 520, 520), 640, 520, graph="split9", atomic=True, mean=True, want_out=False, aggregate=True,
      g_out=False, g_aggr=True, dmode=(0, 2, 3)),
    # ---- K = 3072: 96 K steps in GEMM1, 3072 output columns (24 column tiles, three sources) in the dX GEMM
    K("k3072", **K3072),
    K("k3072_x1", mm=1, **K3072),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
INT_SEED, RAND_SEED, LOW_SEED = 11, 12, 13

# one term: is the chain without activation, LayerNorm and mean exact?  Only if z1, dz2 and dz1 (the A operands of the second GEMM
# and of the two backward GEMMs) are bf16 values.  Derived on the CPU by test_one_term_chain_condition, never on the GPU.
ONE_TERM_CHAIN = {"one_row_k3_dout1_x1": True, "mixed_chain_x1": False, "split_atomic_chain_x1": True}


def is_chain(c):
    return c.no_act and not c.ln and not c.mean


def exact_names(case, forward):
    names = exact_quantities(case, forward)
    if terms(case) == 1 and is_chain(case) and not ONE_TERM_CHAIN[case.name]:
        # z1 only; dz2 = g_out + g_aggr and its column sum pass through no matrix product
        names = ["z1"] if forward else ["dz2", "db2"]
    return names


def one_term_operands_fit(P):
    """The float64 chain's z1, dz2 and dz1 are bf16 values (8 significant bits): a one-term GEMM reads them exactly."""
    ref_f, _ = forward_math(P)
    ref_b, _ = backward_math(P, {"z1": ref_f["z1"]})
    return all(torch.equal(to_bf16(t), t) for t in (ref_f["z1"], ref_b["dz2"], ref_b["dz1"]))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU: the case table, the stand-in, the injected defects, the refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_edges():
    seen = {k: set() for k in range(3)}
    for c in CASES:
        for k in range(len(c.widths)):
            seen[k].add(c.dmode[k])
    assert all(seen[k] == {0, 1, 2, 3} for k in range(3)), seen
    assert {len(c.widths) for c in CASES} == {1, 2, 3}
    flag_sets = {(c.add0, c.add1) for c in CASES}
    assert {(True, False), (False, True), (True, True), (False, False)} <= flag_sets
    assert {(c.g_out, c.g_aggr) for c in CASES} == {(True, False), (False, True), (True, True)}
    assert any(c.add0 and c.g_aggr and not c.g_out for c in CASES)
    assert any(c.ln and not c.ln_beta for c in CASES) and any(c.ln and c.ln_beta for c in CASES) and any(not c.ln for c in CASES)
    assert any(c.mean for c in CASES) and any(c.no_act for c in CASES) and any(c.out_perm for c in CASES)
    assert any(c.atomic for c in CASES) and any(c.graph.startswith("split") and not c.atomic for c in CASES) and any(c.rowseg for c in CASES)
    assert any(c.gather for c in CASES) and any(c.perm for c in CASES) and any(c.broadcast for c in CASES) and any(c.ldw1_pad for c in CASES)
    assert all(not any(c.dmode[: len(c.widths)]) for c in CASES if c.name == "no_data_gradient")
    for c in CASES:   # what the family is about: a ragged tile edge somewhere in every case
        kin = sum(c.widths)
        assert kin % 32 or c.hid % 128 or c.dout % 128 or (c.batch * max(c.rows, 1)) % 128, c.name
    assert {terms(c) for c in CASES} == {1, 3} and {c.mm for c in CASES} == {0, 1, 2, 3}
    # a row tile of 128 that holds rows of two batch items
    assert any(c.batch > 1 and c.rows and c.rows % 128 for c in CASES)


def test_chain_exact_headroom():
    """exact_headroom decides the integer range and which shapes can be chain-exact at all: the chain cases of the table have a
    range, the 3 x 520 -> 640 -> 520 and K = 3072 shapes have none (they are z1-exact only, with LayerNorm on)."""
    want = {"mixed_chain": 2}
    for c in CASES:
        if is_chain(c):
            P = int_problem(c, INT_SEED)
            assert P.irange >= 1 and exact_headroom(P) < 2.0 ** 24, c.name
            if c.name in want:
                assert P.irange == want[c.name], (c.name, P.irange)
    for name in ("split9_virtual_ln_mean", "k3072"):
        c = replace(CASE_BY_NAME[name], ln=False, no_act=True, mean=False)
        with pytest.raises(AssertionError, match="no integer range"):
            int_problem(c, INT_SEED)
        int_problem(CASE_BY_NAME[name], INT_SEED)   # z1 alone has a range


def test_one_term_chain_condition():
    chains = [c for c in CASES if terms(c) == 1 and is_chain(c)]
    assert {c.name for c in chains} == set(ONE_TERM_CHAIN)
    for c in chains:
        assert one_term_operands_fit(int_problem(c, INT_SEED)) == ONE_TERM_CHAIN[c.name], c.name
    assert any(ONE_TERM_CHAIN.values()) and not all(ONE_TERM_CHAIN.values())


# the shape families of the table, each with a tile-list geometry, every residual the widths allow and both gradients
STANDIN = {
    "mixed": Case("standin_mixed", 3, 3, (3, 520, 5), 528, 520, graph="mixed", batch=2, add1=True, dmode=(1, 2, 3), **EDGES),
    "mixed12": Case("standin_mixed12", 3, 3, (130, 130, 130), 200, 130, graph="mixed12", add0=True, add1=True, dmode=(1, 2, 3), **EDGES),
    "split": Case("standin_split", 3, 3, (3, 70, 5), 160, 130, graph="split", batch=2, dmode=(1, 2, 3), **EDGES),
    "split9": Case("standin_split9", 3, 3, (520, 520, 520), 640, 520, graph="split9", add0=True, add1=True, dmode=(1, 2, 3), **EDGES),
    "k3072": Case("standin_k3072", 3, 3, (1024, 1024, 1024), 640, 1000, graph="mixed12", dmode=(1, 0, 3), **EDGES),
    "dense": Case("standin_dense", 3, 3, (3, 700, 5), 528, 520, rows=133, batch=2, gather=(1,), perm=(0,), broadcast=(2,), dmode=(1, 2, 1)),
}


@pytest.mark.parametrize("family", list(STANDIN))
def test_standin_passes_on_the_table_shapes(family):
    """The CPU stand-in (torch fp32) passes tiers (a) to (c) on every shape family of the table, LayerNorm on and off, mean on and
    off, with the budget of one and of three executed terms (the one-term budget contains the three-term one); a dense case has
    no g_aggr (standin_run used to index it regardless)."""
    case = STANDIN[family]
    big = family in ("split9", "k3072")
    variants = [case, replace(case, ln=False)]
    if case.graph and not big:
        variants += [replace(case, mean=True), replace(case, ln=False, mean=True, g_out=False)]
    if family in ("mixed", "mixed12", "split"):
        variants.append(replace(case, ln=False, no_act=True))
    for c in variants:
        assert standin_run(c, "int", nblk=NBLK) == [], c
        for ns in (3,) if big else (1, 3):
            assert standin_run(c, "rand", ns_claimed=ns, nblk=NBLK) == [], (c, ns)
    assert standin_run(case, "low", ns_claimed=3) == []


DEFECT_CASE = Case("defects", 3, 3, (3, 70, 5), 160, 130, graph="split", batch=2, mean=True, dmode=(1, 2, 3), **EDGES)
FORWARD = ("z1", "xhat", "rstd", "out", "aggr")
FIRST = {"boundary_column_from_neighbour": "z1", "second_item_first_row_from_first_item": "z1", "last_column_tile_without_bias": "z1",
         "w2_untransposed_in_dz1": "dz1", "dmode1_scatter_through_wrong_index": "dsrc0", "mean_scale_missing_in_backward": "dz2"}
UPSTREAM = {"z1": (), "dz2": FORWARD, "dz1": FORWARD + ("dz2", "db2", "dgamma", "dbeta"),
            "dsrc0": FORWARD + ("dz2", "db2", "dgamma", "dbeta", "dz1", "db1")}


@pytest.mark.parametrize("defect", list(FIRST))
def test_injected_defect_is_reported(defect):
    """Defects of the kind this family can have (operands concatenated on load, row tiles over two batch items, ragged column
    tiles, W2 read in both layouts, a destination per column): each fails the bounded comparison in the quantity it corrupts
    first and in nothing upstream of it; the z1 defects fail the exact tier too."""
    first = FIRST[defect]
    assert DEFECT_CASE.hid != DEFECT_CASE.dout and DEFECT_CASE.hid % 128
    assert standin_run(DEFECT_CASE, "rand", ns_claimed=3, nblk=NBLK) == []
    bad = standin_run(DEFECT_CASE, "rand", defect, ns_claimed=3, nblk=NBLK)
    assert first in bad and not set(bad) & set(UPSTREAM[first]), (defect, bad)
    if first == "z1":
        assert "z1" in standin_run(DEFECT_CASE, "int", defect, nblk=NBLK), defect
    if defect == "w2_untransposed_in_dz1":
        assert "dz1" in standin_run(replace(DEFECT_CASE, ln=False, no_act=True, mean=False), "int", defect, nblk=NBLK)


def _fake(P):
    return lambda n: None if ((n.startswith("idx") and P.srcs[int(n[3:])].idx is None) or (n == "tiles" and P.tiles is None)
                              or (n == "out_idx" and P.out_idx is None)) else 4096


def describe_both(lib, P):
    """Both descriptors on placeholder addresses, complete enough to pass every check (host logic only)."""
    pf = describe_fwd(P, _fake(P))
    pf.wpack, pf.wpack_floats = 4096, 1 << 40
    pb = describe_bwd(P, _fake(P), lib)
    pb.dz2_ld = 0
    pb.wpack, pb.wpack_floats = 4096, 1 << 40
    pb.vec_partials, pb.vec_partials_rows, pb.vec_stride = 4096, NBLK, 64 * -(-max(P.hid, P.dout) // 64)
    return pf, pb


def test_workspace_queries_refuse_what_the_launches_refuse():
    """nlam_mlp_*_gemm_workspace_floats answer the code the launch returns (every launch below returns before it could start a
    kernel: the descriptors hold placeholder addresses)."""
    lib = L.load()
    null = C.c_void_p(0)
    P = build_problem(CASE_BY_NAME["mixed_add0_aggr_gradient_only"], 1, "int")
    fq, bq = lib.nlam_mlp_fwd_gemm_workspace_floats, lib.nlam_mlp_bwd_gemm_workspace_floats
    pf, pb = describe_both(lib, P)
    M = P.batch * P.rows
    assert fq(C.byref(pf)) == M * P.dout and bq(C.byref(pb)) == M * P.dout + M * P.case.widths[0]
    for flag in (L.F_PRE_ADD, L.F_STORE_BF16, L.F_ACC_DSRC0, L.F_LEAF_WGRAD):
        pf, pb = describe_both(lib, P)
        pf.flags |= flag
        pb.flags |= flag
        assert fq(C.byref(pf)) == EUNSUP == lib.nlam_mlp_fwd_gemm(C.byref(pf), null), flag
        assert bq(C.byref(pb)) == EUNSUP == lib.nlam_mlp_bwd_gemm(C.byref(pb), null), flag
    pf, pb = describe_both(lib, P)
    pf.ncat = 1
    assert fq(C.byref(pf)) == EUNSUP == lib.nlam_mlp_fwd_gemm(C.byref(pf), null)
    for ld in (P.dout - 1, P.dout + 1, 32 * -(-P.dout // 32)):
        pf, pb = describe_both(lib, P)
        pb.dz2_ld = ld
        assert bq(C.byref(pb)) == EINVAL == lib.nlam_mlp_bwd_gemm(C.byref(pb), null), ld
    pf, pb = describe_both(lib, P)
    pb.dz2_ld = P.dout
    assert bq(C.byref(pb)) > 0
    pf, pb = describe_both(lib, P)
    pb.vec_partials_rows = NBLK - 1
    assert lib.nlam_mlp_bwd_gemm_blocks(C.byref(pb)) == NBLK
    assert bq(C.byref(pb)) == EINVAL == lib.nlam_mlp_bwd_gemm(C.byref(pb), null)
    # a workspace one float short: the query cannot know, the launch refuses
    pf, pb = describe_both(lib, P)
    pf.wpack_floats, pb.wpack_floats = fq(C.byref(pf)) - 1, bq(C.byref(pb)) - 1
    assert fq(C.byref(pf)) == pf.wpack_floats + 1 and bq(C.byref(pb)) == pb.wpack_floats + 1
    assert lib.nlam_mlp_fwd_gemm(C.byref(pf), null) == EINVAL and lib.nlam_mlp_bwd_gemm(C.byref(pb), null) == EINVAL
    # the forward's query grows by M * hid when z1 is not saved
    pf, pb = describe_both(lib, P)
    pf.z1 = pf.xhat = pf.rstd = None
    assert fq(C.byref(pf)) == M * (P.dout + P.hid)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU side: the launches
# ---------------------------------------------------------------------------------------------------------------------------
def run_forward(lib, P, dev, save=True):
    """One nlam_mlp_fwd_gemm launch on fresh NaN-filled outputs and a workspace of exactly the floats the query answers -> host
    tensors.  save = False: z1, xhat and rstd are NULL (an inference launch: z1 then lives in the workspace)."""
    c = P.case
    dev.outs = {}
    for n in ("z1", "xhat", "rstd"):
        dev.t.pop(n, None)
    if c.want_out:
        dev.out("out", (P.batch, P.out_rows, c.dout))
    if c.aggregate:
        dev.out("aggr", (P.batch, P.nseg_rows, c.dout), zero=P.has_split)
    if save:
        dev.out("z1", (P.batch, P.rows, c.hid))
        if c.ln:
            dev.out("xhat", (P.batch, P.rows, c.dout))
            dev.out("rstd", (P.batch, P.rows))
    p = describe_fwd(P, dev.addr)
    M = P.batch * P.rows
    need = lib.nlam_mlp_fwd_gemm_workspace_floats(C.byref(p))
    assert need == M * c.dout + (0 if save else M * c.hid), c.name
    p.wpack, p.wpack_floats = dev.out("ws", (need,)).data_ptr(), need
    assert lib.nlam_mlp_fwd_gemm(C.byref(p), _stream()) == 0, c.name
    if c.aggregate and P.comb is not None:
        _combine(lib, dev, dev.t["aggr"], c.dout)
    torch.cuda.synchronize()
    assert dev.guards_intact() == [], f"{c.name}: forward wrote behind an output or behind its workspace"
    res = {n: dev.t[n].float().cpu() for n in dev.outs if n != "ws"}
    if c.aggregate:
        res["aggr"] = res["aggr"][:, : P.nseg]
    return res


def run_backward(lib, P, dev, saved):
    """One nlam_mlp_bwd_gemm launch -> host tensors + the four vectors (the 256 rows of vec_partials summed in float64)."""
    c = P.case
    dev.outs = {}
    for n in ("z1", "xhat", "rstd"):
        if n in saved:
            dev.t[n] = saved[n]
    M = P.batch * P.rows
    dev.out("dz1", (M, c.hid))
    dev.out("dz2", (M, c.dout))
    for k in range(P.nsrc):
        if c.dmode[k] != 0:
            dev.out(f"dsrc{k}", (P.batch, dsrc_rows(P, k), c.widths[k]), zero=c.dmode[k] == 3 and P.has_split)
    vs = 64 * -(-max(c.hid, c.dout) // 64)
    vec = dev.out("vec", (NBLK + VEC_EXTRA, 4, vs))
    p = describe_bwd(P, dev.addr, lib)
    p.dz2_ld = c.dout if c.batch > 1 else 0   # both spellings of "rows of dout floats"
    p.vec_partials, p.vec_partials_rows, p.vec_stride = vec.data_ptr(), NBLK + VEC_EXTRA, vs
    assert lib.nlam_mlp_bwd_gemm_blocks(C.byref(p)) == NBLK
    need = lib.nlam_mlp_bwd_gemm_workspace_floats(C.byref(p))
    assert need == (M * c.dout if (c.ln or c.add1) else 0) + sum(M * c.widths[k] for k in range(P.nsrc) if c.dmode[k] == 3), c.name
    if need:
        p.wpack, p.wpack_floats = dev.out("ws", (need,)).data_ptr(), need
    assert lib.nlam_mlp_bwd_gemm(C.byref(p), _stream()) == 0, c.name
    for k in range(P.nsrc):
        if c.dmode[k] == 3 and P.comb is not None:
            _combine(lib, dev, dev.t[f"dsrc{k}"], c.widths[k])
    torch.cuda.synchronize()
    assert dev.guards_intact() == [], f"{c.name}: backward wrote behind an output or behind its workspace"
    res = {n: dev.t[n].float().cpu() for n in dev.outs if n != "ws"}
    res["dz1"] = res["dz1"].reshape(P.batch, P.rows, c.hid)
    res["dz2"] = res["dz2"].reshape(P.batch, P.rows, c.dout)
    for k in range(P.nsrc):
        if c.dmode[k] == 3:
            res[f"dsrc{k}"] = res[f"dsrc{k}"][:, : P.nseg]
    v = res.pop("vec").double()
    assert bool(torch.isnan(v[NBLK:]).all()), f"{c.name}: rows of vec_partials behind the 256 were written"
    assert bool(torch.isfinite(v[:NBLK]).all()), f"{c.name}: a row of vec_partials among the 256 was not written"
    span = -(-M // NBLK)
    assert torch.count_nonzero(v[-(-M // span): NBLK]) == 0, f"{c.name}: blocks without rows must hold zeros"
    assert torch.count_nonzero(v[:NBLK, 0, c.hid:]) == 0 and torch.count_nonzero(v[:NBLK, 1:, c.dout:]) == 0, f"{c.name}: columns past a width"
    if not c.ln:
        assert torch.count_nonzero(v[:NBLK, 2]) == 0, f"{c.name}: the dgamma row without LayerNorm"
    v = v[:NBLK]
    res["db1"], res["db2"] = v[:, 0, : c.hid].sum(0), v[:, 1, : c.dout].sum(0)
    if c.ln:
        res["dgamma"], res["dbeta"] = v[:, 2, : c.dout].sum(0), v[:, 3, : c.dout].sum(0)
    return res


def _same_fixed_order(case, a, b):
    """_same over what is summed in a fixed order: the aggregates and dmode-3 gradients of NLAM_TILE_SPLIT tiles are atomic sums
    in no fixed order and are compared bounded only."""
    loose = {"aggr"} | {f"dsrc{k}" for k, m in enumerate(case.dmode) if m == 3} if case.atomic else set()
    return [n for n in _same(a, b) if n not in loose]


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_exact_on_integers(lib, case):
    """Tier (a): z1 bit-equal to float64 in every case; the whole chain where nothing can round (integer sums below 2^24 are exact
    in any order, the atomic ones included)."""
    P = int_problem(case, INT_SEED)
    dev = Dev(P)
    got_f = run_forward(lib, P, dev)
    _written(got_f, f"{case} forward")
    ref_f, _ = forward_math(P)
    assert compare_exact(got_f, ref_f, exact_names(case, True)) == [], f"{case}: forward is not the exact result"
    got_b = run_backward(lib, P, dev, _saved_dev(got_f))
    _written(got_b, f"{case} backward")
    ref_b, _ = backward_math(P, {k: got_f[k].double() for k in ("z1", "xhat", "rstd") if k in got_f})
    assert compare_exact(got_b, ref_b, exact_names(case, False)) == [], f"{case}: backward is not the exact result"


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_elementwise_error_budget(lib, case):
    """Tier (b): every output, saved tensor, gradient and vector within its propagated budget; the stages behind GEMM1 also on
    their own (continued from the kernel's z1); the backward on the kernel's saved tensors and on the reference's; two launches
    are bit-equal in everything that is summed in a fixed order."""
    P = rand_problem(case, RAND_SEED)
    dev = Dev(P)
    ns = terms(case)
    got_f = run_forward(lib, P, dev)
    _written(got_f, f"{case} forward")
    keep = _saved_dev(got_f)
    assert _same_fixed_order(case, got_f, run_forward(lib, P, dev)) == [], f"{case}: two forward launches differ"
    ref_f, bud_f = forward_math(P, ns=ns)
    bad = compare_bounded(got_f, ref_f, bud_f, note=lambda n, r: _note(case, n, r))
    ref_2, bud_2 = forward_math(P, ns=ns, z1_given=got_f["z1"].double())
    later = [n for n in ref_2 if n != "z1"]
    bad += [n + "|z1" for n in compare_bounded(got_f, ref_2, bud_2, names=later, note=lambda n, r: _note(case, n + "|z1", r))]
    assert bad == [], f"{case}: forward over its budget in {bad}"
    got_b = run_backward(lib, P, dev, keep)
    _written(got_b, f"{case} backward")
    assert _same_fixed_order(case, got_b, run_backward(lib, P, dev, keep)) == [], f"{case}: two backward launches differ"
    ref_b, bud_b = backward_math(P, {k: got_f[k].double() for k in keep}, ns=ns, nblk=NBLK)
    bad = compare_bounded(got_b, ref_b, bud_b, note=lambda n, r: _note(case, n, r))
    assert bad == [], f"{case}: backward (on the kernel's saved tensors) over its budget in {bad}"
    rounded = {k: ref_f[k].float() for k in keep}   # the reference's, as stored
    got_r = run_backward(lib, P, dev, {k: v.cuda() for k, v in rounded.items()})
    ref_r, bud_r = backward_math(P, {k: v.double() for k, v in rounded.items()}, ns=ns, nblk=NBLK)
    bad = compare_bounded(got_r, ref_r, bud_r, note=lambda n, r: _note(case, n, r))
    assert bad == [], f"{case}: backward (on the reference's saved tensors) over its budget in {bad}"


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_gemm1_low_order_terms(lib, case):
    """Tier (c): every three-term forward (requested f32, bf16x2, bf16x3) keeps all three bf16 terms of W1 -- z1 bit-equal to
    float64; the one-term forward gives the integer count."""
    P = build_problem(case, LOW_SEED, "low")
    got = run_forward(lib, P, Dev(P))
    assert torch.equal(got["z1"].double(), low_reference(P, terms(case))), f"{case}: z1 of the low-order probe ({terms(case)} terms)"


MODE_CASES = ["straddle_133x2", "mixed_out_gradient_only", "split9_virtual_ln_mean", "rows_are_segments"]


@gpu
@pytest.mark.parametrize("name", MODE_CASES)
def test_three_term_modes_are_bit_identical(lib, name):
    """Requested modes f32, bf16x2 and bf16x3 run the same three-term kernels: the same bits in every output of both directions."""
    base = CASE_BY_NAME[name]
    assert not base.atomic
    runs = []
    for mm in (0, 2, 3):
        P = rand_problem(replace(base, mm=mm), RAND_SEED)
        dev = Dev(P)
        f = run_forward(lib, P, dev)
        runs.append((f, run_backward(lib, P, dev, _saved_dev(f))))
    for f, b in runs[1:]:
        assert _same(runs[0][0], f) == [] and _same(runs[0][1], b) == [], name


SAVE_CASES = ["one_row_k3_dout1", "straddle_133x2_x1", "mixed_add0_aggr_gradient_only", "split_virtual_chain", "k3072"]


@gpu
@pytest.mark.parametrize("name", SAVE_CASES)
def test_forward_without_saved_tensors_is_bit_identical(lib, name):
    """z1 = xhat = rstd = NULL: z1 lives in the workspace (the query grows by M * hid, run_forward asserts it and guards the
    buffer); out and aggr are those of the saving launch."""
    case = CASE_BY_NAME[name]
    P = rand_problem(case, RAND_SEED)
    dev = Dev(P)
    saving = run_forward(lib, P, dev)
    plain = run_forward(lib, P, dev, save=False)
    assert set(plain) == set(saving) - {"z1", "xhat", "rstd"} and plain
    _written(plain, f"{name} without saved tensors")
    assert _same(plain, saving) == [], name


@gpu
def test_launch_without_rows(lib):
    """rows == 0 (nlam_gemm.inc): aggr rows of the receivers the tile list covers and dmode-3 dsrc are zeros, the 256 vec_partials
    rows are zeros, every other output keeps its NaN fill, the return code is 0 -- with wpack == NULL, as the query answers 0."""
    d, hid, nseg = 520, 528, 5
    rowptr = torch.zeros(nseg + 1, dtype=torch.int32)
    tiles, _, _ = G_.build_tile_schedule(rowptr)
    tiles, rowptr = tiles.cuda(), rowptr.cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    W1, b1, W2, b2 = torch.randn(hid, 3 * d).cuda(), torch.randn(hid).cuda(), torch.randn(d, hid).cuda(), torch.randn(d).cuda()
    gamma, beta = torch.randn(d).cuda(), torch.randn(d).cuda()
    srcs = [torch.randn(1, 4, d).cuda() for _ in range(3)]
    out, z1, xhat, rstd = nan(4 * d), nan(4 * hid), nan(4 * d), nan(4)
    aggr = nan(nseg * d + GUARD)
    p = L.MlpFwd()
    p.nsrc, p.batch, p.rows, p.ntiles, p.tiles = 3, 1, 0, int(tiles.shape[0]), tiles.data_ptr()
    for k, t in enumerate(srcs):
        p.src[k].ptr, p.src[k].width, p.src[k].bstride = t.data_ptr(), d, 4 * d
    p.W1, p.b1, p.W2, p.b2, p.ln_w, p.ln_b = (t.data_ptr() for t in (W1, b1, W2, b2, gamma, beta))
    p.hid, p.dout, p.eps, p.flags = hid, d, 1e-5, L.F_ADD_SRC0 | L.F_MEAN
    inv_deg = torch.zeros(nseg).cuda()
    p.out, p.out_bstride, p.z1, p.xhat, p.rstd = out.data_ptr(), 0, z1.data_ptr(), xhat.data_ptr(), rstd.data_ptr()
    p.aggr, p.rowptr, p.inv_deg, p.nseg_total = aggr.data_ptr(), rowptr.data_ptr(), inv_deg.data_ptr(), nseg
    assert lib.nlam_mlp_fwd_gemm_workspace_floats(C.byref(p)) == 0
    assert lib.nlam_mlp_fwd_gemm(C.byref(p), _stream()) == 0
    q = L.MlpBwd()
    q.nsrc, q.batch, q.rows, q.ntiles, q.tiles = 3, 1, 0, int(tiles.shape[0]), tiles.data_ptr()
    for k, t in enumerate(srcs):
        q.src[k].ptr, q.src[k].width, q.src[k].bstride = t.data_ptr(), d, 4 * d
    q.W1, q.W2, q.ln_w, q.hid, q.dout, q.nseg_total, q.flags = W1.data_ptr(), W2.data_ptr(), gamma.data_ptr(), hid, d, nseg, L.F_ADD_SRC0 | L.F_MEAN
    g_aggr, g_out, seg_of_row = nan(nseg * d), nan(4 * d), torch.zeros(1, dtype=torch.int32).cuda()
    q.g_aggr, q.seg_of_row, q.rowptr, q.inv_deg = g_aggr.data_ptr(), seg_of_row.data_ptr(), rowptr.data_ptr(), inv_deg.data_ptr()
    q.g_out, q.out_bstride = g_out.data_ptr(), 0
    dz1, dz2, d0, d1 = nan(4 * hid), nan(4 * d), nan(4 * d), nan(4 * d)
    q.z1, q.xhat, q.rstd, q.dz1, q.dz2 = z1.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), dz1.data_ptr(), dz2.data_ptr()
    drec = nan(nseg * d + GUARD)
    q.dmode[0], q.dsrc[0], q.dsrc_bstride[0] = 1, d0.data_ptr(), 4 * d
    q.dmode[1], q.dsrc[1], q.dsrc_bstride[1] = 2, d1.data_ptr(), 4 * d
    q.dmode[2], q.dsrc[2], q.dsrc_bstride[2] = 3, drec.data_ptr(), nseg * d
    vs = 576
    vecp = nan(NBLK + VEC_EXTRA, 4, vs)
    q.vec_partials, q.vec_partials_rows, q.vec_stride = vecp.data_ptr(), NBLK + VEC_EXTRA, vs
    assert lib.nlam_mlp_bwd_gemm_workspace_floats(C.byref(q)) == 0
    assert lib.nlam_mlp_bwd_gemm(C.byref(q), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.count_nonzero(aggr[: nseg * d]) == 0 and torch.count_nonzero(drec[: nseg * d]) == 0
    assert torch.count_nonzero(vecp[:NBLK]) == 0
    kept = dict(out=out, z1=z1, xhat=xhat, rstd=rstd, dz1=dz1, dz2=dz2, dsrc0=d0, dsrc1=d1, aggr_guard=aggr[nseg * d:],
                dsrc2_guard=drec[nseg * d:], vec_extra=vecp[NBLK:])
    assert [n for n, t in kept.items() if not bool(torch.isnan(t).all())] == [], "written by a launch without rows"
