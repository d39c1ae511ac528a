"""Kernel-level checks of the aggregation kernels (segment_sum_kernel, segment_sum_split_kernel<2|4>, segment_sum_bf16_kernel,
split_combine_kernel) through the five C entry points nlam_segment_sum, _acc, _add, _bf16 and nlam_split_combine, against the
float64 math of linear_segsum_ref.py.  Segment lengths sit at the edges of the kernels' 8-row batches (0, 1, 7, 8, 9, 15, 16, 17
for one thread per segment; 8 S and its neighbours for S lane groups per segment), the last wave of a split launch has dead lanes,
one case per kernel has more threads than the 4096 x 256 of the grid-stride cap, and every fp32 kernel also runs without `order`,
without `scale`, with repeated row ids and through _acc / _add.  Each case states the nlam_segment_sum_groups answer it is built for.
Every output is NaN-filled with NaN guard floats behind it; the floats between the batch items of an input are NaN.
  (a) exact on integers in [-4, 4] with scales in {0.25, 0.5, 1, 2}: bit-equal to float64;
  (b) random data, scale = 1 / len: |got - R| <= U (len + 4) |scale| sum |in| + U (|extra| + |prev| + |R|) element by element.
Identities: two launches are bit-equal; nseg == 0 writes nothing.
Without a GPU: the kernel each case takes, the stand-in passing both tiers, six injected defects reported, the refusals."""
import json
import os
import time

import pytest
import torch

from neural_lam_amd import _lib as L

from linear_segsum_ref import (PLAIN_CYCLE, SEG_DEFECTS, Bufs, CombCase, SegCase, bf16_bits, comb_problem, combine_math, compare_bounded,
                               compare_exact, seg_problem, seg_standin, segsum_math, split_cycle)
from mlp_kernel_ref import _stream

gpu = pytest.mark.gpu
EINVAL, EUNSUP = -1, -2
GRID_CAP_THREADS = 4096 * 256      # elementwise_blocks(total, 256 * 16) workgroups of 256 threads
KERNEL = {0: "segment_sum_bf16_kernel", 1: "segment_sum_kernel", 2: "segment_sum_split_kernel<2>", 4: "segment_sum_split_kernel<4>"}
_RATIOS = {}      # kernel -> largest |got - R| / bound over the tier-(b) runs

PLAIN = PLAIN_CYCLE * 3
SPLIT4 = split_cycle(4) * 2 + (150,)     # one long segment: 35 rows on average
SPLIT2 = split_cycle(2) * 2 + (200,)     # 24 rows on average
LENS = {1: PLAIN, 2: SPLIT2, 4: SPLIT4}
WIDTH = {1: 64, 2: 128, 4: 64}

CASES = [SegCase(f"plain_w{w}", 1, w, PLAIN) for w in (64, 128, 256, 20, 17, 3)]     # float4 path; w4 = 5; the scalar path
CASES += [SegCase("plain_shared_input_w64", 1, 64, SPLIT4, shared=True)]             # in_bstride = 0: the row count is unknown
CASES += [SegCase(f"split4_w{w}", 4, w, SPLIT4) for w in (4, 16, 32, 64)]
CASES += [SegCase("split2_w128", 2, 128, SPLIT2)]
for g_ in (1, 2, 4):   # each fp32 kernel: order = NULL, scale = NULL, repeated row ids, _acc and _add on integer contents
    nm = {1: "plain", 2: "split2", 4: "split4"}[g_]
    CASES += [SegCase(f"{nm}_no_order", g_, WIDTH[g_], LENS[g_], order="none"),
              SegCase(f"{nm}_no_scale", g_, WIDTH[g_], LENS[g_], scale=False),
              SegCase(f"{nm}_repeated_ids", g_, WIDTH[g_], LENS[g_], order="repeat"),
              SegCase(f"{nm}_acc", g_, WIDTH[g_], LENS[g_], entry="acc"),
              SegCase(f"{nm}_add", g_, WIDTH[g_], LENS[g_], entry="add")]
CASES += [SegCase(f"bf16_w{w}", 0, w, PLAIN, entry="bf16") for w in (8, 64, 136, 256)]
CASES += [SegCase("bf16_no_order_no_scale", 0, 64, PLAIN, entry="bf16", order="none", scale=False)]
# more threads than the grid-stride cap: every workgroup walks a second element
CASES += [SegCase("plain_grid_stride", 1, 64, (0, 1, 2, 3) * 16500, batch=1, tiers="a"),
          SegCase("split4_grid_stride", 4, 16, (16, 17) * 33000, batch=1, tiers="a"),
          SegCase("bf16_grid_stride", 0, 64, (0, 1, 2, 3) * 33000, entry="bf16", batch=1, tiers="a")]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

COMB = [CombCase(f"combine_w{w}", w, (1, 2, 5, 2)) for w in (3, 64, 130, 300)]     # 64, 64, 128 and 256 threads; column loops that do not divide
COMB += [CombCase("combine_in_place_w130", 130, (2, 5, 1), in_place=True)]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib = L.load()
    t0 = time.time()
    yield lib
    path = os.environ.get("NLAM_SEGSUM_REPORT")
    if path and _RATIOS:
        rep = {"wall_seconds": round(time.time() - t0, 2), "ratios": [{"kernel": k, "max_ratio": v} for k, v in sorted(_RATIOS.items())]}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)


def threads(c):
    """Threads a launch of the case needs before the cap."""
    nseg = len(c.lens)
    if c.groups == 0:
        return c.batch * nseg * (c.width // 8)
    if c.groups == 1:
        return c.batch * nseg * ((c.width + 3) // 4)
    return c.batch * nseg * c.groups * (c.width // 4)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_cases_take_the_kernel_they_are_built_for():
    lib = L.load()
    seen = set()
    for c in CASES:
        P = seg_problem(c, 1, "int") if len(c.lens) < 1000 else None
        nseg, total = len(c.lens), sum(c.lens)
        in_bstride = 0 if c.shared else max(total, 1) * c.width + c.pad
        assert P is None or (P.in_bstride == in_bstride and P.nseg == nseg)
        if c.groups:
            assert lib.nlam_segment_sum_groups(in_bstride, nseg, c.width) == c.groups, c.name
            if c.groups > 1:   # the rule of the header: 16+ rows per segment on average, known from the batch stride
                assert in_bstride // c.width >= 16 * nseg and c.width % 4 == 0 and 64 % (c.width // 4) == 0
                if "grid_stride" not in c.name:
                    assert threads(c) % 256 != 0, f"{c}: the last workgroup must have dead lanes"
                    S = c.groups
                    assert set(split_cycle(S)) <= set(c.lens) and {8 * S - 1, 8 * S, 8 * S + 1, 0, 1} <= set(c.lens)
            elif c.lens == PLAIN:
                assert {0, 1, 7, 8, 9, 15, 16, 17} <= set(c.lens)
        seen.add((c.groups, c.entry, c.order, c.scale))
        if "grid_stride" in c.name:
            assert threads(c) > GRID_CAP_THREADS, c.name
    for g in (1, 2, 4):
        for key in ((g, "sum", "none", True), (g, "sum", "perm", False), (g, "sum", "repeat", True), (g, "acc", "perm", True), (g, "add", "perm", True)):
            assert key in seen, key
    # the rule itself, at its edges
    G = lib.nlam_segment_sum_groups
    assert [G(16 * 10 * w, 10, w) for w in (4, 8, 16, 32, 64, 128)] == [4, 4, 4, 4, 4, 2]
    assert [G(16 * 10 * w - 1, 10, w) for w in (4, 64, 128)] == [1, 1, 1]          # fewer than 16 rows per segment
    assert [G(1 << 20, 10, w) for w in (256, 20, 24, 17, 3, 48)] == [1] * 6        # width / 4 above 32 or no divisor of 64
    assert G(0, 10, 64) == 1 and G(64, 1, 0) == EINVAL and G(64, -1, 4) == EINVAL


STANDIN = ("plain_w64", "plain_w17", "plain_shared_input_w64", "split4_w16", "split2_w128", "plain_no_order", "split4_no_scale",
           "split2_repeated_ids", "plain_acc", "split4_add", "bf16_w136")


@pytest.mark.parametrize("name", STANDIN)
def test_standin_passes_both_tiers(name):
    assert seg_standin(BY_NAME[name], "int") == [] and seg_standin(BY_NAME[name], "rand") == []


FIRST = {
    "tail_row_past_the_end_added": "plain_w64",
    "lane_group_partial_left_out": "split4_w16",
    "scale_applied_to_extra": "split2_add",
    "acc_overwrites": "plain_acc",
    "order_ignored": "split4_w64",
    "empty_segment_unwritten": "bf16_w64",
}


@pytest.mark.parametrize("defect", SEG_DEFECTS)
def test_injected_defect_is_reported(defect):
    c = BY_NAME[FIRST[defect]]
    for kind in ("int", "rand"):
        assert seg_standin(c, kind) == []
        assert seg_standin(c, kind, defect) == ["out"], kind


def test_combine_standin_and_defect():
    for c in COMB:
        for kind in ("int", "rand"):
            P = comb_problem(c, 5, kind)
            ref, bud = combine_math(P)
            got, _ = combine_math(P, torch.float32)
            bad, _ = combine_math(P, torch.float32, defect="last_piece_left_out")
            if kind == "int":
                assert compare_exact(got, ref, ["buf"]) == [] and compare_exact(bad, ref, ["buf"]) == ["buf"]
            else:
                assert compare_bounded(got, ref, bud) == [] and compare_bounded(bad, ref, bud) == ["buf"]
        assert c.width % {3: 64, 64: 64, 130: 128, 300: 256}[c.width] != 0 or c.width == 64
        assert set(int(d) for d in P.dst).isdisjoint(int(s) for s in P.src) != c.in_place


def test_refusals():
    lib = L.load()
    a = 0x10000   # placeholder addresses: refused before anything is read or launched
    assert lib.nlam_segment_sum_bf16(a, 0, a, None, None, a, 4, 12, 1, None) == EUNSUP     # width no multiple of 8
    assert lib.nlam_segment_sum_bf16(a, 0, a, None, None, a, 4, 4, 1, None) == EINVAL
    assert lib.nlam_segment_sum_bf16(None, 0, a, None, None, a, 4, 8, 1, None) == EINVAL
    assert lib.nlam_segment_sum(a, 0, None, None, None, a, 4, 8, 1, None) == EINVAL
    assert lib.nlam_segment_sum(a, 0, a, None, None, a, -1, 8, 1, None) == EINVAL
    assert lib.nlam_segment_sum_acc(a, 0, a, None, None, a, 4, 0, 1, None) == EINVAL
    assert lib.nlam_segment_sum_add(a, 0, a, None, None, None, a, 4, 8, 1, None) == EINVAL   # _add without extra
    assert lib.nlam_split_combine(a, 0, a, a, None, 1, 8, 1, None) == EINVAL
    assert lib.nlam_split_combine(a, 0, a, a, a, 1, 8, 65536, None) == EUNSUP
    for f in (lib.nlam_segment_sum, lib.nlam_segment_sum_acc, lib.nlam_segment_sum_bf16):
        assert f(a, 0, a, None, None, a, 0, 8, 1, None) == 0                                  # nseg == 0: nothing to do
    assert lib.nlam_split_combine(a, 0, a, a, a, 0, 8, 1, None) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def upload(P):
    c = P.case
    dev = Bufs()
    nb = P.inp.shape[0]
    if c.entry == "bf16":
        flat = torch.full((nb, max(P.in_bstride, P.rows * c.width)), 0x7FC0, dtype=torch.int16)   # NaN between the batch items
        flat[:, : P.rows * c.width] = bf16_bits(P.inp).reshape(nb, -1)
        dev.put("in", flat, torch.int16)
    else:
        flat = torch.full((nb, max(P.in_bstride, P.rows * c.width)), float("nan"), dtype=torch.float64)
        flat[:, : P.rows * c.width] = P.inp.reshape(nb, -1)
        dev.put("in", flat)
    dev.put("ptr", P.ptr, torch.int32)
    if P.order is not None:
        dev.put("order", P.order, torch.int32)
    if P.scale is not None:
        dev.put("scale", P.scale)
    dev.put("extra", P.extra)
    return dev


def launch(lib, P, dev, nseg=None):
    c = P.case
    out = dev.out("out", (c.batch, P.nseg, c.width))
    if c.entry in ("acc", "add"):
        out.copy_(P.prev.float())
    nseg = P.nseg if nseg is None else nseg
    head = (dev.addr("in"), P.in_bstride, dev.addr("ptr"), dev.addr("order"), dev.addr("scale"))
    tail = (dev.addr("out"), nseg, c.width, c.batch, _stream())
    if c.entry == "add":
        rc = lib.nlam_segment_sum_add(*head, dev.addr("extra"), *tail)
    else:
        rc = {"sum": lib.nlam_segment_sum, "acc": lib.nlam_segment_sum_acc, "bf16": lib.nlam_segment_sum_bf16}[c.entry](*head, *tail)
    assert rc == 0
    torch.cuda.synchronize()
    assert dev.guards_intact() == []
    return {"out": dev.t["out"].cpu()}


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_segment_sum_tiers(lib, case):
    for kind in ("int", "rand"):
        if {"int": "a", "rand": "b"}[kind] not in case.tiers:
            continue
        P = seg_problem(case, 2, kind)
        ref, bud = segsum_math(P)
        dev = upload(P)
        got = launch(lib, P, dev)
        if kind == "int":
            assert compare_exact(got, ref, ["out"]) == [], "tier (a)"
            assert torch.equal(launch(lib, P, dev)["out"], got["out"]), "two launches differ"
        else:
            note = lambda name, ratio: _RATIOS.__setitem__(KERNEL[case.groups], max(_RATIOS.get(KERNEL[case.groups], 0.0), float(ratio)))
            bad = compare_bounded(got, ref, bud, note=note)
            print(f"{case}: largest |got - R| / bound so far for {KERNEL[case.groups]}: {_RATIOS[KERNEL[case.groups]]:.3f}")
            assert bad == [], "tier (b)"
            assert torch.equal(launch(lib, P, dev)["out"], got["out"]), "two launches differ"


@gpu
@pytest.mark.parametrize("case", COMB, ids=str)
def test_split_combine_tiers(lib, case):
    for kind in ("int", "rand"):
        P = comb_problem(case, 3, kind)
        ref, bud = combine_math(P)
        runs = []
        for _ in range(2):
            dev = Bufs()
            buf = dev.out("buf", (case.batch, P.bstride))
            buf[:, : P.nrows * case.width] = P.buf.float().reshape(case.batch, -1).cuda()
            for n, t in (("ptr", P.ptr), ("src", P.src), ("dst", P.dst)):
                dev.put(n, t, torch.int32)
            assert lib.nlam_split_combine(dev.addr("buf"), P.bstride, dev.addr("ptr"), dev.addr("src"), dev.addr("dst"), P.n, case.width,
                                          case.batch, _stream()) == 0
            torch.cuda.synchronize()
            full = dev.t["buf"].cpu()
            assert dev.guards_intact() == [] and bool(torch.isnan(full[:, P.nrows * case.width:]).all()), "written between the batch items"
            runs.append({"buf": full[:, : P.nrows * case.width].reshape(case.batch, P.nrows, case.width)})
        assert torch.equal(runs[0]["buf"], runs[1]["buf"]), "two launches differ"
        if kind == "int":
            assert compare_exact(runs[0], ref, ["buf"]) == []
        else:
            note = lambda name, ratio: _RATIOS.__setitem__("split_combine_kernel", max(_RATIOS.get("split_combine_kernel", 0.0), float(ratio)))
            assert compare_bounded(runs[0], ref, bud, note=note) == []


@gpu
def test_launch_without_segments(lib):
    for name in ("plain_w64", "split4_add", "bf16_w64"):
        P = seg_problem(BY_NAME[name], 4, "int")
        dev = upload(P)
        keep = P.prev.float() if P.case.entry == "add" else None
        got = launch(lib, P, dev, nseg=0)["out"]
        assert torch.equal(got, keep) if keep is not None else bool(torch.isnan(got).all())
