"""Kernel-level checks of the window-moments kernels (moments_partials_kernel<DIFF, T>, moments_finish_kernel of
csrc/nlam_stats.inc) through the C entry points nlam_window_moments and nlam_window_moments_q16, row by row against the exact
float64 math of moments_ref.py.  The (nodes, nvars) geometries sit at the edges of mom_split and of the two kernels' segments: one
partial chunk with a dead lane, a second span of 5, 17 and 7 elements, a row that ends on a chunk end, nvars = 1, 100, 129 and
256 (G = 1, once by the clamp), 256 spans of one chunk and 129 spans of two; each states the nslot, span, lanes, G and segment
lengths it is built for.  Every small geometry runs on a quad boundary and one element off it, in both modes and both element
types; the layouts (overlapping analysis samples, forecast members, a shared member series, odd strides, row_begin, one row) and
the difference strides (1, 2, 3, 4 with an unread ninth row, exactly one pair, a ramp that tells a pair across sub-offsets from
one within) run on a one-span and a two-span geometry.  The series lies in a NaN-filled allocation (code -32768 for a packed one);
out_mean, out_sq and the workspace, sized exactly, are NaN-filled between NaN guards, and every output must be finite.
  (a) exact: integer data in [-8, 8], integer mean, std in {0.5, 1, 2, 4}, integer decode tables: every sum is exact in fp64 and
      an output carries the bits of float64(sum) / float64(count);
  (b) random data around offsets up to 250: |got - R| <= depth * 2^-53 * sum |term| / count + 2^-53 |R| element by element, R the
      exact quotient, depth derived in moments_ref.py from the addition chains of the two kernels.
Identities, bit for bit: two launches; the rows of [0, n) against launches over [first, first + count); the packed entry against
the fp32 entry on the decoded series.  Without a GPU: the geometry each case is built for, the numpy stand-in of the kernel pair
passing both tiers, nine injected defects reported, the refusals of both entries."""
import ctypes as C
import dataclasses
import json
import os
import time

import numpy as np
import pytest
import torch

from neural_lam_amd import _lib as L

import moments_ref as M
from moments_ref import MOM_DEFECTS, MomCase, Out, compare_bounded, compare_exact, mom_geometry, mom_problem, moments_math, put, standin_check
from test_standardization_stats import OFFSETS

gpu = pytest.mark.gpu
EINVAL, EUNSUP = -1, -2
_RATIOS = {}      # kernel instantiation -> largest |got - R| / bound over the tier-(b) runs

# (nodes, nvars) -> nslot, span in chunks, mom_lanes, G, seglen of the partials kernel, seglen of the finish, elements of the last span
GEOM = {
    (37, 5): (1, 1, 255, 25, 9, 1, 185),          # one partial chunk, lane 255 dead, 185 = 46 quads + 1
    (33, 17): (1, 1, 255, 7, 9, 1, 561),
    (409, 5): (2, 1, 255, 25, 9, 1, 5),           # the second span: one whole quad and one element
    (121, 17): (2, 1, 255, 7, 9, 1, 17),
    (288, 7): (1, 1, 252, 18, 8, 1, 2016),        # W = 1008: e1 on the chunk end
    (289, 7): (2, 1, 252, 18, 8, 1, 7),
    (2049, 1): (2, 1, 256, 128, 8, 1, 1),         # R = 1024
    (9, 256): (2, 1, 256, 1, 4, 2, 256),          # 512 columns on 256 threads
    (17, 129): (3, 1, 129, 1, 4, 3, 129),         # 256 / 258 = 0, clamped to G = 1
    (21, 100): (2, 1, 200, 1, 8, 2, 500),         # R = 8
    (131072, 4): (256, 1, 256, 32, 8, 8, 2048),   # a span of one chunk
    (131073, 4): (129, 2, 256, 32, 8, 5, 4),      # a span of two chunks; finish segments 26 ... 31 are empty
}
SMALL = [g for g in GEOM if g[0] * g[1] < 100000]
ONE_SPAN, TWO_SPANS = (37, 5), (409, 5)

CASES = []
for (n_, f_) in SMALL:       # every small geometry: both element types, both modes, on a quad boundary and one element off it
    for elem in ("f32", "q16"):
        for off in (0, 1):
            CASES += [MomCase(f"g{n_}x{f_}_values_{elem}_off{off}", n_, f_, nbase=2, elem=elem, off=off),
                      MomCase(f"g{n_}x{f_}_diff_{elem}_off{off}", n_, f_, step=1, nbase=2, elem=elem, off=off)]
for (n_, f_) in ((131072, 4), (131073, 4)):
    for elem in ("f32", "q16"):
        CASES += [MomCase(f"g{n_}x{f_}_values_{elem}", n_, f_, nrows=2, nbase=1, elem=elem),
                  MomCase(f"g{n_}x{f_}_diff_{elem}", n_, f_, step=2, nrows=4, nbase=1, elem=elem)]
for (n_, f_) in (ONE_SPAN, TWO_SPANS):
    g_ = f"g{n_}x{f_}"
    for elem in ("f32", "q16"):
        CASES += [
            MomCase(f"{g_}_odd_step_values_{elem}", n_, f_, nrows=4, elem=elem, odd_step=True),
            MomCase(f"{g_}_odd_step_diff_{elem}", n_, f_, step=1, nrows=4, elem=elem, odd_step=True),
            MomCase(f"{g_}_members_values_{elem}", n_, f_, nrows=9, row_begin=2, layout="forecast", nbase=2, members=2, elem=elem, off=1,
                    odd_member=True),
            MomCase(f"{g_}_members_diff_{elem}", n_, f_, step=2, nrows=9, layout="forecast", nbase=2, members=2, elem=elem, off=1,
                    odd_member=True),
            MomCase(f"{g_}_shared_values_{elem}", n_, f_, nrows=9, layout="shared", nbase=2, members=3, elem=elem),
        ]
    CASES += [
        MomCase(f"{g_}_one_row", n_, f_, nrows=1),
        MomCase(f"{g_}_row_begin_2", n_, f_, nrows=9, row_begin=2),
        MomCase(f"{g_}_shared_diff", n_, f_, step=3, nrows=9, row_begin=2, layout="shared", nbase=2, members=3),
        MomCase(f"{g_}_step1", n_, f_, step=1, nrows=9),
        MomCase(f"{g_}_step2", n_, f_, step=2, nrows=9, row_begin=2),
        MomCase(f"{g_}_step3", n_, f_, step=3, nrows=9),
        MomCase(f"{g_}_step4_ninth_row_unread", n_, f_, step=4, nrows=9, layout="forecast", nbase=2, members=2),   # lead 8 is NaN
        MomCase(f"{g_}_one_pair_step3", n_, f_, step=3, nrows=6),
        MomCase(f"{g_}_one_pair_step1", n_, f_, step=1, nrows=2),
        MomCase(f"{g_}_ramp_step2", n_, f_, step=2, nrows=9, data="ramp"),
        MomCase(f"{g_}_ramp_step2_q16", n_, f_, step=2, nrows=8, data="ramp", elem="q16", off=1),
    ]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SEED = {c.name: 100 + i for i, c in enumerate(CASES)}


def kernel_of(c):
    return f"moments_partials_kernel<{'true' if c.step else 'false'}, {'float' if c.elem == 'f32' else 'int16_t'}>"


def _note(c):
    def note(name, ratio):
        keys = [kernel_of(c)] + (["moments_finish_kernel"] if GEOM[(c.nodes, c.nvars)][0] > 1 else [])   # the finish adds 2+ partials
        for k in keys:
            _RATIOS[k] = max(_RATIOS.get(k, 0.0), float(ratio))
    return note


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib = L.load()
    t0 = time.time()
    yield lib
    for k, v in sorted(_RATIOS.items()):
        print(f"largest |got - R| / bound: {k:48s} {v:.3f}")
    path = os.environ.get("NLAM_MOMENTS_REPORT")
    if path and _RATIOS:
        rep = {"wall_seconds": round(time.time() - t0, 2), "ratios": [{"kernel": k, "max_ratio": round(v, 4)} for k, v in sorted(_RATIOS.items())]}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_cases_take_the_geometry_they_are_built_for():
    lib = L.load()
    assert M.OFFSETS == OFFSETS and max(OFFSETS) == 250.0
    assert (M.THREADS, M.QUADS, M.SLOTS) == (256, 2, 256)
    for (nodes, nvars), (nslot, span, lanes, G, seglen, fseglen, last) in GEOM.items():
        g = mom_geometry(nodes, nvars)
        assert (g.nslot, g.span_chunks, g.lanes, g.G, g.seglen, g.fseglen) == (nslot, span, lanes, G, seglen, fseglen), (nodes, nvars)
        assert g.per_row - (nslot - 1) * g.span == last and g.chunk == 8 * lanes and g.R * nvars == g.W
        assert 2 * nvars * G <= 2 * 256, "the LDS segment table of both kernels"
        # the C mom_split answers the same: the workspace is nslot * 2 * nvars doubles per output row
        assert lib.nlam_moments_workspace_doubles(nodes, nvars, 1, 0) == nslot * 2 * nvars
        assert lib.nlam_moments_workspace_doubles(nodes, nvars, 3, 2) == 6 * nslot * 2 * nvars
    assert GEOM[(37, 5)][2] == 255 and 185 % 4 == 1 and 561 % 4 == 1                      # a dead lane; totals off a quad
    assert 256 // (2 * 129) == 0 and 256 // (2 * 256) == 0 and 256 // (2 * 100) == 1       # G by the clamp, and G = 1 without it
    assert -(-129 // 5) == 26 < 32                                                         # the finish of 129 partials: empty segments
    assert {(c.nodes, c.nvars) for c in CASES} == set(GEOM)
    for c in CASES:
        ss, st, sm, total = c.strides()
        n_times, steps, n_flat = c.sizes()
        B = c.nodes * c.nvars
        assert st > B and (c.layout != "forecast" or sm > steps * st) and n_flat >= 1
        rows = {(c.off + m * sm + j * st) % 4 for m in range(c.members) for j in range(c.row_begin, c.row_begin + c.nrows)}
        if c.odd_step or c.odd_member:
            assert 0 in rows and len(rows) > 1, f"{c}: rows on and off a quad boundary"
        else:
            assert rows == {c.off}, c.name
        if c.step:
            assert c.nsub >= 2
        assert 0 <= M.depth_of(c) <= max(c.count - 1, 0)
        if B <= 2100 and c.name.endswith(("_off0", "_off1")):
            assert BY_NAME[c.name[:-1] + "0"].off == 0 and BY_NAME[c.name[:-1] + "1"].off == 1
    for g_ in ("g37x5", "g409x5"):
        c = BY_NAME[f"{g_}_step4_ninth_row_unread"]
        assert c.used == 8 and c.nrows == 9 and c.forecast
        P = mom_problem(c, 1, "int")
        assert int(np.isnan(P.flat).sum()) > 2 * 2 * 2 * c.nodes * c.nvars     # leads 8 and 9 of every (time, member) are NaN
        assert BY_NAME[f"{g_}_one_pair_step3"].nsub == 2 and BY_NAME[f"{g_}_one_pair_step1"].nsub == 2
    # the derived depth per family: lane adds + LDS segment + segments + finish segment + finish segments, each n - 1
    assert M.depth_of(BY_NAME["g409x5_values_f32_off0"]) == (2 * 3 - 1) + 8 + 22 + 0 + 1
    assert M.depth_of(BY_NAME["g131073x4_values_f32"]) == (2 * 2 * 2 - 1) + 7 + 31 + 4 + 25
    assert M.depth_of(BY_NAME["g131072x4_diff_f32"]) == (2 * 1 - 1) + 7 + 31 + 7 + 31
    assert M.depth_of(BY_NAME["g37x5_one_row"]) == (2 * 1 - 1) + 8 + 22 + 0 + 0 <= 37 - 1


STANDIN = ("g37x5_values_f32_off0", "g33x17_diff_f32_off1", "g409x5_values_q16_off1", "g121x17_diff_q16_off0", "g288x7_values_f32_off0",
           "g289x7_diff_f32_off0", "g2049x1_values_f32_off1", "g9x256_values_q16_off0", "g17x129_diff_f32_off0", "g21x100_values_f32_off1",
           "g409x5_members_diff_q16", "g37x5_members_values_f32", "g409x5_shared_diff", "g37x5_step4_ninth_row_unread",
           "g409x5_odd_step_diff_f32", "g409x5_ramp_step2", "g37x5_one_pair_step3", "g37x5_one_row")


@pytest.mark.parametrize("name", STANDIN)
def test_standin_passes_both_tiers(name):
    assert standin_check(BY_NAME[name], "int") == [] and standin_check(BY_NAME[name], "rand") == []


def test_standin_of_the_two_chunk_span():
    """131073 x 4 once: the lane's second chunk, 129 partials in finish segments of 5."""
    c = dataclasses.replace(BY_NAME["g131073x4_values_f32"], nrows=1)
    assert standin_check(c, "int") == []


# defect -> (the case that reports it, the tiers that can)
FIRST = {
    "last_partial_quad_dropped": ("g37x5_values_f32_off0", ("int", "rand")),
    "last_span_skipped": ("g409x5_values_f32_off0", ("int", "rand")),
    "span_end_not_clamped": ("g37x5_values_q16_off1", ("int", "rand")),
    "features_of_256_lanes": ("g409x5_values_f32_off0", ("int", "rand")),
    "zp_carried_over_sub_offsets": ("g409x5_ramp_step2", ("int", "rand")),
    "first_row_difference_counted": ("g37x5_step1", ("int", "rand")),
    "count_without_minus_one": ("g409x5_one_pair_step3", ("int", "rand")),
    "finish_one_partial_short": ("g289x7_values_f32_off0", ("int", "rand")),
    "decode_fused": ("g37x5_values_q16_off0", ("rand",)),       # integer tables decode alike fused or not: tier (b) on packed data
}


@pytest.mark.parametrize("defect", MOM_DEFECTS)
def test_injected_defect_is_reported(defect):
    name, kinds = FIRST[defect]
    for kind in kinds:
        assert standin_check(BY_NAME[name], kind) == []
        assert standin_check(BY_NAME[name], kind, defect) != [], kind
    if defect == "span_end_not_clamped":    # and the fp32 series: the NaN gap behind the block
        assert standin_check(BY_NAME["g409x5_values_f32_off0"], "int", defect) == ["mean", "sq"]
    if defect == "zp_carried_over_sub_offsets":   # the ramp: the crossing pair is far from the pairs within a sub-offset
        P = mom_problem(BY_NAME[name], 5, "rand")
        got, bad = M.standin(P), M.standin(P, defect=defect)
        assert np.array_equal(got["mean"][0::2], bad["mean"][0::2])           # sub-offset 0 has no predecessor
        assert float(np.abs(got["mean"][1::2] - bad["mean"][1::2]).min()) > 0.1 * float(np.abs(got["mean"][1::2]).min())


def _fake_moments(**kw):
    fake = 0x10000   # placeholder addresses: refused before anything is read or launched
    p = L.Moments()
    p.series = p.workspace = p.out_mean = p.out_sq = fake
    p.workspace_doubles = 1 << 40
    p.stride_sample = p.stride_step = 185
    p.n_times, p.count, p.members, p.nodes, p.nvars, p.nrows = 16, 2, 1, 37, 5, 5
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_refusals():
    lib = L.load()
    fake = 0x10000
    entries = (lambda p: lib.nlam_window_moments(C.byref(p), None), lambda p: lib.nlam_window_moments_q16(C.byref(p), fake, fake, fake, None))
    short = lib.nlam_moments_workspace_doubles(37, 5, 2, 0) - 1
    short_diff = lib.nlam_moments_workspace_doubles(37, 5, 2, 2) - 1
    assert short == 2 * 10 - 1 and short_diff == 2 * 2 * 10 - 1
    for run in entries:
        for kw in (dict(step=1), dict(step=1, mean=fake), dict(step=1, std=fake),         # the difference mode without its statistics
                   dict(mean=fake, std=fake), dict(mean=fake), dict(std=fake),              # the values mode with them
                   dict(step=3, mean=fake, std=fake), dict(step=5, mean=fake, std=fake),    # nrows / step < 2: no pair
                   dict(first=11), dict(first=12, count=1), dict(count=13), dict(first=-1),  # 12 flat samples
                   dict(is_forecast=1, steps=5, first=15), dict(is_forecast=1, steps=5, members=2, first=31),
                   dict(workspace_doubles=short), dict(step=2, mean=fake, std=fake, workspace_doubles=short_diff),
                   dict(nrows=17), dict(row_begin=12), dict(workspace=None), dict(out_mean=None), dict(out_sq=None), dict(nodes=0),
                   dict(nrows=0), dict(members=0), dict(step=-1), dict(row_begin=-1), dict(is_forecast=2)):
            assert run(_fake_moments(**kw)) == EINVAL, kw
        assert run(_fake_moments(nvars=257)) == EUNSUP
        assert run(_fake_moments(nodes=(1 << 31) // 5 + 1)) == EUNSUP
    assert lib.nlam_window_moments(None, None) == EINVAL and lib.nlam_window_moments(C.byref(_fake_moments(series=None)), None) == EINVAL
    assert lib.nlam_moments_workspace_doubles(37, 257, 1, 0) == EINVAL and lib.nlam_moments_workspace_doubles(37, 256, 1, 0) == 5 * 512
    assert lib.nlam_moments_workspace_doubles(0, 5, 1, 0) == EINVAL and lib.nlam_moments_workspace_doubles(37, 5, 0, 0) == EINVAL
    assert lib.nlam_moments_workspace_doubles(37, 5, 1, -1) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def upload(P):
    d = {"flat": put(P.flat)}
    for n in ("mean", "std", "scale", "offset"):
        if getattr(P, n) is not None:
            d[n] = put(getattr(P, n))
    item = P.flat.dtype.itemsize
    assert d["flat"].data_ptr() % 16 == 0 and (d["flat"].data_ptr() + item * P.case.off) % (4 * item) == item * P.case.off
    return d


def launch(lib, P, d, first=0, count=None):
    """One launch over [first, first + count) -> {"mean", "sq"} (count * max(step, 1), nvars); guards and finiteness asserted."""
    c = P.case
    count = P.n_flat - first if count is None else count
    n_out, F = count * max(c.step, 1), c.nvars
    nws = lib.nlam_moments_workspace_doubles(c.nodes, F, count, c.step)
    assert nws == n_out * mom_geometry(c.nodes, F).nslot * 2 * F
    ws, om, osq = Out(nws), Out(n_out * F), Out(n_out * F)
    packed = P.flat.dtype == np.int16
    series = d["flat"].data_ptr() + P.flat.dtype.itemsize * c.off
    p = L.Moments()
    p.series = None if packed else series
    if c.step:
        p.mean, p.std = d["mean"].data_ptr(), d["std"].data_ptr()
    p.workspace, p.out_mean, p.out_sq, p.workspace_doubles = ws.ptr(), om.ptr(), osq.ptr(), nws
    p.stride_sample, p.stride_step, p.stride_member = P.stride_sample, P.stride_step, P.stride_member
    p.n_times, p.first, p.count = P.n_times, first, count
    p.is_forecast, p.members, p.steps = int(c.forecast), c.members, P.steps
    p.nodes, p.nvars, p.row_begin, p.nrows, p.step = c.nodes, F, c.row_begin, c.nrows, c.step
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if packed:
        rc = lib.nlam_window_moments_q16(C.byref(p), series, d["scale"].data_ptr(), d["offset"].data_ptr(), stream)
    else:
        rc = lib.nlam_window_moments(C.byref(p), stream)
    assert rc == 0
    torch.cuda.synchronize()
    ws.read()      # its guards
    got = {"mean": om.read().reshape(n_out, F), "sq": osq.read().reshape(n_out, F)}
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["sq"]).all(), "a NaN of the gaps or an unwritten element"
    return got


def same_bits(a, b):
    return all(np.array_equal(a[n].view(np.int64), b[n].view(np.int64)) for n in ("mean", "sq"))


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_moments_tiers(lib, case):
    for kind in ("int", "rand"):
        P = mom_problem(case, SEED[case.name], kind)
        ref = moments_math(P)
        d = upload(P)
        got = launch(lib, P, d)
        if kind == "int":
            assert compare_exact(got, ref) == [], "tier (a)"
        else:
            bad = compare_bounded(got, ref, note=_note(case))
            print(f"{case}: depth {M.depth_of(case)}, largest |got - R| / bound so far for {kernel_of(case)}: {_RATIOS[kernel_of(case)]:.3f}")
            assert bad == [], "tier (b)"
        assert same_bits(launch(lib, P, d), got), "two launches differ"


RANGES = ["g409x5_members_values_f32", "g409x5_members_diff_f32", "g409x5_members_values_q16", "g409x5_members_diff_q16",
          "g17x129_values_f32_off1", "g37x5_step3"]


@gpu
@pytest.mark.parametrize("name", RANGES)
def test_rows_do_not_depend_on_first_and_count(lib, name):
    c = dataclasses.replace(BY_NAME[name], nbase=3 if BY_NAME[name].forecast else 6)     # six flat samples
    P = mom_problem(c, 7, "rand")
    assert P.n_flat == 6
    d = upload(P)
    S = max(c.step, 1)
    full = launch(lib, P, d)
    for first, count in ((0, 1), (3, 1), (5, 1), (0, 3), (3, 3), (1, 4)):
        part = launch(lib, P, d, first, count)
        want = {n: full[n][first * S: (first + count) * S] for n in full}
        assert same_bits(part, want), (first, count)


PACKED = ["g37x5_values_q16_off0", "g37x5_diff_q16_off1", "g409x5_values_q16_off1", "g409x5_members_diff_q16", "g409x5_members_values_q16",
          "g9x256_diff_q16_off0", "g21x100_values_q16_off1", "g409x5_odd_step_diff_q16", "g131073x4_diff_q16"]


@gpu
@pytest.mark.parametrize("name", PACKED)
def test_packed_entry_gives_the_bits_of_the_fp32_entry_on_the_decoded_series(lib, name):
    for kind in ("int", "rand"):
        P = mom_problem(BY_NAME[name], 9, kind)
        Q = M.decoded_float_problem(P)
        got = launch(lib, P, upload(P))
        assert same_bits(got, launch(lib, Q, upload(Q))), kind
