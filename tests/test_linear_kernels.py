"""Kernel-level checks of nlam_linear (linear_bf_kernel<KB, MB, NS>, linear_bfw_kernel<NS>, linear_gemm_kernel<NS, WN, TA, SK>)
through the C entry point with hand-filled nlam_linear_t structs, against the float64 math of linear_segsum_ref.py.  The cases name
the SMALLEST shapes at which each edge exists -- one row, a ragged last tile, the second pass of a persistent loop, a second and
third round of the strip kernel with dead waves, an odd K-chunk count, row tiles of 64 and of 128 rows padded to groups of eight,
forward and transposed weights, a second product in the same launch -- and the nlam_linear_plan code each one is built for.
Every output is NaN-filled with NaN guard floats and PAD_ROWS NaN rows behind it; rows past `rows` must keep their NaN.
  (a) exact on integers in [-127, 127] (lin_headroom): bit-equal to float64 in every matrix mode, both outputs of a dual launch,
      accumulating on integer contents, and a second accumulating launch on top of a plain one gives exactly twice the product;
  (b) |got - R| <= (U (k + 2) + MODE_TERM[NS]) (|x| @ |A|^T) (+ U |R|) element by element, NS = the terms the plan says run;
  (c) three low-order probes, exact at any K: the weights carry three bf16 terms, the rows carry them, both carry two (the product
      of the two second terms) -- bit-equal to the value for the NS executed.
Identities, bit for bit: two launches; a dual launch and two single ones; rows == 0.
Without a GPU: the plan table, the default dispatch, the refusals (plan and launch answer alike), the stand-in passing the tiers,
eight injected defects reported, exactness of the probe expectations."""
import ctypes as C
import json
import os
import time

import pytest
import torch

from neural_lam_amd import _lib as L

from linear_segsum_ref import (CROSS_W, LIN_DEFECTS, LOW_W, PAD_ROWS, Bufs, LinCase, compare_bounded, compare_exact, describe_linear,
                               lin_headroom, lin_problem, lin_standin, linear_math, probe_reference, probe_value)
from mlp_kernel_ref import GRID_WAVES, _stream

gpu = pytest.mark.gpu
EINVAL, EUNSUP = -1, -2
GEMM_ALL, GEMM_OFF = ((L.TUNE_LIN_GEMM, 2),), ((L.TUNE_LIN_GEMM, 0),)
GEMM_128 = ((L.TUNE_LIN_GEMM, 128), (L.TUNE_LIN_GEMM, 2))     # a value above 2 sets the 128-row threshold AND mode 1: then mode 2
PROBES = ("low_w", "low_x", "cross")
_RATIOS = {}      # (kernel, terms executed) -> largest |got - R| / bound over the tier-(b) runs


def set_tuning(lib, pairs):
    for key, value in pairs:
        assert lib.nlam_set_tuning(key, value) == 0


def restore_tuning(lib):
    set_tuning(lib, ((L.TUNE_LIN_WGS, 256), (L.TUNE_LIN_GEMM, 32768), (L.TUNE_LIN_GEMM, 1)))


@pytest.fixture(scope="module")
def host():
    """The library for the host-only tests (plan codes and refusals: no launch)."""
    lib = L.load()
    restore_tuning(lib)
    yield lib
    restore_tuning(lib)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    lib = L.load()
    restore_tuning(lib)
    t0 = time.time()
    yield lib
    restore_tuning(lib)
    path = os.environ.get("NLAM_LINEAR_REPORT")
    if path and _RATIOS:
        rep = {"wall_seconds": round(time.time() - t0, 2),
               "ratios": [{"kernel": kn, "terms": ns, "max_ratio": v} for (kn, ns), v in sorted(_RATIOS.items())]}
        with open(path, "w") as f:
            json.dump(rep, f, indent=1)


# ---------------------------------------------------------------------------------------------------------------------------
# cases: name, (kernel the plan must answer), k, n, rows
# ---------------------------------------------------------------------------------------------------------------------------
BF, RES, STR = ("bf",), ("bfw", True), ("bfw", False)
CASES = []
for k_ in (32, 64):
    for n_ in (32, 64):
        # 1 row; a second, ragged tile; 2050 tiles for 2048 waves: the second pass of the persistent loop with its row prefetch
        CASES += [LinCase(f"bf_{k_}x{n_}_r{r_}", BF, k_, n_, r_) for r_ in (1, 33, 65569)]
CASES += [
    LinCase("bf_odd_column_offset", BF, 64, 64, 33, woff=1),                 # W + 4 bytes: the scalar staging path
    LinCase("bf_ldk2", BF, 32, 64, 33, layout="f2"),                         # every other column of a row of W
    LinCase("bf_transposed", BF, 64, 32, 33, layout="t"),                    # k != n, ldn = 1
    # the strip kernel: n % 128 != 0 (or NLAM_TUNE_LIN_GEMM = 0)
    LinCase("res_128x192_r1", RES, 128, 192, 1),
    LinCase("res_128x192_r65", RES, 128, 192, 65),
    LinCase("res_128x192_r300", RES, 128, 192, 300),                         # ten tiles: two workgroup columns, one with two live waves
    LinCase("res_192x64_r1", RES, 192, 64, 1),
    LinCase("res_192x64_r65", RES, 192, 64, 65, layout="t"),
    LinCase("res_192x64_r300", RES, 192, 64, 300),
    LinCase("str_320x192_r300", STR, 320, 192, 300),                         # KC = 5: the last chunk sits in buffer 0
    LinCase("str_512x448_r65", STR, 512, 448, 65),
    LinCase("str_320x192_r65_transposed", STR, 320, 192, 65, layout="t"),
    LinCase("res_dual_192x192_r300", RES, 192, 192, 300, dual=True),
    LinCase("res_misaligned_128x128_r65", RES, 128, 128, 65, woff=1),        # n % 128 == 0, but the GEMM cannot read W: must route here
    LinCase("res_misaligned_dual_64x128_r65", RES, 64, 128, 65, woff=3, dual=True),
    # three rounds on one workgroup column: the last with two live waves (one ragged tile) and six dead ones
    LinCase("res_three_rounds_128x192_r545", RES, 128, 192, 545, tune=((L.TUNE_LIN_WGS, 3),)),
    # 514 tiles on 64 workgroup columns of eight waves: two rounds of the streamed strip, both products
    LinCase("str_two_rounds_dual_320x512_r16417", STR, 320, 512, 16417, modes=(1, 3), dual=True, tune=GEMM_OFF),
    LinCase("str_wgs0_128x192_r65", STR, 128, 192, 65, tune=((L.TUNE_LIN_WGS, 0),)),   # k <= 256 streamed: NLAM_TUNE_LIN_WGS = 0
    # the LDS-tiled GEMM, both products of a launch: 64-row tiles (forced wherever it applies) and 128-row tiles
    LinCase("g64_dual_64x256_r577", ("gemm", 1, 4), 64, 256, 577, dual=True, tune=GEMM_ALL),
    LinCase("g64_dual_96x256_r65_t", ("gemm", 1, 2), 96, 256, 65, layout="t", dual=True, tune=GEMM_ALL),
    LinCase("g128_dual_320x256_r129", ("gemm", 2, 2), 320, 256, 129, dual=True, tune=GEMM_128),
    LinCase("g128_dual_64x256_r1153_t", ("gemm", 2, 2), 64, 256, 1153, layout="t", dual=True, tune=GEMM_128),
]
# single products: every K (one 64-column chunk; 96 = three 32-column chunks; five and eight chunks) in both layouts at both
# widths; the rows cycle through one row / two tiles / ten tiles padded to sixteen (64-row tiles: forced wherever the GEMM
# applies) and one full tile / a one-row second tile / ten tiles padded to sixteen (128-row tiles: the threshold lowered to 128)
for i_, (k_, lay_, n_) in enumerate((k_, lay_, n_) for k_ in (64, 96, 320, 512) for lay_ in "ft" for n_ in (128, 384)):
    r64, r128 = (1, 65, 577)[(i_ + i_ // 6) % 3], (128, 129, 1153)[(i_ + i_ // 6 + 1) % 3]
    suffix = "_t" if lay_ == "t" else ""
    CASES.append(LinCase(f"g64_{k_}x{n_}_r{r64}{suffix}", ("gemm", 1, 2 if k_ == 96 else 4), k_, n_, r64, layout=lay_, tune=GEMM_ALL))
    if (i_ + k_ // 64) % 2 == 0:   # half of them on 128-row tiles too: each K in both layouts
        CASES.append(LinCase(f"g128_{k_}x{n_}_r{r128}{suffix}", ("gemm", 2, 2), k_, n_, r128, layout=lay_, tune=GEMM_128))
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every instantiation nlam_linear can launch
REACHABLE = ({L.linp_bf(ns, kb, mb) for ns in (1, 2, 3) for kb in (1, 2) for mb in (1, 2)}
             | {L.linp_bfw(ns, res) & ~L.LINP_DUAL for ns in (1, 2, 3) for res in (True, False)}
             | {L.linp_gemm(ns, 2, 2, ta) for ns in (1, 2, 3) for ta in (False, True)}
             | {L.linp_gemm(ns, 1, 2, ta) for ns in (2, 3) for ta in (False, True)}
             | {L.linp_gemm(1, 1, sk, ta) for sk in (2, 4) for ta in (False, True)})


def fake_addr(case):
    """Placeholder addresses with the alignment of the real buffers (the plan reads nothing through them)."""
    table = {"x": 0x10000, "W": 0x20000, "W2": 0x30000, "out": 0x40000, "out2": 0x50000}
    return table.__getitem__


def plan_of(lib, case, ns):
    return lib.nlam_linear_plan(C.byref(describe_linear(case, ns, fake_addr(case))))


def test_case_table_hits_every_instantiation(host):
    assert host.nlam_grid_waves() == GRID_WAVES == 2048, "the 65 569-row cases are built for 2048 persistent waves"
    hit = {}
    for c in CASES:
        try:
            set_tuning(host, c.tune)
            for ns in c.modes:
                code = plan_of(host, c, ns)
                assert code == c.code(ns), f"{c} ns {ns}: plan {code:#x}, built for {c.code(ns):#x}"
                assert (code >> 2) & 3 == ns, "nlam_linear executes the terms that are requested"
                hit.setdefault(code & ~L.LINP_DUAL, []).append(c.name)
                if c.dual:
                    hit.setdefault(("dual", code & 3, bool(code & L.LINP_RESIDENT)), []).append(c.name)
        finally:
            restore_tuning(host)
    assert set(k for k in hit if isinstance(k, int)) == REACHABLE, sorted(REACHABLE ^ set(k for k in hit if isinstance(k, int)))
    assert len(REACHABLE) == 12 + 6 + 6 + 4 + 4
    for key in (("dual", L.LINP_BFW, True), ("dual", L.LINP_BFW, False), ("dual", L.LINP_GEMM, False)):
        assert key in hit, key
    # the GEMM's table: every K in both layouts and every row count in both layouts on either tile height, both widths and a dual one
    for wn, rows in ((1, (1, 65, 577)), (2, (128, 129, 1153))):
        g = [c for c in CASES if c.kernel[0] == "gemm" and c.kernel[1] == wn]
        assert {(c.k, c.layout) for c in g} == {(k, lay) for k in (64, 96, 320, 512) for lay in "ft"}
        assert {(c.rows, c.layout) for c in g} == {(r, lay) for r in rows for lay in "ft"}
        assert {c.n for c in g} == {128, 256, 384} and {c.layout for c in g if c.dual} == {"f", "t"}
    # the geometry the names promise
    assert -(-65569 // 32) == 2050 > GRID_WAVES
    assert -(-545 // 32) == 18 and 545 % 32 == 1            # rounds of 8 tiles on one workgroup column: 8, 8, 2
    assert -(-16417 // 32) == 514 and 4 * 256 // 16 == 64   # 64 columns x 8 waves = 512 tiles per round
    assert -(-577 // 64) == 10 == -(-1153 // 128)           # padded to 16: six workgroups per feature tile return at once


def test_default_dispatch_is_pinned(host):
    """NLAM_TUNE_LIN_GEMM = 1: the "where it wins" rule of the two workload row classes, by plan code only."""
    restore_tuning(host)
    for rows, kn, three_term_gemm in ((6561, 256, True), (6561, 512, False), (63784, 512, True), (63784, 256, False)):
        c = LinCase("d", ("gemm", 2 if rows >= 32768 else 1, 4), kn, kn, rows)
        strip = LinCase("d", ("bfw", kn <= 256), kn, kn, rows)
        for ns in (2, 3):
            assert plan_of(host, c, ns) == (c if three_term_gemm else strip).code(ns), (rows, kn, ns)
        assert plan_of(host, c, 1) == c.code(1), (rows, kn)
        # the transposed layout (the data gradient) follows the same rule
        ct = LinCase("d", c.kernel, kn, kn, rows, layout="t")
        assert plan_of(host, ct, 1) == ct.code(1) and bool(plan_of(host, ct, 1) & L.LINP_TA)


def test_refusals_plan_and_launch_agree(host):
    restore_tuning(host)
    base = BY_NAME["res_128x192_r65"]
    addr = fake_addr(base)

    def both(p, want):
        assert host.nlam_linear_plan(C.byref(p)) == want
        assert host.nlam_linear(C.byref(p), None) == want   # refused before anything is launched

    both(describe_linear(base, 0, addr), EUNSUP)                                   # the fp32-MFMA mode is not instantiated
    for k, n in ((48, 64), (64, 48), (100, 128)):
        both(describe_linear(LinCase("r", BF, k, n, 5), 3, addr), EUNSUP)          # k or n no multiple of 32
    for name in ("x", "out"):
        p = describe_linear(base, 3, addr)
        setattr(p, name, addr(name) + 4)
        both(p, EINVAL)
    p = describe_linear(base, 3, addr)
    p.W2 = addr("W2")
    both(p, EINVAL)                                                                # W2 without out2
    p = describe_linear(base, 3, addr)
    p.out2 = addr("out2")
    both(p, EINVAL)
    both(describe_linear(LinCase("r", BF, 64, 64, 5, dual=True), 3, addr), EUNSUP)  # the dual form exists above 64 only
    both(describe_linear(LinCase("r", BF, 96, 128, 5, woff=1), 3, addr), EUNSUP)   # only the GEMM takes k = 96, and it cannot read this W
    assert plan_of(host, LinCase("r", ("gemm", 1, 2), 96, 128, 5), 3) > 0
    for k, n in ((576, 128), (128, 576), (640, 640)):
        both(describe_linear(LinCase("r", BF, k, n, 5), 3, addr), EUNSUP)          # a width above 512
    for field in ("x", "W", "out"):
        p = describe_linear(base, 3, addr)
        setattr(p, field, None)
        both(p, EINVAL)
    p = describe_linear(base, 3, addr)
    p.rows = -1
    both(p, EINVAL)
    p.rows = 0
    assert host.nlam_linear_plan(C.byref(p)) == L.LINP_EMPTY and host.nlam_linear(C.byref(p), None) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the checker's own test: the stand-in passes, each defect is reported
# ---------------------------------------------------------------------------------------------------------------------------
STANDIN = ("bf_32x64_r33", "bf_ldk2", "bf_transposed", "res_192x64_r65", "res_dual_192x192_r300", "g64_96x128_r65", "g128_dual_320x256_r129")


@pytest.mark.parametrize("name", STANDIN)
def test_standin_passes_the_tiers(name):
    c = BY_NAME[name]
    for ns in c.modes:
        assert lin_standin(c, "int", ns) == [] and lin_standin(c, "int", ns, accumulate=True) == []
        assert lin_standin(c, "rand", ns) == [] and lin_standin(c, "rand", ns, accumulate=True) == []
        for kind in PROBES:
            assert lin_standin(c, kind, ns) == [], (kind, ns)


# defect -> (case, tier, terms, accumulate, the outputs that must be reported)
FIRST = {
    "ragged_last_row_from_neighbour": ("bf_32x64_r33", "int", 3, False, ["out"]),
    "out2_from_first_weights": ("res_dual_192x192_r300", "int", 3, False, ["out2"]),
    "accumulate_overwrites": ("g64_96x128_r65", "int", 1, True, ["out"]),
    "skip_last_k_chunk": ("g64_96x128_r65", "int", 2, False, ["out"]),
    "swap_ldn_ldk": ("bf_transposed", "int", 3, False, ["out"]),
    "drop_third_term": ("res_192x64_r65", "low_w", 3, False, ["out"]),
    "drop_second_terms_product": ("g128_dual_320x256_r129", "cross", 3, False, ["out", "out2"]),
    "skip_padding_group_row_tile": ("g64_dual_64x256_r577", "int", 3, False, ["out", "out2"]),
}


@pytest.mark.parametrize("defect", LIN_DEFECTS)
def test_injected_defect_is_reported(defect):
    name, kind, ns, acc, want = FIRST[defect]
    c = BY_NAME[name]
    assert lin_standin(c, kind, ns, accumulate=acc) == []
    assert lin_standin(c, kind, ns, defect=defect, accumulate=acc) == want
    if kind == "int":   # and the bounded tier sees it too
        assert lin_standin(c, "rand", ns, defect=defect, accumulate=acc) == want
    if defect == "drop_third_term":   # the rows' third term is probed on its own; one norm over the tensor would not see either
        assert lin_standin(c, "low_x", ns, defect=defect) == want
        assert lin_standin(c, "int", ns, defect=defect) == [], "integers of 8 bits are one term: tier (a) cannot see a dropped term"


def test_probe_expectations_are_exact():
    """Derived from the bf16 terms in float64: LOW_W = 1 + 2^-9 + 2^-18 is its own three terms, CROSS_W = 1 + 2^-9 its own two."""
    for kind in ("low_w", "low_x"):
        assert [probe_value(kind, ns) for ns in (1, 2, 3)] == [1.0, 1.0 + 2.0 ** -9, LOW_W]
    assert [probe_value("cross", ns) for ns in (1, 2, 3)] == [1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -18]
    assert probe_value("cross", 3) == CROSS_W * CROSS_W
    for name in ("bf_32x32_r33", "str_512x448_r65", "g64_dual_96x256_r65_t"):
        for kind in PROBES:
            P = lin_problem(BY_NAME[name], 3, kind)
            assert int((P.x != 0).sum(1).max()) <= 16 and int((P.x != 0).sum(0).min()) >= 1, "every column of K is hit by some row"
            for ns in (1, 2, 3):
                ref = probe_reference(P, ns)
                exact, _ = linear_math(P, ns=ns)
                if ns == 3:   # three terms hold the operands: the float64 product itself
                    assert compare_exact(ref, exact, list(exact)) == []
    assert all(lin_headroom(c) == 127 for c in CASES)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def upload(P):
    c = P.case
    dev = Bufs()
    dev.put("x", P.x)
    dev.put("W", P.W)
    dev.put("W2", P.W2)
    return dev


def launch(lib, P, dev, ns, prev=False, accumulate=False, dual=None, tag=""):
    """One nlam_linear launch into fresh NaN-filled guarded outputs (pre-filled with P.prev when asked) -> {out, out2} on the host."""
    c = P.case
    dual = c.dual if dual is None else dual
    names = ["out"] + (["out2"] if dual else [])
    for nme in names:
        t = dev.out(nme + tag, (c.rows + PAD_ROWS, c.n))
        if prev:
            t[: c.rows] = (P.prev if nme == "out" else P.prev2).float().cuda()
    addr = lambda nme: dev.addr(nme + tag) if nme.startswith("out") else dev.addr(nme)
    p = describe_linear(c, ns, addr, accumulate=accumulate, dual=dual)
    assert lib.nlam_linear(C.byref(p), _stream()) == 0
    return p, names


def collect(dev, c, names, tag=""):
    torch.cuda.synchronize()
    res = {}
    for nme in names:
        full = dev.t[nme + tag].cpu()
        assert bool(torch.isnan(full[c.rows:]).all()), f"{nme}: rows past the end were written"
        res[nme] = full[: c.rows]
    assert dev.guards_intact() == []
    return res


def run(lib, P, ns, prev=False, accumulate=False, dual=None, W_swap=False):
    dev = upload(P)
    if W_swap:   # the second product as a single launch
        dev.t["W"] = dev.t["W2"]
    _, names = launch(lib, P, dev, ns, prev, accumulate, dual)
    return collect(dev, P.case, names)


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_exact_on_integers(lib, case):
    P = lin_problem(case, 1, "int")
    ref, _ = linear_math(P)
    ref_acc, _ = linear_math(P, accumulate=True)   # (the products are computed once per problem)
    twice = {n: 2 * v for n, v in ref.items()}
    try:
        set_tuning(lib, case.tune)
        for ns in case.modes:
            assert lib.nlam_linear_plan(C.byref(describe_linear(case, ns, fake_addr(case)))) == case.code(ns)
            got = run(lib, P, ns)
            assert compare_exact(got, ref, list(ref)) == [], f"ns {ns}"
            assert compare_exact(run(lib, P, ns, prev=True, accumulate=True), ref_acc, list(ref)) == [], f"ns {ns}: accumulate"
            # a second, accumulating launch on top of the first: exactly twice; the first launch's outputs twice: bit-equal
            dev = upload(P)
            p, names = launch(lib, P, dev, ns)
            first = {n: v.clone() for n, v in collect(dev, case, names).items()}
            assert all(torch.equal(first[n], got[n]) for n in names), f"ns {ns}: two launches differ"
            p.accumulate = 1
            assert lib.nlam_linear(C.byref(p), _stream()) == 0
            assert compare_exact(collect(dev, case, names), twice, list(ref)) == [], f"ns {ns}: accumulate on top of a launch"
            if case.dual:   # the two products as single launches
                assert torch.equal(run(lib, P, ns, dual=False)["out"], got["out"])
                assert torch.equal(run(lib, P, ns, dual=False, W_swap=True)["out"], got["out2"])
    finally:
        restore_tuning(lib)


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_elementwise_error_budget(lib, case):
    P = lin_problem(case, 2, "rand")
    try:
        set_tuning(lib, case.tune)
        for ns in case.modes:
            ex = (lib.nlam_linear_plan(C.byref(describe_linear(case, ns, fake_addr(case)))) >> 2) & 3
            key = (case.kernel[0], ex)
            note = lambda name, ratio, key=key: _RATIOS.__setitem__(key, max(_RATIOS.get(key, 0.0), float(ratio)))
            for acc in (False, True):
                ref, bud = linear_math(P, ns=ex, accumulate=acc)
                got = run(lib, P, ns, prev=acc, accumulate=acc)
                bad = compare_bounded(got, ref, bud, note=note)
                print(f"{case} ns {ns} accumulate {acc}: largest |got - R| / bound so far for {key}: {_RATIOS[key]:.3f}")
                assert bad == [], f"ns {ns} accumulate {acc}"
                if not acc:
                    plain = got
            if case.dual:   # bit for bit the two products as single launches
                assert torch.equal(run(lib, P, ns, dual=False)["out"], plain["out"]), f"ns {ns}: dual out"
                assert torch.equal(run(lib, P, ns, dual=False, W_swap=True)["out"], plain["out2"]), f"ns {ns}: dual out2"
    finally:
        restore_tuning(lib)


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_low_order_probes(lib, case):
    try:
        set_tuning(lib, case.tune)
        for kind in PROBES:
            P = lin_problem(case, 3, kind)
            for ns in case.modes:
                ex = (lib.nlam_linear_plan(C.byref(describe_linear(case, ns, fake_addr(case)))) >> 2) & 3
                ref = probe_reference(P, ex)
                assert compare_exact(run(lib, P, ns), ref, list(ref)) == [], f"{kind} ns {ns}"
    finally:
        restore_tuning(lib)


@gpu
def test_launch_without_rows(lib):
    for name in ("bf_32x64_r33", "res_dual_192x192_r300", "g64_96x128_r65"):
        c = BY_NAME[name]
        P = lin_problem(c, 4, "int")
        dev = upload(P)
        names = ["out"] + (["out2"] if c.dual else [])
        for nme in names:
            dev.out(nme, (c.rows + PAD_ROWS, c.n))
        p = describe_linear(c, 3, dev.addr)
        p.rows = 0
        assert lib.nlam_linear_plan(C.byref(p)) == L.LINP_EMPTY
        assert lib.nlam_linear(C.byref(p), _stream()) == 0
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(dev.t[nme]).all()) for nme in names) and dev.guards_intact() == []
