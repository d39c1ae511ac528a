"""The kernels of the forecast path where they stop being one workgroup: the chunk reductions (forecast_tail / forecast_finish,
ens_scores / ens_finish, ens_products / ens_products_finish, the counting and finishing passes of nlam_ens_neighbourhood) at
C = 4, 5, 9 and 37 chunks per item -- every wave of a finisher holding a chunk, a short and an empty wave, an unrolled body with a
remainder --, the second lane round of forecast_finish_kernel, and the grid-stride loops past their block caps
(nlam_philox_normal_fill past 4096 blocks, nlam_latent_sample past 1024 blocks per item, the data rows of nlam_series.inc past 512
blocks of 2048 elements).  The references, launch helpers and budgets are those of the per-feature suites; the chunk size is read
off the public workspace queries.

Without a GPU: numpy fp32 stand-ins of the finishers' order (tests/forecast_scale_ref.py) stay inside the budgets at every shape,
every injected defect is reported by the comparison the GPU tests make, the wave and unroll defects are NOT reported at the
shapes the older suites stop at, and every case reaches the regime it is named for.  The largest error / budget per kernel and
output is printed, and written to the path NLAM_FORECAST_SCALE_REPORT names (profiles/forecast_scale_tests records one run)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import forecast_ref as FR
import forecast_scale_ref as S
import neighbourhood_ref as NR
import packed_ref as Q
import philox_ref as P
import test_ensemble_forecast as EF
import test_ensemble_neighbourhood as EN
import test_ensemble_products as EP
import test_forecast as TF
import test_packed_series as PS
from neural_lam_amd import _lib as L
from oracle import data as od
from tail_ref import Out, put

EPS32 = 2.0 ** -23
CHUNKS = [4, 5, 9, 37]
OLD_CHUNKS = [1, 2, 3]                 # what the per-feature suites reach
TAIL_FB = [(17, 3), (16, 2)]           # (F, batch): 102 sums, two lane rounds with the second partial; exactly 64 sums
TAIL_OPTIONS = [(False, False, False), (True, False, True), (False, True, True), (True, True, False)]   # clamp, std head, misaligned
F_ENS = 17
SCORE_CASES = [(3, 4), (3, 5), (3, 9), (3, 37), (1, 5), (1, 37), (64, 5), (64, 37)]   # (M, C)
PRODUCT_CASES = [(3, 5), (3, 37), (64, 5), (64, 37)]
PRODUCT_EQ = (4, 3)                    # events, quantiles
NBR_CASES = [(129, 128, 3), (95, 94, 17)]   # (nx, ny, F)
NBR_MEMBERS = [1, 5]
FILL_N = 4096 * 1024 + 4099
FILL_SEED, FILL_COUNTER = 0x9E3779B97F4A7C15, (5, 2, 0xFFFFFFF0)
LATENT_SHAPES = [(300, 7), (16401, 64)]

WORST = {}


def _note(kernel, quantity, ratio):
    key = (kernel, quantity)
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not WORST:
        return
    rows = [{"kernel": k, "quantity": q, "ratio": round(v, 4)} for (k, q), v in sorted(WORST.items())]
    for r in rows:
        print(f"largest error / budget: {r['kernel']:28s} {r['quantity']:14s} {r['ratio']:.3f}")
    path = os.environ.get("NLAM_FORECAST_SCALE_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump(rows, fh, indent=1)


# ---------------------------------------------------------------------------
# the chunk size and the chunk counts, from the public workspace queries
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tail_chunk_nodes(F):
    """Nodes per workgroup of forecast_tail_kernel: the node count at which nlam_forecast_workspace_floats grows a second row."""
    ws = L.load().nlam_forecast_workspace_floats
    n = 1
    while ws(1, n + 1, F) == 2 * F:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def _score_chunk_nodes(F, M):
    return EF._chunk_nodes(F, M)


@functools.lru_cache(maxsize=None)
def _product_chunk_nodes(F):
    return EP._chunk_nodes(F)


def _tail_chunks(N, F):
    return int(L.load().nlam_forecast_workspace_floats(1, N, F)) // (2 * F)


def _score_chunks(N, F, M):
    return int(L.load().nlam_ens_scores_workspace_floats(1, M, N, F)) // (F * (M + 5))


def _product_chunks(N, F):
    ws = L.load().nlam_ens_products_workspace_floats
    return int(ws(1, 1, N, F, 1, 0)) // int(ws(1, 1, 1, F, 1, 0))


def _nbr_words(nx, ny, F, M=1, S_=1, E=2, W=5):
    """Words nbr_finish_kernel adds per output: what the workspace holds beyond the node tables, per (start, event, scale, sum)."""
    total = int(L.load().nlam_ens_neighbourhood_workspace_floats(S_, M, nx, ny, F, E, W))
    return (total - nx * ny * (1 + 2 * S_ * E)) // (2 * S_ * E * W)


def _nodes_of(C, cn):
    """The two node counts of C chunks: the last chunk one node, the last chunk full."""
    return [(C - 1) * cn + 1, C * cn]


# ---------------------------------------------------------------------------
# inputs and per-node terms (host), shared by the stand-ins and the GPU tests
# ---------------------------------------------------------------------------
def _exact_scores_case(g, M, F, N, S_):
    """The integer recipe of test_ensemble_forecast.test_ens_scores_exact_on_integers."""
    a = torch.randint(-1, 2, (S_, 1, N, F), generator=g)
    t = torch.randint(-2, 3, (S_, 1, N, F), generator=g)
    j = torch.randint(0, M, (S_, 1, N, F), generator=g)
    x = (M * (a + t * (torch.arange(M).view(1, M, 1, 1) == j))).double()
    off = torch.randint(-1, 2, (S_, N, F), generator=g) * (torch.rand(S_, N, F, generator=g) < 0.125)
    y = (M * (a[:, 0] + off)).double()
    w = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N,), generator=g)].double()
    w[-1] = 2.0   # the last node, alone in its chunk at N = (C - 1) cn + 1, is counted
    mean, std = torch.randint(-3, 4, (F,), generator=g).double(), 2.0 ** torch.randint(-2, 3, (F,), generator=g).double()
    return x, y, w, mean, std


def _random_scores_case(g, M, F, N, S_):
    """The random recipe of test_ensemble_forecast.test_ens_scores_within_the_rounding_budget."""
    scale = torch.logspace(-1, 1, F).double()
    x = (torch.randn(S_, M, N, F, generator=g).float().double() * scale + 0.3 * scale).float().double()
    y = (torch.randn(S_, N, F, generator=g).float().double() * scale).float().double()
    w = torch.rand(N, generator=g).float().double() * (torch.rand(N, generator=g) > 0.3)
    w[0] = 0.0
    mean, std = torch.randn(F, generator=g).float().double(), (torch.rand(F, generator=g) + 0.5).float().double()
    return x, y, w, mean, std


def _score_terms(x, y, w):
    """The per-node float64 terms (S, F, N) of the four sums of philox_ref.ens_scores, and the rank of the truth (-1: not live)."""
    S_, M, N, F = x.shape
    xbar = x.mean(1)
    wn = w.view(1, N, 1)
    var = ((x - xbar[:, None]) ** 2).sum(1) / (M - 1) if M > 1 else torch.zeros_like(xbar)
    pair = torch.zeros_like(xbar)
    for i in range(M):
        for j in range(i):
            pair = pair + (x[:, i] - x[:, j]).abs()
    pair = pair / (M * (M - 1)) if M > 1 else pair
    t = {"ens_sq": wn * (xbar - y) ** 2, "ens_var": wn * var, "ens_abs": wn * (x - y[:, None]).abs().mean(1), "ens_pair": wn * pair}
    rank = torch.where((w != 0).view(1, N, 1), (x < y[:, None]).sum(1), torch.full((), -1, dtype=torch.int64))
    return {k: v.permute(0, 2, 1).numpy() for k, v in t.items()}, rank.permute(0, 2, 1).numpy()


def _scores_standin(x, y, w, cn, defect=None):
    """The sums and the histogram through the stand-in of ens_scores_kernel's node order and ens_finish_kernel's chunk order."""
    terms, rank = _score_terms(x, y, w)
    M = x.shape[1]
    got = {k: torch.from_numpy(S.chunked_sum(v, cn, defect)) for k, v in terms.items()}
    hist = np.stack([S.chunked_count(rank == r, cn, defect) for r in range(M + 1)], axis=-1)
    got["rank_hist"] = torch.from_numpy(hist.astype(np.int32))
    return got


def _score_failures(got, want, bounds=None):
    """The comparison of both tiers: the names of the outputs that miss -- bit for bit without `bounds`, inside them with."""
    bad = []
    for k in ("ens_sq", "ens_var", "ens_abs", "ens_pair"):
        if k not in got:
            continue
        if bounds is None:
            ok = torch.equal(got[k].double(), want[k])
        else:
            err = (got[k].double() - want[k]).abs()
            ok = bool((err <= bounds[k] * (1 + 1e-3)).all())
        if not ok:
            bad.append(k)
    if not torch.equal(got["rank_hist"], want["rank_hist"]):
        bad.append("rank_hist")
    return bad


def _tail_inputs(g, F, batch, nodes):
    """fp32 states, truths and interior weights of the tail's verification sums; the last node is interior and far from its truth,
    so that a chunk holding that node alone carries a visible share of every sum."""
    new = torch.randn(batch, nodes, F, generator=g) * 0.7
    truth = torch.randn(batch, nodes, F, generator=g) * 0.7
    truth[:, -1] += 40.0
    interior = (torch.rand(nodes, generator=g) >= 0.3).float()
    interior[-1] = 1.0
    return new, truth, interior / interior.sum()


def _tail_workspace(new, truth, w, cn):
    """forecast_tail_kernel's workspace (B, C, 2 F) in fp32: w (d d) and w |d| of live nodes, each chunk in node order."""
    d = new - truth
    wn = w.view(1, -1, 1)
    live = wn != 0
    sq = torch.where(live, wn * (d * d), torch.zeros(())).permute(0, 2, 1).numpy()
    ab = torch.where(live, wn * d.abs(), torch.zeros(())).permute(0, 2, 1).numpy()
    assert sq.dtype == np.float32
    return np.concatenate([S.chunk_partials(sq, cn), S.chunk_partials(ab, cn)], axis=1).transpose(0, 2, 1)   # (B, C, 2 F)


def _tail_sum_ratio(got, want64, nodes):
    """|got - want| over the bar of test_forecast.test_tail_against_the_step_tail_and_the_restatement, (nodes + 8) EPS32 |want|."""
    assert bool((want64 > 0).all())
    return float(((got.double() - want64).abs() / ((nodes + 8) * EPS32 * want64)).max())


def _product_tables(M, F, thresholds, levels):
    E, Qn = PRODUCT_EQ
    return EP._tables(EP._events(E, F, thresholds), levels[:Qn], M)


def _product_terms(x, y, w, tb, want):
    """Per-node float64 terms of the Brier (S, E, N) and pinball (S, Q, F, N) sums of ens_products_ref.ens_products."""
    N = x.shape[2]
    o = torch.stack([(y[:, :, v] < t) if s else (y[:, :, v] > t) for v, s, t in zip(tb.var, tb.sense, tb.thr.double().tolist())], 1)
    brier = w.view(1, 1, N) * (want["prob"] - o.double()) ** 2
    qs, yy = want["quant_std"], y[:, None]
    lev = tb.lev.double().view(1, -1, 1, 1)
    rho = torch.where(yy >= qs, lev * (yy - qs), (1.0 - lev) * (qs - yy))
    live = (w != 0).view(1, 1, N, 1)
    return {"brier": brier.numpy(), "pinball": (w.view(1, 1, N, 1) * rho).permute(0, 1, 3, 2).numpy(),
            "below": ((yy < qs) & live).permute(0, 1, 3, 2).numpy()}


def _products_standin(x, y, w, tb, want, cn, defect=None):
    t = _product_terms(x, y, w, tb, want)
    return {"brier": torch.from_numpy(S.chunked_sum(t["brier"], cn, defect)), "pinball": torch.from_numpy(S.chunked_sum(t["pinball"], cn, defect)),
            "below": torch.from_numpy(S.chunked_count(t["below"], cn, defect).astype(np.int32))}


def _nbr_case(g, M, nx, ny, F):
    """Integer members and truths (the exact tier's recipe), two events on the first variable with both senses, S = 1."""
    N = nx * ny
    x = torch.randint(-2, 3, (1, M, N, F), generator=g).double()
    y = torch.randint(-2, 3, (1, N, F), generator=g).double()
    w = EN._weights("random", nx, ny, g)
    var, sense, thr = EN._events(F, [0.5, 0.0, -0.5, 1.0])
    return x, y, w, (var[:2], sense[:2], thr[:2])


@functools.lru_cache(maxsize=None)
def _nbr_reference(M, nx, ny, F):
    """Computed once per case: the CPU tests and the GPU test share it."""
    x, y, w, ev = _nbr_case(torch.Generator().manual_seed(4000 + M + nx), M, nx, ny, F)
    return x, y, w, ev, NR.ens_neighbourhood(x, y, w, ev[0], ev[1], ev[2].double().tolist(), EN.RADII, nx, ny)


def _nbr_ratios(got, ref, w):
    b_fbs, b_ref = EN._budget(ref, w)
    return {k: float(((got[k].double() - ref[k]).abs() / b.clamp_min(1e-300)).max()) for k, b in (("fbs", b_fbs), ("fbs_ref", b_ref))}


def _nbr_standin(ref, w, defect=None):
    N = w.numel()
    lv = (w != 0).view(1, 1, 1, N)
    zero = torch.zeros((), dtype=torch.float64)
    p, o = torch.where(lv, ref["p"], zero), torch.where(lv, ref["o"], zero)
    wd = w.view(1, 1, 1, N)
    return {"fbs": torch.from_numpy(S.nbr_finish(S.nbr_words((wd * (p - o) ** 2).numpy()), defect).astype(np.float64)),
            "fbs_ref": torch.from_numpy(S.nbr_finish(S.nbr_words((wd * (p * p + o * o)).numpy()), defect).astype(np.float64))}


def _normal_ratio(got, want64):
    """The largest error of fp32 normals against the float64 Box-Muller values in units of EPS32 |want|: EF.NORMAL_ULPS is the bar."""
    return float((np.abs(np.asarray(got, dtype=np.float64) - want64) / (EPS32 * np.abs(want64))).max())


@functools.lru_cache(maxsize=None)
def _fill_reference():
    return P.normals(FILL_N, FILL_SEED, *FILL_COUNTER)


# ---------------------------------------------------------------------------
# CPU: the regimes, the stand-ins inside the budgets, the defects reported
# ---------------------------------------------------------------------------
def test_every_case_reaches_the_regime_it_is_named_for():
    table = {4: (1, [1, 1, 1, 1]), 5: (2, [2, 2, 1, 0]), 9: (3, [3, 3, 3, 0]), 37: (10, [10, 10, 10, 7])}
    for C_, (per, counts) in table.items():
        r = S.regime(C_)
        assert (r["per"], r["counts"]) == (per, counts)
    assert S.regime(4)["waves_used"] == 4 and not S.regime(4)["two_in_a_wave"]
    r = S.regime(37)
    assert r["per"] >= 8 and r["body_and_remainder"] and r["remainder_only"] and [n % 8 for n in r["counts"]] == [2, 2, 2, 7]
    for C_ in OLD_CHUNKS:   # the older suites: no chunk in wave 3, no wave with two chunks
        r = S.regime(C_)
        assert r["counts"][3] == 0 and not r["two_in_a_wave"] and not r["body_and_remainder"]
    # the chunk counts, from the workspace queries
    for F, batch in TAIL_FB:
        cn = _tail_chunk_nodes(F)
        assert cn == {17: 240, 16: 256}[F]
        for C_ in CHUNKS:
            assert [_tail_chunks(n, F) for n in _nodes_of(C_, cn)] == [C_, C_] and _tail_chunks((C_ - 1) * cn, F) == C_ - 1
    assert 3 * 2 * 17 > 64 and 3 * 2 * 17 <= 128 and 2 * 2 * 16 == 64   # forecast_finish_kernel's lane rounds
    assert 3 * 2 * TF.NVARS < 64                                        # the older suite: a third of one round idle
    for M, C_ in SCORE_CASES:
        cn = _score_chunk_nodes(F_ENS, M)
        assert [_score_chunks(n, F_ENS, M) for n in _nodes_of(C_, cn)] == [C_, C_]
    cn = _product_chunk_nodes(F_ENS)
    for M, C_ in PRODUCT_CASES:
        assert [_product_chunks(n, F_ENS) for n in _nodes_of(C_, cn)] == [C_, C_]
    # the neighbourhood grids: a second stride of nbr_finish_kernel's 64 lanes; 13 and at least 37 counting chunks
    assert _nbr_words(129, 128, 3) == 65 > 64 and _nbr_words(37, 37, 3) == 6   # the largest older grid: 1369 nodes, one round
    assert _product_chunks(129 * 128, 3) == 13 and _product_chunks(95 * 94, 17) == 38 >= 37
    # the grid caps
    assert (FILL_N + 3) // 4 > S.FILL_CAP_QUADS and (4099 + 3) // 4 < S.FILL_CAP_QUADS
    rows, dim = LATENT_SHAPES[1]
    assert rows * dim == 1049664 and (rows * dim + 3) // 4 > S.LATENT_CAP_QUADS > (300 * 7 + 3) // 4 > 256
    for nodes, ds in ROW_BIG.values():
        assert nodes * ds > S.ROW_CAP and nodes * ds - S.ROW_CAP < 512
    assert (61701 * 17) % 4 == 1 and (61704 * 17) % 4 == 0 and 2049 * 7 > 2048 and (2052 * 7) % 4 == 0 and (2049 * 7) % 4 == 3


@pytest.mark.parametrize("F,batch", TAIL_FB)
def test_tail_standin_stays_inside_the_bar_and_its_defects_are_reported(F, batch):
    cn = _tail_chunk_nodes(F)
    g = torch.Generator().manual_seed(F)
    for C_ in CHUNKS:
        r = S.regime(C_)
        for nodes in _nodes_of(C_, cn):
            new, truth, w = _tail_inputs(g, F, batch, nodes)
            ws = _tail_workspace(new, truth, w, cn)
            assert ws.shape == (batch, C_, 2 * F)
            sq64, ab64 = FR.masked_sums(new, truth, w)
            want = torch.cat([sq64, ab64], dim=1)

            def ratio(defect=None):
                return _tail_sum_ratio(torch.from_numpy(S.forecast_finish(ws, defect)), want, nodes)

            assert ratio() <= 1.0, (C_, nodes)
            assert ratio("last_chunk_dropped") > 1.0, (C_, nodes)
            if r["counts"][3]:
                assert ratio("wave3_dropped") > 1.0, (C_, nodes)
            if r["body_and_remainder"]:
                assert ratio("unroll_remainder_dropped") > 1.0, (C_, nodes)
            if batch * 2 * F > 64:
                assert ratio("second_round_wrong_item") > 1.0, (C_, nodes)


def test_wave_and_unroll_defects_pass_unnoticed_at_the_older_shapes():
    """What this file closes: at one to three chunks -- all the per-feature suites reach -- a finisher that drops wave 3 or the
    chunks behind an unrolled body gives every sum bit for bit, and with 30 sums forecast_finish_kernel has no second round."""
    g = torch.Generator().manual_seed(7)
    F, batch = TF.NVARS, TF.BATCH
    cn = _tail_chunk_nodes(F)
    for nodes in (TF.NODES, 1721):
        assert _tail_chunks(nodes, F) in OLD_CHUNKS
        ws = _tail_workspace(*_tail_inputs(g, F, batch, nodes), cn)
        for defect in ("wave3_dropped", "unroll_remainder_dropped", "second_round_wrong_item"):
            assert np.array_equal(S.forecast_finish(ws, defect), S.forecast_finish(ws)), (nodes, defect)
    M = 3
    cn = _score_chunk_nodes(F_ENS, M)
    for N in (cn - 1, cn, cn + 1):
        assert _score_chunks(N, F_ENS, M) in OLD_CHUNKS
        x, y, w, mean, std = _exact_scores_case(g, M, F_ENS, N, 1)
        want = P.ens_scores(x, y, w, mean, std)
        for defect in ("wave3_dropped", "unroll_remainder_dropped"):
            assert _score_failures(_scores_standin(x, y, w, cn, defect), want) == [], (N, defect)
    assert _nbr_words(37, 37, 3) == 6   # the largest older grid: one round of nbr_finish_kernel's lanes
    words = np.random.default_rng(0).random((2, 6)).astype(np.float32)
    assert np.array_equal(S.nbr_finish(words, "words_past_64_dropped"), S.nbr_finish(words))


@pytest.mark.parametrize("C_", CHUNKS)
def test_scores_standin_is_exact_on_integers_inside_the_budget_and_its_defects_are_reported(C_):
    M = 3
    cn = _score_chunk_nodes(F_ENS, M)
    r = S.regime(C_)
    g = torch.Generator().manual_seed(50 + C_)
    for N in _nodes_of(C_, cn):
        x, y, w, mean, std = _exact_scores_case(g, M, F_ENS, N, 1)
        want = P.ens_scores(x, y, w, mean, std)
        assert all(2 * float(want[k].max()) < 2 ** 24 for k in ("ens_sq", "ens_var", "ens_abs", "ens_pair"))
        terms, _ = _score_terms(x, y, w)
        assert all(np.array_equal(terms[k].sum(-1), want[k].numpy()) for k in terms)   # the terms are the reference's
        assert _score_failures(_scores_standin(x, y, w, cn), want) == []
        defects = ["last_chunk_dropped"] + (["wave3_dropped"] if r["counts"][3] else []) + (["unroll_remainder_dropped"] if r["body_and_remainder"] else [])
        for defect in defects:
            bad = _score_failures(_scores_standin(x, y, w, cn, defect), want)
            assert "rank_hist" in bad and "ens_abs" in bad, (N, defect, bad)
        x, y, w, mean, std = _random_scores_case(g, M, F_ENS, N, 1)
        want = P.ens_scores(x, y, w, mean, std)
        bounds = EF._score_bounds(x, y, w, mean, std, want)
        assert _score_failures(_scores_standin(x, y, w, cn), want, bounds) == []
        if N == C_ * cn:   # a full last chunk: the budget tier reports the dropped chunks too
            for defect in defects:
                assert {"ens_sq", "ens_var", "ens_abs", "ens_pair"} <= set(_score_failures(_scores_standin(x, y, w, cn, defect), want, bounds)), defect


@pytest.mark.parametrize("C_", [5, 37])
def test_products_standin_is_exact_on_integers_inside_the_budget_and_its_defects_are_reported(C_):
    M = 3
    cn = _product_chunk_nodes(F_ENS)
    r = S.regime(C_)
    g = torch.Generator().manual_seed(60 + C_)
    for N in _nodes_of(C_, cn):
        x, y, w, mean, std = EP._exact_case(g, M, F_ENS, N, 1)
        w[-1] = 2.0
        tb = _product_tables(M, F_ENS, [0.5, 0.0, -0.5, 1.0], EP.DYADIC)
        want = EP._reference(x, y, w, mean, std, tb)
        got = _products_standin(x, y, w, tb, want, cn)
        assert 2 ** 9 * float(want["pinball"].max()) < 2 ** 24
        assert torch.equal(got["pinball"], want["pinball"]) and torch.equal(got["below"], want["below"])
        defects = ["last_chunk_dropped"] + (["wave3_dropped"] if r["counts"][3] else []) + (["unroll_remainder_dropped"] if r["body_and_remainder"] else [])
        for defect in defects:
            bad = _products_standin(x, y, w, tb, want, cn, defect)
            assert not torch.equal(bad["pinball"], want["pinball"]), (N, defect)
        x, y, w, mean, std, tb = EP._random_case(g, M, F_ENS, N, 1, *PRODUCT_EQ)
        want = EP._reference(x, y, w, mean, std, tb)
        bounds = EP._bounds(x, y, w, std, tb, want)
        got = _products_standin(x, y, w, tb, want, cn)
        EP._check_budget(got, want, bounds, (C_, N))
        if N == C_ * cn:
            for defect in defects:
                with pytest.raises(AssertionError):
                    EP._check_budget(_products_standin(x, y, w, tb, want, cn, defect), want, bounds, (C_, N, defect))


def test_neighbourhood_standin_stays_inside_the_budget_and_the_dropped_words_are_reported():
    nx, ny, F = NBR_CASES[0]
    x, y, w, ev, ref = _nbr_reference(1, nx, ny, F)
    assert all(v <= 1.0 for v in _nbr_ratios(_nbr_standin(ref, w), ref, w).values())
    assert all(v > 1.0 for v in _nbr_ratios(_nbr_standin(ref, w, "words_past_64_dropped"), ref, w).values())


def test_generator_standin_passes_and_a_quad_index_that_wraps_with_the_grid_is_reported():
    want = _fill_reference()
    assert _normal_ratio(S.normals_standin(FILL_N, FILL_SEED, *FILL_COUNTER), want) <= 0.5 < EF.NORMAL_ULPS
    wrapped = S.normals_standin(FILL_N, FILL_SEED, *FILL_COUNTER, cap_quads=S.FILL_CAP_QUADS)
    assert _normal_ratio(wrapped, want) > EF.NORMAL_ULPS * (1 + 1e-3)
    assert _normal_ratio(wrapped[:4 * S.FILL_CAP_QUADS], want[:4 * S.FILL_CAP_QUADS]) <= 0.5      # only the second sweep is wrong,
    assert _normal_ratio(wrapped[:4099], want[:4099]) <= 0.5                                      # which n = 4099 never reaches
    rows, dim = LATENT_SHAPES[1]
    per = rows * dim
    want = P.latent_noise(0, 2, [5, 5], per, FILL_SEED)
    for b in range(2):
        assert _normal_ratio(S.normals_standin(per, FILL_SEED, 0, b, 5), want[b]) <= 0.5
        assert _normal_ratio(S.normals_standin(per, FILL_SEED, 0, b, 5, cap_quads=S.LATENT_CAP_QUADS), want[b]) > EF.NORMAL_ULPS * (1 + 1e-3)


def test_a_row_left_unwritten_past_the_capped_grid_is_reported():
    rng = np.random.default_rng(1)
    for nodes, ds in ROW_BIG.values():
        row = rng.standard_normal((nodes, ds)).astype(np.float32)
        assert _rows_equal(row.copy(), row)
        assert not _rows_equal(S.row_with_cap_defect(row), row)
    small = rng.standard_normal((2049, 7)).astype(np.float32)
    assert _rows_equal(S.row_with_cap_defect(small), small)   # the older shapes end below the cap: nothing to report


def _rows_equal(got, want):
    """The comparison of the data-row tests: the same fp32 bits, element by element (a NaN never equals)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and bool(np.array_equal(got.view(np.int32), want.view(np.int32)))


ROW_BIG = {"element": (61701, 17), "quad": (61704, 17)}   # 1 048 917 and 1 048 968 elements: just past 512 x 2048


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


_bits, _ptr, _stream = TF._bits, TF._ptr, TF._stream


@pytest.mark.gpu
@pytest.mark.parametrize("F,batch", TAIL_FB)
@pytest.mark.parametrize("C_", CHUNKS)
def test_forecast_tail_and_finish_over_many_chunks(dev, C_, F, batch):
    """nlam_forecast_tail + nlam_forecast_finish at C chunks per forecast, the last chunk one node and full, with and without
    clamps and the std head, aligned and one float off: the checks of test_forecast.test_tail_against_the_step_tail_and_the_restatement
    -- the state bit-equal to StepTailExtFunction, the sums inside (nodes + 8) EPS32 of the float64 sums of the values the kernel
    held, a second run bit-identical, every other slot at its sentinel.  The last node is interior and 40 away from its truth."""
    from neural_lam_amd.ops import StepTailExtFunction

    K, LEAD = 2, TF.LEAD
    cn = _tail_chunk_nodes(F)
    for nodes in _nodes_of(C_, cn):
        assert _tail_chunks(nodes, F) == C_
        for clamp, std_head, misalign in TAIL_OPTIONS:
            what = (C_, F, batch, nodes, clamp, std_head, misalign)
            c, put = TF._tail_case(dev, nodes, clamp, std_head, misalign, with_times=not misalign, nvars=F, batch=batch)
            c.truth[:, -1] += 40.0
            c.bmask[-1] = 0.0
            interior = 1.0 - c.bmask
            c.row_weight = interior / interior.sum()
            pred, pred_std, _ = StepTailExtFunction.apply(c.delta.view(batch, nodes, c.ld), c.prev0, c.truth, None, c.dstd, c.dmean, c.bmask,
                                                          None, None, 1.0, None, c.clamp)
            b = TF._tail_buffers(c, put, LEAD, verify=True)
            TF._run_tail(c, b, LEAD, K)
            assert torch.equal(_bits(b.prev), _bits(pred)) and torch.equal(_bits(b.pprev), _bits(c.prev0)), what
            assert int(c.lead) == K + 1
            mean, std = c.stats["state_mean"].double(), c.stats["state_std"].double()
            want = pred.double() * std + mean
            bound = 2 * EPS32 * ((pred.double() * std).abs() + mean.abs())
            assert bool(((b.out_state[:, K].double() - want).abs() <= bound).all()), what
            others = [k for k in range(LEAD) if k != K]
            assert bool(torch.isnan(b.out_state[:, others]).all()), what
            if std_head:
                want_std = pred_std.double() * std
                assert bool(((b.out_std[:, K].double() - want_std).abs() <= EPS32 * want_std.abs()).all()), what
                assert bool(torch.isnan(b.out_std[:, others]).all()), what
            t_valid = c.start + K + 1
            assert torch.equal(b.valid_times[:, K], c.times[t_valid] if c.times is not None else t_valid)
            assert bool((b.valid_times[:, others] == -1).all())
            sq64, ab64 = FR.masked_sums(b.prev.cpu(), c.truth.cpu(), c.row_weight.cpu())
            tol = (nodes + 8) * EPS32
            for name, got, want64 in (("sq", b.sq, sq64), ("ab", b.ab, ab64)):
                ratio = _tail_sum_ratio(got[:, K].cpu(), want64, nodes)
                print(what, name, "error / bar", ratio)
                _note("forecast_tail+finish", name, ratio)
                assert bool(((got[:, K].cpu().double() - want64).abs() <= tol * want64.abs()).all()), (what, name, ratio)
                assert bool(torch.isnan(got[:, others]).all()), what
            b2 = TF._tail_buffers(c, put, LEAD, verify=True)
            TF._run_tail(c, b2, LEAD, K)
            assert torch.equal(_bits(b.sq[:, K]), _bits(b2.sq[:, K])) and torch.equal(_bits(b.ab[:, K]), _bits(b2.ab[:, K])), what
            assert torch.equal(_bits(b.out_state[:, K]), _bits(b2.out_state[:, K])) and torch.equal(_bits(b.prev), _bits(b2.prev)), what


def _score_scale_shapes(M, C_):
    """(N, S, misaligned): the last chunk one node with one start, aligned; the last chunk full with three starts (one at M = 64,
    where the float64 budget of three starts at C = 37 would hold a gigabyte of temporaries), misaligned."""
    cn = _score_chunk_nodes(F_ENS, M)
    n_one, n_full = _nodes_of(C_, cn)
    return [(n_one, 1, False), (n_full, 1 if M == 64 else 3, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,C_", SCORE_CASES)
def test_ens_scores_exact_on_integers_over_many_chunks(dev, M, C_):
    """Tier (a) of test_ensemble_forecast at C chunks per start: every sum and the rank histogram bit for bit."""
    g = torch.Generator().manual_seed(1000 + 64 * C_ + M)
    for N, S_, misalign in _score_scale_shapes(M, C_):
        assert _score_chunks(N, F_ENS, M) == C_
        x, y, w, mean, std = _exact_scores_case(g, M, F_ENS, N, S_)
        want = P.ens_scores(x, y, w, mean, std)
        assert all(2 * float(want[k].max()) < 2 ** 24 for k in ("ens_sq", "ens_var", "ens_abs", "ens_pair"))   # halves, non-negative terms
        got = EF._scores_run(dev, x, y, w, mean, std, misalign)
        what = (M, C_, N, S_, misalign)
        assert _score_failures(got, want) == [], what
        assert torch.equal(got["mean"].double(), want["mean"]), what
        var = ((x - x.mean(1, keepdim=True)) ** 2).sum(1) / max(M - 1, 1)
        assert torch.equal(got["spread"], torch.sqrt(var.float()) * std.float()), what
        again = EF._scores_run(dev, x, y, w, mean, std, misalign)
        assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in again), what


@pytest.mark.gpu
@pytest.mark.parametrize("M,C_", SCORE_CASES)
def test_ens_scores_within_the_rounding_budget_over_many_chunks(dev, M, C_):
    """Tier (b) of test_ensemble_forecast at C chunks per start, against _score_bounds, whose tau counts the chunks."""
    g = torch.Generator().manual_seed(2000 + 64 * C_ + M)
    for N, S_, misalign in _score_scale_shapes(M, C_):
        x, y, w, mean, std = _random_scores_case(g, M, F_ENS, N, S_)
        assert not bool((x == y[:, None]).any())   # no ties: the histogram is exact
        want = P.ens_scores(x, y, w, mean, std)
        got = EF._scores_run(dev, x, y, w, mean, std, misalign)
        what = (M, C_, N, S_, misalign)
        bounds = EF._score_bounds(x, y, w, mean, std, want)
        for k, bound in bounds.items():
            err = (got[k].double() - want[k]).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            _note("ens_scores+finish", k, ratio)
            assert bool((err <= bound * (1 + 1e-3)).all()), (what, k, ratio)
        assert _score_failures(got, want, bounds) == [], what   # the comparison the stand-in's defects are reported by
        if M == 1:
            assert float(got["spread"].abs().max()) == 0.0
            assert float(got["ens_var"].abs().max()) == 0.0 and float(got["ens_pair"].abs().max()) == 0.0
        assert torch.equal(got["rank_hist"], want["rank_hist"]), what
        assert int(got["rank_hist"].sum()) == S_ * F_ENS * int((w != 0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("M,C_", PRODUCT_CASES)
def test_products_over_many_chunks(dev, M, C_):
    """Both tiers of test_ensemble_products at C chunks per start with four events and three quantiles.  The exact tier: prob, the
    reliability table, the quantile fields, the pinball sums and `below` bit for bit, the Brier sums bit for bit at M = 64 (dyadic
    probabilities; the condition on the float64 totals is asserted) and inside the budget at M = 3.  The budget tier: _bounds."""
    cn = _product_chunk_nodes(F_ENS)
    g = torch.Generator().manual_seed(3000 + 64 * C_ + M)
    n_one, n_full = _nodes_of(C_, cn)
    for N, S_, misalign in ((n_one, 1, False), (n_full, 1 if M == 64 else 3, True)):
        assert _product_chunks(N, F_ENS) == C_
        what = (M, C_, N, S_, misalign)
        x, y, w, mean, std = EP._exact_case(g, M, F_ENS, N, S_)
        w[-1] = 2.0
        tb = _product_tables(M, F_ENS, [0.5, 0.0, -0.5, 1.0], EP.DYADIC)
        want = EP._reference(x, y, w, mean, std, tb)
        got = EP._products_run(dev, x, y, w, mean, std, tb, misalign)
        assert torch.equal(got["prob"], want["count"].float() / float(M)), what
        assert torch.equal(got["rel_count"], want["rel_count"]) and torch.equal(got["rel_obs"], want["rel_obs"]), what
        assert bool((got["rel_count"].sum(-1) == int((w != 0).sum())).all()), what
        if M == 64:
            assert 2 ** 13 * float(want["brier"].max()) < 2 ** 24
            assert torch.equal(got["brier"].double(), want["brier"]), what
        else:
            EP._check_budget({"brier": got["brier"]}, want, EP._bounds(x, y, w, std, tb, want), what)
        assert torch.equal(got["quant"].double(), want["quant"]), what
        assert 2 ** 9 * float(want["pinball"].max()) < 2 ** 24
        assert torch.equal(got["pinball"].double(), want["pinball"]), what
        assert torch.equal(got["below"], want["below"]), what
        again = EP._products_run(dev, x, y, w, mean, std, tb, misalign)
        assert all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got), what
        # the budget tier
        x, y, w, mean, std, tb = EP._random_case(g, M, F_ENS, N, S_, *PRODUCT_EQ)
        for v, t in zip(tb.var, tb.thr.double().tolist()):
            assert not bool((x[..., v] == t).any()) and not bool((y[..., v] == t).any())
        want = EP._reference(x, y, w, mean, std, tb)
        got = EP._products_run(dev, x, y, w, mean, std, tb, misalign)
        bounds = EP._bounds(x, y, w, std, tb, want)
        for k in ("prob", "brier", "quant", "pinball"):
            err = (got[k].double() - want[k]).abs()
            _note("ens_products+finish", k, float((err / bounds[k].clamp_min(1e-300)).max()))
        EP._check_budget(got, want, bounds, what)
        assert torch.equal(got["rel_count"], want["rel_count"]) and torch.equal(got["rel_obs"], want["rel_obs"]), what
        assert bool((got["rel_count"].sum(-1) == int((w != 0).sum())).all()) and bool((got["rel_obs"] <= got["rel_count"]).all()), what


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,F", NBR_CASES)
@pytest.mark.parametrize("M", NBR_MEMBERS)
def test_neighbourhood_over_many_counting_chunks_and_a_second_finishing_stride(dev, M, nx, ny, F):
    """129 x 128 at F = 3: 65 evaluation workgroups, so nbr_finish_kernel's lanes take a second word, and 13 counting chunks;
    95 x 94 at F = 17: 38 counting chunks.  One start, two events, through test_ensemble_neighbourhood._check."""
    assert (_nbr_words(nx, ny, F, M) > 64) == (F == 3) and _product_chunks(nx * ny, F) == (13 if F == 3 else 38)
    x, y, w, ev, ref = _nbr_reference(M, nx, ny, F)
    for misalign in (False, True):
        got = EN._nbr_run(dev, x, y, w, ev, EN.RADII, nx, ny, misalign)
        for k, v in _nbr_ratios(got, ref, w).items():
            _note("ens_neighbourhood", k, v)
        EN._check(got, ref, w, (M, nx, ny, F, misalign))
    assert bool(torch.isnan(got["nprob"]).any()) and bool((ref["A"][4] == int((w != 0).sum())).all())


@pytest.mark.gpu
def test_generator_past_its_block_cap_matches_float64_box_muller(dev):
    """n = 4096 x 1024 + 4099: the 4096 blocks stride a second time over 1025 quads, the last one partial."""
    want = _fill_reference()
    first = None
    for misalign in (False, True):
        got = EF._fill(dev, FILL_N, FILL_SEED, *FILL_COUNTER, misalign=misalign)
        ratio = _normal_ratio(got.cpu().numpy(), want)
        print("normals past the block cap, misaligned", misalign, ": worst error", ratio, "ulp-units, bar", EF.NORMAL_ULPS)
        _note("philox_normal_fill", "normal", ratio / EF.NORMAL_ULPS)
        assert ratio <= EF.NORMAL_ULPS * (1 + 1e-3), (misalign, ratio)
        first = got.clone() if first is None else first
        assert torch.equal(_bits(got), _bits(first)), misalign   # the 16-byte and the element stores: the same values


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("rows,dim", LATENT_SHAPES)
@pytest.mark.parametrize("diagonal", [False, True])
def test_latent_sample_over_several_workgroups_and_past_its_block_cap(dev, diagonal, rows, dim, misalign):
    """(300, 7): 525 quads, three workgroups per item; (16401, 64): 262 416 quads per item on the 1024 blocks the launch is capped
    at, so 272 threads draw a second quad.  The checks of test_ensemble_forecast.test_latent_sample_draws_and_reparameterises."""
    lib = L.load()
    put = EF._misaligned if misalign else (lambda t: t)
    big = rows * dim > 4 * S.LATENT_CAP_QUADS
    S_, M, LEAD, K = (1, 2, 1, 0) if big else (2, 3, 4, 2)
    B, SEED = S_ * M, 0xDEADBEEF12345
    g = torch.Generator().manual_seed(rows * 10 + dim)
    params = put((torch.randn(B, rows, dim * (2 if diagonal else 1), generator=g) * 1.5).to(dev))
    if diagonal:
        params[0, 0, dim] = 25.0   # softplus' linear branch
    t0 = [(1 << 32) + 9] * M if big else [5] * M + [(1 << 32) + 9] * M
    start = torch.tensor(t0, dtype=torch.int64, device=dev)
    lead = torch.full((1,), K, dtype=torch.int32, device=dev)
    seed = torch.tensor([SEED], dtype=torch.int64, device=dev)
    nan = lambda *shape: put(torch.full(shape, float("nan"), device=dev))   # noqa: E731
    latent, noise = nan(B, rows, dim), nan(LEAD, B, rows, dim)
    p = EF._sample_args(params, latent, start, lead, seed, M, rows, dim, diagonal, LEAD, noise_out=noise)
    L.check(lib.nlam_latent_sample(C.byref(p), _stream()), "nlam_latent_sample")
    torch.cuda.synchronize()
    assert int(lead) == K
    others = [k for k in range(LEAD) if k != K]
    assert bool(torch.isnan(noise[others]).all()) and bool(torch.isfinite(noise[K]).all()) and bool(torch.isfinite(latent).all())
    want = P.latent_noise(K, M, t0, rows * dim, SEED)
    ratio = _normal_ratio(noise[K].cpu().numpy().reshape(B, -1), want)
    _note("latent_sample", "noise", ratio / EF.NORMAL_ULPS)
    assert ratio <= EF.NORMAL_ULPS * (1 + 1e-3), ratio
    for b in range(B):   # the generator's own values for counter (quad, lead, member, low word of t0)
        assert torch.equal(_bits(noise[K, b].reshape(-1)), _bits(EF._fill(dev, rows * dim, SEED, K, b % M, t0[b] & 0xFFFFFFFF))), b
    latent2 = nan(B, rows, dim)
    p2 = EF._sample_args(params, latent2, start, lead, None, M, rows, dim, diagonal, LEAD, noise_in=noise)
    L.check(lib.nlam_latent_sample(C.byref(p2), _stream()), "nlam_latent_sample")
    assert torch.equal(_bits(latent2), _bits(latent))
    ref64 = P.latent_sample(params.cpu(), noise[K].cpu(), diagonal)
    ref32 = P.latent_sample(params.cpu(), noise[K].cpu(), diagonal, torch.float32)
    err, err_ref = EF.rel_err(latent.cpu().double(), ref64), EF.rel_err(ref32.double(), ref64)
    bar = 2 * err_ref + 1e-6 + 2 * EPS32
    _note("latent_sample", "latent", err / bar)
    assert err <= bar, (err, err_ref)


# -- the data rows of nlam_series.inc ------------------------------------------
ROW_KINDS = ["plain", "members", "q16_state", "q16_forcing", "q16_both"]
ROW_ENTRIES = {"plain": ("nlam_window_batch", ""), "members": ("nlam_window_batch_ens", "_strided"), "q16_state": ("nlam_window_batch_q16", "_q16"),
               "q16_forcing": ("nlam_window_batch_q16", "_q16"), "q16_both": ("nlam_window_batch_q16", "_q16")}
ROW_PAST, ROW_FUT, ROW_TIMES = 2, 1, 6   # a window of four slots; a handful of times
ROW_SMALL = [(2049, 0), (2052, 0), (2052, 1)]   # nodes at d_state = 7; floats every fp32 buffer lies past a 16-byte boundary
ROW_BIG_PATH = {"plain": "quad", "members": "element", "q16_state": "quad", "q16_forcing": "element", "q16_both": "element"}


def _row_world(dev, kind, nodes, ds, df, lead, off):
    """A dataset of ROW_TIMES analysis times (two members unless plain) with the series of `kind` packed, and the float32 numpy
    series it stands for (decoded where packed)."""
    from neural_lam_amd.data import DeviceWeatherDataset, PackedSeries

    rng = np.random.default_rng(nodes + ds)
    members = 1 if kind == "plain" else 2
    axes = (ROW_TIMES,) if kind == "plain" else (ROW_TIMES, members)
    series = {"state": PS._field(rng, axes + (nodes, ds)), "forcing": PS._field(rng, axes + (nodes, df))}
    stats = PS._stats((nodes, ds, df))
    given, stands_for = {}, {}
    for name, x in series.items():
        if kind in ("q16_" + name, "q16_both"):
            scale, offset = Q.default_tables(x)
            codes = Q.encode(x, scale, offset)
            given[name], stands_for[name] = PackedSeries(codes, scale, offset), Q.decode(codes, scale, offset)
        else:
            given[name], stands_for[name] = put(torch.from_numpy(x), dev, off), x
    data = DeviceWeatherDataset(given["state"], given["forcing"], None, ar_steps=lead, num_past_forcing_steps=ROW_PAST,
                                num_future_forcing_steps=ROW_FUT, standardization=stats, device=dev)
    assert data.kernel == ROW_ENTRIES[kind][0] and data.members == members
    assert len(data) == members * od.dataset_len(ROW_TIMES, ROW_TIMES, lead, ROW_PAST, ROW_FUT)
    return data, stands_for["state"], stands_for["forcing"], stats, members


def _row_reference(state, forcing, stats, members, i, lead):
    """Sample i on the CPU: (init, target, windowed forcing) raw and standardised, float32 with one rounding per operation."""
    s, m = divmod(i, members)
    st, fo = (state, forcing) if members == 1 else (state[:, m], forcing[:, m])
    init, target, forc, _ = od.build_item(st, fo, None, s, lead, ROW_PAST, ROW_FUT)
    std = od.standardize_item(init, target, forc, stats["state_mean"], stats["state_std"], stats["forcing_mean"], stats["forcing_std"],
                              ROW_PAST + ROW_FUT + 1)
    assert all(a.dtype == np.float32 for a in std)
    return (init, target, forc), std


def _check_rows(dev, kind, nodes, ds, df, lead, off):
    from neural_lam_amd.forecast import dataset_source

    lib = L.load()
    data, state, forcing, stats, members = _row_world(dev, kind, nodes, ds, df, lead, off)
    count, W = len(data), ROW_PAST + ROW_FUT + 1
    picks = [0, count - 1] if members == 1 else [1, count - 2]
    assert len({(i // members, i % members) for i in picks}) == 2 and len({i % members for i in picks}) == members
    refs = [_row_reference(state, forcing, stats, members, i, lead) for i in picks]
    B = len(picks)
    # the window batch, raw and standardised
    for standardize in (False, True):
        outs = [Out((B, 2, nodes, ds), dev, off), Out((B, lead, nodes, ds), dev, off), Out((B, lead, nodes, df * W), dev, off)]
        times = torch.full((B, lead), -1, dtype=torch.int64, device=dev)
        data.batch(picks, standardize=standardize, out=tuple(o.view.view(o.shape) for o in outs) + (times,))
        torch.cuda.synchronize()
        got = [o.read().numpy() for o in outs]   # read() checks the guards
        for b, i in enumerate(picks):
            for name, g, want in zip(("init", "target", "forcing"), got, refs[b][int(standardize)]):
                assert _rows_equal(g[b], np.ascontiguousarray(want)), (kind, nodes, off, standardize, i, name)
        assert times.cpu().tolist() == [[i // members + 2 + k for k in range(lead)] for i in picks]
    # the forecast pair: the standardised rows, lead by lead
    idx = torch.tensor(picks, dtype=torch.int64, device=dev)
    start = idx + max(2, ROW_PAST) - 1   # the plain pair is handed the time index of `prev`
    counter = torch.full((1,), 7, dtype=torch.int32, device=dev)
    keep = {k: torch.as_tensor(v).to(dev) for k, v in stats.items()}
    p = L.Forecast()
    p.lead = _ptr(counter)
    p.state_mean, p.state_std, p.forcing_mean, p.forcing_std = (_ptr(keep[k]) for k in ("state_mean", "state_std", "forcing_mean", "forcing_std"))
    p.nodes, p.d_state, p.d_forcing, p.batch = nodes, ds, df, B
    p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps = lead, ROW_PAST, ROW_FUT
    suffix = ROW_ENTRIES[kind][1]
    if kind == "plain":
        p.state, p.forcing, p.start, p.n_times = _ptr(data.state), _ptr(data.forcing), _ptr(start), ROW_TIMES
        extra = []
    else:
        src = dataset_source(data, idx)
        extra = [C.byref(src)] + ([C.byref(data.packed_source())] if suffix == "_q16" else [])
    init_fn, head_fn = getattr(lib, "nlam_forecast_init" + suffix), getattr(lib, "nlam_forecast_head" + suffix)
    prev, pprev = Out((B, nodes, ds), dev, off), Out((B, nodes, ds), dev, off)
    p.prev, p.prev_prev = C.c_void_p(prev.ptr()), C.c_void_p(pprev.ptr())
    truth0, fw0 = Out((B, nodes, ds), dev, off), Out((B, nodes, df * W), dev, off)
    p.truth, p.forcing_windowed = C.c_void_p(truth0.ptr()), C.c_void_p(fw0.ptr())
    L.check(init_fn(C.byref(p), *extra, _stream()), "nlam_forecast_init" + suffix)
    torch.cuda.synchronize()
    assert int(counter) == 0 and truth0.untouched() and fw0.untouched()
    got_pprev, got_prev = pprev.read().numpy(), prev.read().numpy()
    for b, i in enumerate(picks):
        want = refs[b][1][0]
        assert _rows_equal(got_pprev[b], np.ascontiguousarray(want[0])) and _rows_equal(got_prev[b], np.ascontiguousarray(want[1])), (kind, nodes, off, i)
    for k in range(lead):
        truth, fw = Out((B, nodes, ds), dev, off), Out((B, nodes, df * W), dev, off)
        p.truth, p.forcing_windowed = C.c_void_p(truth.ptr()), C.c_void_p(fw.ptr())
        counter.fill_(k)
        L.check(head_fn(C.byref(p), *extra, _stream()), "nlam_forecast_head" + suffix)
        torch.cuda.synchronize()
        assert int(counter) == k
        got_truth, got_fw = truth.read().numpy(), fw.read().numpy()
        for b, i in enumerate(picks):
            assert _rows_equal(got_truth[b], np.ascontiguousarray(refs[b][1][1][k])), (kind, nodes, off, i, k, "truth")
            assert _rows_equal(got_fw[b], np.ascontiguousarray(refs[b][1][2][k])), (kind, nodes, off, i, k, "forcing")


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,off", ROW_SMALL)
@pytest.mark.parametrize("kind", ROW_KINDS)
def test_data_rows_of_several_workgroups_against_numpy(dev, kind, nodes, off):
    """Rows of 2049 x 7 = 14 343 elements (no multiple of 4: element by element) and 2052 x 7 = 14 364 (the 16-byte path; one float
    off: the fallback) on eight workgroups, windowed forcing rows of 12 per node: nlam_window_batch, nlam_window_batch_ens and
    nlam_window_batch_q16 with the state, the forcing and both packed, raw and standardised, and the forecast pairs
    nlam_forecast_init / _head, _strided and _q16 on the same series, bit for bit against oracle.data and packed_ref in numpy
    float32.  Every output starts as NaN between NaN guards."""
    _check_rows(dev, kind, nodes, 7, 3, lead=2, off=off)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ROW_KINDS)
def test_data_rows_past_the_block_cap_against_numpy(dev, kind):
    """Rows of 61 701 x 17 = 1 048 917 (element by element) or 61 704 x 17 = 1 048 968 (16-byte path) elements, just past the 512
    blocks of 2048 a launch is capped at, so the grid strides a third time over its first few quads; the forcing row of 5 x 4 per
    node holds 1.23 M.  Once per entry, one lead."""
    nodes, ds = ROW_BIG[ROW_BIG_PATH[kind]]
    assert nodes * ds > S.ROW_CAP and nodes * 5 * (ROW_PAST + ROW_FUT + 1) > S.ROW_CAP
    _check_rows(dev, kind, nodes, ds, 5, lead=1, off=0)
