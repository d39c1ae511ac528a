"""Exceedance probabilities and quantile fields of a sampled ensemble (nlam_ens_products; EnsembleForecast(events=..., quantiles=...)).
Without a GPU: the C-ABI (exports, struct layout, every argument check, the workspace function), the float64 reference against
hand-computed cases and numpy.quantile, and the engine's host validation.  On the GPU: the launch against the reference -- an
exact tier on integers, a budget tier on random states, run-to-run bit identity, truth = NULL -- and the engine on the Graph-EFM
golden cases: graph against eager, launch counts, set_thresholds, the reference applied to the members, given noise, and a
deterministic predictor."""
import ctypes as C
import subprocess
import types

import numpy as np
import pytest
import torch

import ens_products_ref as R
from conftest import ROOT
from neural_lam_amd import _lib as L

U = 2.0 ** -24   # fp32 unit roundoff
NEW_EXPORTS = ["nlam_ens_products", "nlam_ens_products_workspace_floats"]
POINTERS = ("prev", "truth", "row_weight", "state_mean", "state_std", "lead", "event_var", "event_sense", "event_thr", "q_index",
            "q_frac", "q_level", "prob", "quant", "brier", "rel_count", "rel_obs", "pinball", "below", "workspace")
SCORES = ("brier", "rel_count", "rel_obs", "pinball", "below")


# ---------------------------------------------------------------------------
# CPU: the C-ABI
# ---------------------------------------------------------------------------
def test_products_symbols_are_exported_and_the_struct_matches_c_layout(tmp_path):
    import re

    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert declared == set(L.EXPORTS)
    assert lib.nlam_abi_version() == 8 == L.ABI_VERSION
    fields = [name for name, _ in L.EnsProducts._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
                   'int main(){printf("%zu", sizeof(nlam_ens_products_t));\n'
                   + "".join(f'printf(" %zu", offsetof(nlam_ens_products_t, {f}));\n' for f in fields)
                   + 'printf(" %d %d %d %d\\n", NLAM_ABI_VERSION, NLAM_ENS_MAX_MEMBERS, NLAM_ENS_MAX_EVENTS, NLAM_ENS_MAX_QUANTILES);'
                     ' return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == ([C.sizeof(L.EnsProducts)] + [getattr(L.EnsProducts, f).offset for f in fields]
                   + [8, L.ENS_MAX_MEMBERS, L.ENS_MAX_EVENTS, L.ENS_MAX_QUANTILES])
    assert (L.ENS_MAX_EVENTS, L.ENS_MAX_QUANTILES) == (32, 16)


def test_products_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    ws = lib.nlam_ens_products_workspace_floats
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    S, M, N, F, LEAD, E, Q = 2, 3, 37, 5, 4, 3, 2
    nws = ws(S, M, N, F, E, Q)
    assert nws == S * (E * (2 * M + 3) + 2 * Q * F)   # one chunk: E Brier + Q F pinball sums, 2 E (M + 1) + Q F counts
    for bad in ((0, M, N, F, E, Q), (S, 0, N, F, E, Q), (S, M, 0, F, E, Q), (S, M, N, 0, E, Q), (S, M, N, F, -1, Q), (S, M, N, F, E, -1),
                (S, M, N, F, 0, 0)):
        assert ws(*bad) == -1, bad
    for bad in ((S, 65, N, F, E, Q), (S, M, N, 257, E, Q), (S, M, N, F, 33, Q), (S, M, N, F, E, 17)):
        assert ws(*bad) == -2, bad
    # at the maxima: 256 variables make chunks of 16 nodes; per (start, chunk) 32 (2 * 64 + 3) + 2 * 16 * 256 words
    assert ws(3, 64, 1000, 256, 32, 16) == 3 * -(-1000 // 16) * (32 * 131 + 2 * 16 * 256)
    assert ws(S, M, N, F, E, 0) == S * E * (2 * M + 3) and ws(S, M, N, F, 0, Q) == S * 2 * Q * F

    def args(**kw):
        p = L.EnsProducts()
        for name in POINTERS:
            setattr(p, name, fake)
        p.workspace_floats, p.starts, p.members, p.nodes, p.d_state, p.max_lead, p.events, p.quantiles = nws, S, M, N, F, LEAD, E, Q
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    call = lib.nlam_ens_products
    assert call(None, None) == -1
    no_scores = {name: None for name in SCORES}
    einval = [{name: None} for name in ("prev", "row_weight", "state_mean", "state_std", "lead", "workspace")]
    einval += [dict(starts=0), dict(members=0), dict(nodes=0), dict(d_state=0), dict(max_lead=0), dict(events=-1), dict(quantiles=-1),
               dict(events=0, quantiles=0), dict(workspace_floats=nws - 1)]
    einval += [{name: None} for name in ("event_var", "event_sense", "event_thr", "prob", "q_index", "q_frac", "q_level", "quant")]
    einval += [{name: None} for name in SCORES]                                     # truth without all of them
    einval += [dict(no_scores, truth=None, **{name: fake}) for name in SCORES]      # a score pointer without truth
    for kw in einval:
        assert call(args(**kw), None) == -1, kw
    for kw in (dict(members=65), dict(d_state=257), dict(starts=65536), dict(events=33), dict(quantiles=17),
               dict(nodes=1 << 27, d_state=16)):
        assert call(args(workspace_floats=1 << 50, **kw), None) == -2, kw
    # a part that was not asked for needs none of its pointers
    assert call(args(events=0, event_var=None, event_sense=None, event_thr=None, prob=None, brier=None, rel_count=None, rel_obs=None,
                     starts=65536, workspace_floats=1 << 50), None) == -2
    assert call(args(quantiles=0, q_index=None, q_frac=None, q_level=None, quant=None, pinball=None, below=None, starts=65536,
                     workspace_floats=1 << 50), None) == -2
    assert call(args(truth=None, starts=65536, workspace_floats=1 << 50, **no_scores), None) == -2


# ---------------------------------------------------------------------------
# CPU: the reference
# ---------------------------------------------------------------------------
def _t(v):
    return torch.tensor(v, dtype=torch.float64)


def test_products_reference_against_hand_computed_cases():
    # M = 2, members 1 and 4 (given unsorted): the median is 2.5, levels 0 and 1 give the ends
    idx, frac = R.quantile_tables([0.5, 0.0, 1.0], 2)
    assert (idx, frac) == ([0, 0, 1], [0.5, 0.0, 0.0])
    x = _t([4.0, 1.0]).view(1, 2, 1, 1)
    r = R.ens_products(x, _t([3.0]).view(1, 1, 1), _t([0.5]), q_index=idx, q_frac=frac, q_level=[0.5, 0.0, 1.0],
                       state_mean=_t([10.0]), state_std=_t([2.0]))
    assert r["quant_std"].view(-1).tolist() == [2.5, 1.0, 4.0] and r["quant"].view(-1).tolist() == [15.0, 12.0, 18.0]
    # truth 3: above the median by 0.5 -> 0.5 * 0.5; above the minimum by 2 -> 0 * 2; below the maximum by 1 -> (1 - 1) * 1
    assert r["pinball"].view(-1).tolist() == [0.5 * 0.25, 0.0, 0.0] and r["below"].view(-1).tolist() == [0, 0, 1]
    # M = 1: every quantile is the member, prob is 0 or 1
    idx, frac = R.quantile_tables([0.0, 0.3, 1.0], 1)
    assert idx == [0, 0, 0] and frac == [0.0, 0.0, 0.0]
    r = R.ens_products(_t([7.0]).view(1, 1, 1, 1), None, _t([1.0]), [0, 0], [0, 1], [5.0, 5.0], idx, frac, [0.0, 0.3, 1.0])
    assert r["quant"].view(-1).tolist() == [7.0, 7.0, 7.0] and r["prob"].view(-1).tolist() == [1.0, 0.0] and "brier" not in r
    # ties on the threshold count in neither sense: members (2, 2, 5) against 2
    x = _t([2.0, 2.0, 5.0]).view(1, 3, 1, 1)
    r = R.ens_products(x, _t([2.0]).view(1, 1, 1), _t([1.0]), [0, 0], [0, 1], [2.0, 2.0])
    assert r["count"].view(-1).tolist() == [1, 0] and r["prob"].view(-1).tolist() == [1 / 3, 0.0]
    assert r["rel_obs"].sum().item() == 0   # the truth on the threshold is in neither event
    # three members, three nodes, one event x > 0; the last node has weight 0 and is in no table
    #   node 0: members (-1, 1, 2) -> c = 2, truth 1 in the event:  (2/3 - 1)^2 = 1/9
    #   node 1: members (-1, -2, 3) -> c = 1, truth -1 not in it:   (1/3)^2     = 1/9
    #   node 2: members (1, 1, 1)  -> c = 3, weight 0
    x = _t([[-1.0, -1.0, 1.0], [1.0, -2.0, 1.0], [2.0, 3.0, 1.0]]).view(1, 3, 3, 1)
    y = _t([1.0, -1.0, 1.0]).view(1, 3, 1)
    w = _t([0.5, 2.0, 0.0])
    r = R.ens_products(x, y, w, [0], [0], [0.0], [1], [0.0], [0.5])
    assert r["count"].view(-1).tolist() == [2, 1, 3]
    assert abs(r["brier"].item() - (0.5 / 9 + 2.0 / 9)) < 1e-15
    assert r["rel_count"].view(-1).tolist() == [0, 1, 1, 0] and r["rel_obs"].view(-1).tolist() == [0, 0, 1, 0]
    # medians 1, -1, 1 against truths 1, -1, 1: no loss, nothing below; weight 0 counted nowhere
    assert r["pinball"].item() == 0.0 and r["below"].item() == 0
    r = R.ens_products(x, y - 0.5, w, q_index=[1], q_frac=[0.0], q_level=[0.5])
    assert r["pinball"].item() == 0.5 * 0.25 + 2.0 * 0.25 and r["below"].item() == 2


def test_products_reference_quantile_is_numpys_linear_quantile():
    rng = np.random.default_rng(5)
    for M in (1, 2, 3, 5, 20, 33, 64):
        x = rng.standard_normal((2, M, 7, 3)) * 10.0 ** rng.integers(-2, 3, size=(1, 1, 1, 3))
        levels = [0.0, 1.0, 0.5, 0.1, 0.9, 1 / 3, 0.77] + list(rng.random(4))
        idx, frac = R.quantile_tables(levels, M)
        got = R.quantiles(torch.from_numpy(x), idx, frac, dim=1).numpy()
        want = np.moveaxis(np.quantile(x, levels, axis=1), 0, 1)
        scale = np.abs(x).max(axis=1, keepdims=True)
        assert np.all(np.abs(got - want) <= 8 * np.finfo(np.float64).eps * scale), M   # two float64 forms of one interpolation


def test_engine_validates_events_and_quantiles_on_the_host():
    from neural_lam_amd.forecast import EnsembleForecast, parse_products, quantile_tables

    names = ["t2m", "u10", "v10"]
    ev, lv = parse_products([("u10", ">", 3.5), (2, "<", -1)], [0, 0.5, 1], names, 3)
    assert ev == [(1, 0, 3.5), (2, 1, -1.0)] and lv == [0.0, 0.5, 1.0]
    assert parse_products(None, None, names, 3) == ([], [])
    assert quantile_tables([0.0, 0.5, 1.0, 0.1], 5) == R.quantile_tables([0.0, 0.5, 1.0, 0.1], 5)
    step = types.SimpleNamespace(state_var_names=names, state_mean=torch.zeros(3))   # the checks come before anything else is read
    bad = [dict(events=[("q", ">", 0.0)]), dict(events=[(3, ">", 0.0)]), dict(events=[(-1, "<", 0.0)]), dict(events=[(1.5, "<", 0.0)]),
           dict(events=[("t2m", ">=", 0.0)]), dict(events=[("t2m", 0, 0.0)]), dict(events=[("t2m", ">")]),
           dict(events=[("t2m", ">", float("nan"))]), dict(quantiles=[1.01]), dict(quantiles=[0.5, -0.1]),
           dict(events=[(0, ">", float(i)) for i in range(33)]), dict(quantiles=[i / 16 for i in range(17)])]
    for kw in bad:
        with pytest.raises(ValueError, match="EnsembleForecast"):
            EnsembleForecast(step, None, 3, members=4, **kw)
    with pytest.raises(ValueError, match="Forecast needs"):   # the maxima themselves pass on to the next check
        EnsembleForecast(step, None, 3, members=4, events=[(0, ">", float(i)) for i in range(32)], quantiles=[i / 15 for i in range(16)])


# ---------------------------------------------------------------------------
# GPU: nlam_ens_products at the C-ABI
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _misaligned(t):
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


def _chunk_nodes(F):
    """Nodes per workgroup, read off the workspace function: the node count at which a second row of words appears."""
    ws = L.load().nlam_ens_products_workspace_floats
    n = 1
    while ws(1, 1, n + 1, F, 1, 0) == ws(1, 1, 1, F, 1, 0):
        n += 1
    return n


class Tables(types.SimpleNamespace):
    """The device tables' host values: event_var / event_sense (int), event_thr / q_frac / q_level (fp32 values as float64)."""


def _tables(events, levels, M):
    idx, frac = R.quantile_tables(levels, M)
    f32 = lambda v: torch.tensor(v, dtype=torch.float64).float()   # noqa: E731
    return Tables(var=[e[0] for e in events], sense=[e[1] for e in events], thr=f32([e[2] for e in events]), idx=idx,
                  frac=f32(frac), lev=f32(list(levels)))


def _reference(x, y, w, mean, std, tb):
    return R.ens_products(x, y, w, tb.var, tb.sense, tb.thr.double().tolist(), tb.idx, tb.frac.double().tolist(),
                          tb.lev.double().tolist(), mean, std)


def _products_run(dev, x, y, w, mean, std, tb, misalign, K=1, LEAD=3):
    """One nlam_ens_products launch at lead K on x (S, M, N, F), y (S, N, F) or None: outputs with every other slot poisoned."""
    lib = L.load()
    put = _misaligned if misalign else (lambda t: t)
    S, M, N, F = x.shape
    E, Q = len(tb.var), len(tb.idx)
    prev = put(x.reshape(S * M, N, F).float().to(dev))
    truth = None
    if y is not None:
        truth = torch.full((S, M, N, F), float("nan"))
        truth[:, 0] = y.float()   # the truth of member 0 is used
        truth = put(truth.reshape(S * M, N, F).to(dev))
    nan = lambda *shape: put(torch.full(shape, float("nan"), device=dev))   # noqa: E731
    ints = lambda *shape: put(torch.full(shape, -7, dtype=torch.int32, device=dev))   # noqa: E731
    o = types.SimpleNamespace()
    if E:
        o.prob = nan(S, LEAD, E, N)
        if y is not None:
            o.brier, o.rel_count, o.rel_obs = nan(S, LEAD, E), ints(S, LEAD, E, M + 1), ints(S, LEAD, E, M + 1)
    if Q:
        o.quant = nan(S, LEAD, Q, N, F)
        if y is not None:
            o.pinball, o.below = nan(S, LEAD, Q, F), ints(S, LEAD, Q, F)
    nws = int(lib.nlam_ens_products_workspace_floats(S, M, N, F, E, Q))
    ws = torch.full((nws,), float("nan"), device=dev)
    lead = torch.full((1,), K, dtype=torch.int32, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    keep = [t.float().to(dev) for t in (w, mean, std)] + [i32(tb.var), i32(tb.sense), tb.thr.to(dev), i32(tb.idx), tb.frac.to(dev),
                                                           tb.lev.to(dev)]
    p = L.EnsProducts()
    p.prev, p.truth, p.lead, p.workspace, p.workspace_floats = _ptr(prev), _ptr(truth), _ptr(lead), _ptr(ws), nws
    p.row_weight, p.state_mean, p.state_std = (_ptr(t) for t in keep[:3])
    if E:
        p.event_var, p.event_sense, p.event_thr = (_ptr(t) for t in keep[3:6])
    if Q:
        p.q_index, p.q_frac, p.q_level = (_ptr(t) for t in keep[6:])
    for name, t in vars(o).items():
        setattr(p, name, _ptr(t))
    p.starts, p.members, p.nodes, p.d_state, p.max_lead, p.events, p.quantiles = S, M, N, F, LEAD, E, Q
    L.check(lib.nlam_ens_products(C.byref(p), _stream()), "nlam_ens_products")
    torch.cuda.synchronize()
    assert int(lead) == K   # only read
    others = [k for k in range(LEAD) if k != K]
    got = {}
    for name, t in vars(o).items():
        assert bool(torch.isnan(t[:, others]).all()) if t.dtype == torch.float32 else bool((t[:, others] == -7).all()), name
        got[name] = t[:, K].cpu().clone()
    return got


MEMBERS = [1, 2, 3, 5, 20, 33, 64]
COUNTS = [(e, q) for e in (0, 1, 32) for q in (0, 1, 16) if e or q]


def _shapes():
    """(F, N, S, misaligned, E, Q): every F with every N around the chunk, both S, both alignments; the eight (E, Q) pairs go
    round, two per shape."""
    i = 0
    for F in (1, 5, 17):
        cn = _chunk_nodes(F)
        for N in sorted({1, 5, cn - 1, cn, cn + 1} - {0}):
            for S, misalign in ((1, False), (3, True)) if N > 5 else ((1, False), (1, True), (3, False), (3, True)):
                for E, Q in (COUNTS[i % 8], COUNTS[(i + 5) % 8]):
                    yield F, N, S, misalign, E, Q
                i += 1


def _events(E, F, thresholds):
    """E events: variable e // 2 % F, so two events share a variable, with both senses; the thresholds go round."""
    return [((e // 2) % F, e % 2, thresholds[(e // 2) % len(thresholds)]) for e in range(E)]


DYADIC = [0.0, 1.0, 0.5, 0.25, 0.8125] + [k / 16 for k in (1, 2, 3, 5, 6, 7, 9, 10, 11, 14, 15)]
LEVELS = [0.0, 1.0, 0.5, 0.1, 0.9] + [0.05, 0.2, 0.3, 1 / 3, 0.4, 0.6, 2 / 3, 0.7, 0.8, 0.95, 0.99]


def _exact_case(g, M, F, N, S):
    """Integer members around an integer a per element (a third of them one or two away), the truth a, rarely one away;
    weights in {0, 1/2, 1, 2}, an integer mean and a power-of-two std."""
    a = torch.randint(-1, 2, (S, 1, N, F), generator=g)
    t = torch.randint(-2, 3, (S, M, N, F), generator=g) * (torch.rand(S, M, N, F, generator=g) < 1 / 3)
    x = (a + t).double()
    off = torch.randint(-1, 2, (S, N, F), generator=g) * (torch.rand(S, N, F, generator=g) < 0.125)
    y = (a[:, 0] + off).double()
    w = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N,), generator=g)].double()
    mean, std = torch.randint(-3, 4, (F,), generator=g).double(), 2.0 ** torch.randint(-2, 3, (F,), generator=g).double()
    return x, y, w, mean, std


def _tau(F, N):
    cn = _chunk_nodes(F)
    return U * (min(cn, N) + -(-N // cn) + 24)


def _bounds(x, y, w, std, tb, want):
    """The budget of test_products_within_the_rounding_budget's docstring; `near` counts the live nodes whose truth lies within
    the quantile's own error of it (only there may `below` differ)."""
    S, M, N, F = x.shape
    tau = _tau(F, N)
    b = {}
    if tb.var:
        p = want["prob"]
        b["prob"] = U * p
        if y is not None:
            o = torch.stack([(y[:, :, v] < t) if s else (y[:, :, v] > t) for v, s, t in zip(tb.var, tb.sense, tb.thr.double().tolist())], 1)
            d = (p - o.double()).abs()
            b["brier"] = (w.view(1, 1, N) * 2 * U * p * d).sum(2) + (tau + 4 * U) * want["brier"]
    if tb.idx:
        xs = torch.sort(x, dim=1).values
        gap = torch.stack([xs[:, min(i + 1, M - 1)] - xs[:, i] for i in tb.idx], 1)
        e_q = U * (tb.frac.double().view(1, -1, 1, 1) * gap + want["quant_std"].abs())
        b["quant"] = e_q * std + U * want["quant"].abs()
        if y is not None:
            b["pinball"] = (w.view(1, 1, N, 1) * e_q).sum(2) + (tau + 4 * U) * want["pinball"]
            close = ((y[:, None] - want["quant_std"]).abs() <= e_q) & (w != 0).view(1, 1, N, 1)
            b["near"] = close.sum(2)
    return b


def _check_budget(got, want, bounds, what):
    for k in ("prob", "brier", "quant", "pinball"):
        if k in got:
            err = (got[k].double() - want[k]).abs()
            assert bool((err <= bounds[k] * (1 + 1e-3)).all()), (what, k, float((err / bounds[k].clamp_min(1e-300)).max()))
    if "below" in got:
        assert bool(((got["below"] - want["below"]).abs() <= bounds["near"]).all()), what


@pytest.mark.gpu
@pytest.mark.parametrize("M", MEMBERS)
def test_products_exact_on_integers(dev, M):
    """Tier (a).  Integer members and truths, thresholds on half-integers and on integers (ties), dyadic levels k / 16: the
    interpolation weight g = q (M - 1) - i is a multiple of 1/16, so every quantile is a multiple of 1/16 of small magnitude and,
    with an integer mean and a power-of-two std, exact in both units; rho is a multiple of 2^-8 and w rho of 2^-9, so every
    partial pinball sum is exact while 2^9 * total < 2^24 (asserted; the terms are non-negative).  prob = (float)c / (float)M is
    one correctly rounded division, the integer tables are exact for every M, and for M in {1, 2, 64} c / M is dyadic, (c / M -
    o)^2 a multiple of 2^-12 and the Brier sum exact while 2^13 * total < 2^24 (asserted).  For the other M the Brier sum is
    checked inside tier (b)'s budget."""
    g = torch.Generator().manual_seed(40 + M)
    seen = dict(tie=False, above=False, below=False, none=False, all=False)
    for F, N, S, misalign, E, Q in _shapes():
        x, y, w, mean, std = _exact_case(g, M, F, N, S)
        tb = _tables(_events(E, F, [0.5, 0.0, -0.5, 1.0, -3.5, 3.5, -1.0, 1.5]), DYADIC[:Q], M)
        want = _reference(x, y, w, mean, std, tb)
        got = _products_run(dev, x, y, w, mean, std, tb, misalign)
        what = (M, F, N, S, misalign, E, Q)
        if E:
            assert torch.equal(got["prob"], want["count"].float() / float(M)), what
            assert torch.equal(got["rel_count"], want["rel_count"]) and torch.equal(got["rel_obs"], want["rel_obs"]), what
            assert bool((got["rel_count"].sum(-1) == int((w != 0).sum())).all()), what
            if M in (1, 2, 64):
                assert 2 ** 13 * float(want["brier"].max()) < 2 ** 24
                assert torch.equal(got["brier"].double(), want["brier"]), what
            else:
                _check_budget({"brier": got["brier"]}, want, _bounds(x, y, w, std, tb, want), what)
            for v, s, t in zip(tb.var, tb.sense, tb.thr.tolist()):
                seen["tie"] |= bool((x[..., v] == t).any()) and bool((y[..., v] == t).any())
                seen["below" if s else "above"] = True
            seen["none"] |= bool((want["count"] == 0).all(-1).any())
            seen["all"] |= bool((want["count"] == M).all(-1).any())
        if Q:
            assert torch.equal(got["quant"].double(), want["quant"]), what
            assert 2 ** 9 * float(want["pinball"].max()) < 2 ** 24
            assert torch.equal(got["pinball"].double(), want["pinball"]), what
            assert torch.equal(got["below"], want["below"]), what
    assert all(seen.values()), seen   # ties on a threshold, both senses, an event no member is in and one every member is in


def _random_case(g, M, F, N, S, E, Q):
    """Random fp32 states with per-variable scales, weights with zeros among them, and thresholds moved to the next fp32 value
    that no member and no truth sits on."""
    scale = torch.logspace(-1, 1, F).double()
    x = (torch.randn(S, M, N, F, generator=g).double() * scale + 0.3 * scale).float().double()
    y = (torch.randn(S, N, F, generator=g).double() * scale).float().double()
    w = torch.rand(N, generator=g).float().double() * (torch.rand(N, generator=g) > 0.3)
    if N > 1:
        w[0] = 0.0
    mean, std = torch.randn(F, generator=g).float().double(), (torch.rand(F, generator=g) + 0.5).float().double()
    events = []
    for v, s, t in _events(E, F, [0.25, -0.5, 1.0, 0.0, -1.5, 2.0]):
        t = np.float32(t * float(scale[v]))
        while bool((x[..., v] == float(t)).any()) or bool((y[..., v] == float(t)).any()):
            t = np.nextafter(t, np.float32(np.inf))
        events.append((v, s, float(t)))
    return x, y, w, mean, std, _tables(events, LEVELS[:Q], M)


@pytest.mark.gpu
@pytest.mark.parametrize("M", MEMBERS)
def test_products_within_the_rounding_budget(dev, M):
    """Tier (b): random fp32 states with per-variable scales against the float64 reference, first order, U = 2^-24.
      prob     (float)c / (float)M, c exact: one correctly rounded division                      U prob
      Q_j      d = x_(hi) - x_(lo) (one rounding), Q = fma(g, d, x_(lo)) (one rounding):          e_q = U (g |x_(hi) - x_(lo)| + |Q_j|)
      quant    fma(Q, std, mean), one rounding:                                                   e_q std + U |quant|
      brier    p (1 + d1) - o (one rounding), its square, the weight: per node w (2 U p |p - o| + 4 U (p - o)^2), and the sum:
                                                                                                  sum_n w 2 U p |p - o| + (tau + 4 U) brier
      pinball  y - Q (e_q + one rounding), times q or fl(1 - q) (two roundings), the weight (one); a truth within e_q of Q_j may
               take the other branch, which moves rho by at most e_q:                            sum_n w e_q + (tau + 4 U) pinball
    tau = U (chunk nodes + chunks + 24), the additions of one output as in nlam_ens_scores' test.  Thresholds lie on no member and
    no truth (asserted), so the reliability table is exact; `below` may differ only by live nodes whose truth lies within e_q of
    the quantile."""
    g = torch.Generator().manual_seed(300 + M)
    for F, N, S, misalign, E, Q in _shapes():
        x, y, w, mean, std, tb = _random_case(g, M, F, N, S, E, Q)
        for v, t in zip(tb.var, tb.thr.double().tolist()):
            assert not bool((x[..., v] == t).any()) and not bool((y[..., v] == t).any())
        want = _reference(x, y, w, mean, std, tb)
        got = _products_run(dev, x, y, w, mean, std, tb, misalign)
        what = (M, F, N, S, misalign, E, Q)
        _check_budget(got, want, _bounds(x, y, w, std, tb, want), what)
        if E:
            assert torch.equal(got["rel_count"], want["rel_count"]) and torch.equal(got["rel_obs"], want["rel_obs"]), what
            assert bool((got["rel_count"].sum(-1) == int((w != 0).sum())).all()) and bool((got["rel_obs"] <= got["rel_count"]).all()), what


@pytest.mark.gpu
@pytest.mark.parametrize("M", MEMBERS)
def test_products_have_the_same_bits_from_run_to_run(dev, M):
    """No floating-point atomics and a fixed order of additions: a second launch on the same inputs gives every output's bits."""
    g = torch.Generator().manual_seed(500 + M)
    for F, N, S, misalign, E, Q in _shapes():
        x, y, w, mean, std, tb = _random_case(g, M, F, N, S, E, Q)
        got = _products_run(dev, x, y, w, mean, std, tb, misalign)
        again = _products_run(dev, x, y, w, mean, std, tb, misalign)
        assert set(got) == set(again) and all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got), (M, F, N, S, misalign, E, Q)


@pytest.mark.gpu
@pytest.mark.parametrize("M", MEMBERS)
def test_products_without_truth_are_the_same_fields(dev, M):
    """truth = NULL: only prob and quant are written (there is nothing else to pass), with the bits of the run with the truth."""
    g = torch.Generator().manual_seed(700 + M)
    for F, N, S, misalign, E, Q in _shapes():
        x, y, w, mean, std, tb = _random_case(g, M, F, N, S, E, Q)
        got = _products_run(dev, x, y, w, mean, std, tb, misalign)
        bare = _products_run(dev, x, None, w, mean, std, tb, misalign)
        assert set(bare) == set(got) & {"prob", "quant"}
        assert all(torch.equal(_bits(got[k]), _bits(bare[k])) for k in bare), (M, F, N, S, misalign, E, Q)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [3, 5, 64])
def test_a_nan_member_stays_a_nan_and_is_not_replaced_by_the_padding(dev, M):
    """The members are ordered as bit patterns: a positive NaN sorts above +inf, below the padding of the register array.  Level 1
    and a level halfway between the two largest order statistics then give NaN at the element that has the NaN member (a
    padding value in the NaN's place would make the latter +inf), level 0 the smallest member everywhere."""
    g = torch.Generator().manual_seed(M)
    S, N, F = 1, 9, 5
    x = torch.randn(S, M, N, F, generator=g).float().double()
    x[0, M // 2, 4, 2] = float("nan")
    w, mean, std = torch.ones(N).double(), torch.zeros(F).double(), torch.ones(F).double()
    tb = _tables([], [0.0, 1.0, (M - 1.5) / (M - 1)], M)
    assert tb.idx == [0, M - 1, M - 2] and tb.frac.tolist() == [0.0, 0.0, 0.5]
    got = _products_run(dev, x, None, w, mean, std, tb, False)["quant"]
    hit = torch.zeros(S, N, F, dtype=torch.bool)
    hit[0, 4, 2] = True
    assert bool(torch.isnan(got[:, 1][hit]).all()) and bool(torch.isnan(got[:, 2][hit]).all())
    assert not bool(torch.isnan(got[:, 1:][:, :, ~hit[0]]).any()) and not bool(torch.isnan(got[:, 0]).any())
    clean = torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x)
    assert torch.equal(got[:, 0].double(), clean.min(1).values)
    assert torch.equal(got[:, 1][~hit].double(), x.max(1).values[~hit])


# ---------------------------------------------------------------------------
# GPU: the engine on the golden cases' graphs and weights
# ---------------------------------------------------------------------------
PRODUCT_FIELDS = ("prob", "quantile", "brier", "rel_count", "rel_obs", "pinball", "below")
ENGINE_LEVELS = [0.0, 0.1, 0.5, 0.9, 1.0]


@pytest.fixture(scope="module", params=["efm_hi_81x30", "efm_ms_30x27", "efm_hi_constprior_81x30"])
def efm(request, dev, tmp_path_factory):
    from test_ensemble_forecast import _efm_world

    return _efm_world(request.param, dev, tmp_path_factory.mktemp("products_" + request.param))


def _snap(res):
    d = {k: v.clone() for k, v in res._asdict().items() if torch.is_tensor(v)}
    d.update({"products." + k: getattr(res.products, k).clone() for k in PRODUCT_FIELDS
              if res.products is not None and getattr(res.products, k) is not None})
    return d


def _same(a, b, keys=None):
    keys = list(keys or a)
    return set(a) == set(b) and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in keys)


def _midpoint_threshold(values, std, target):
    """The midpoint of two adjacent distinct pooled values whose gap exceeds 1e-3 std, nearest to the `target` fractile."""
    v = torch.unique(values.double().reshape(-1))   # sorted
    ok = torch.nonzero((v[1:] - v[:-1]) > 1e-3 * std).reshape(-1)
    assert ok.numel() > 0
    i = int(ok[torch.argmin((ok - target * (v.numel() - 1)).abs())])
    return float((v[i] + v[i + 1]) / 2)


@pytest.mark.gpu
def test_engine_products_against_the_reference_and_its_own_replay(dev, efm):
    """The engine's products on the members it returns.  Thresholds are midpoints of adjacent pooled member / truth values more
    than 1e-3 std apart, so nothing lies within rounding of one and prob, the reliability table and the Brier score's inputs are
    exact.  The reference interpolates the physical members: each is the standardised state through at most two roundings, 2 U
    (|member| + |mean|), on top of tier (b)'s e_q std + U |quant|."""
    from neural_lam_amd.forecast import EnsembleForecast, plan_forecast
    from test_ensemble_forecast import E_LEAD, E_TIMES, _dataset

    w, step = efm, efm.step
    S, M, starts = 2, 3, [1, 4]
    data = _dataset(w)
    names = step.state_var_names
    events = [(0, ">", 0.0), (0, "<", 0.0), (names[2], ">", 0.0), (4, "<", 0.0)]
    kw = dict(members=M, n_starts=S, seed=11, record_noise=True)
    ens = EnsembleForecast(step, data, E_LEAD, events=events, quantiles=ENGINE_LEVELS, **kw)
    plain = EnsembleForecast(step, data, E_LEAD, **kw)
    none = EnsembleForecast(step, data, E_LEAD, events=None, quantiles=None, **kw)
    assert none.launches_per_lead == plain.launches_per_lead and not hasattr(none, "prob") and none._pr is None
    assert ens.launches_per_lead == plain.launches_per_lead + 2   # the products and their finishing pass
    fields_only = EnsembleForecast(step, data, E_LEAD, events=events, members=M, n_starts=S, seed=11, verify=False)
    assert fields_only.launches_per_lead == EnsembleForecast(step, data, E_LEAD, members=M, n_starts=S, seed=11,
                                                             verify=False).launches_per_lead + 1
    first = _snap(ens.run(starts))
    base = _snap(plain.run(starts))
    assert plain.run(starts).products is None and _same(base, {k: v for k, v in first.items() if not k.startswith("products.")})
    # thresholds from the first run's members and the analysis
    off, _ = plan_forecast(E_TIMES, 1, 1, E_LEAD)
    t0 = torch.tensor(starts) + off - 1
    truth = torch.stack([w.state[t0.to(dev) + k + 1] for k in range(E_LEAD)], 1)   # (S, leads, N, F) physical
    std_truth = ((truth - step.state_mean) / step.state_std).cpu().double()        # the fp32 standardisation the head launch does
    sstd, smean = step.state_std.cpu().double(), step.state_mean.cpu().double()
    members = first["state"].view(S, M, E_LEAD, w.N, 5)
    thr = [_midpoint_threshold(torch.cat([members[..., v].reshape(-1), truth[..., v].reshape(-1)]).cpu(), float(sstd[v]), target)
           for v, target in ((0, 0.5), (0, 0.5), (2, 0.9), (4, 0.2))]
    graph = ens._graph
    ens.set_thresholds(thr)
    res = ens.run(starts)
    second = _snap(res)
    assert ens._graph is graph and len(ens._recorded) == 0                      # no new recording
    plain_keys = [k for k in first if not k.startswith("products.")]
    assert _same(first, second, plain_keys)                                     # the forecast itself has the same bits
    assert not torch.equal(first["products.prob"], second["products.prob"])
    assert _same(first, second, ["products.quantile", "products.pinball", "products.below"])
    pr = res.products
    assert pr.events == tuple((v, s, t) for (v, s), t in zip(((0, ">"), (0, "<"), (2, ">"), (4, "<")), thr)) and pr.levels == tuple(ENGINE_LEVELS)
    assert pr.prob.shape == (S, E_LEAD, 4, w.N) and pr.quantile.shape == (S, E_LEAD, 5, w.N, 5) and pr.brier.shape == (S, E_LEAD, 4)
    assert pr.rel_count.shape == (S, E_LEAD, 4, M + 1) == pr.rel_obs.shape and pr.pinball.shape == (S, E_LEAD, 5, 5) == pr.below.shape
    # the reference on the members
    wgt = step.interior_weight.cpu().double()
    tb = Tables(var=[0, 0, 2, 4], sense=[0, 1, 0, 1], thr=ens.event_thr.cpu(), idx=ens.q_index.cpu().tolist(), frac=ens.q_frac.cpu(),
                lev=ens.q_level.cpu())
    assert tb.idx == R.quantile_tables(ENGINE_LEVELS, M)[0]
    x_phys = res.members.cpu().double()
    for k in range(E_LEAD):
        x = (x_phys[:, :, k] - smean) / sstd
        y = std_truth[:, k]
        want = _reference(x, y, wgt, smean, sstd, tb)
        assert torch.equal(pr.prob[:, k].cpu(), want["count"].float() / float(M)), k
        assert torch.equal(pr.rel_count[:, k].cpu(), want["rel_count"]) and torch.equal(pr.rel_obs[:, k].cpu(), want["rel_obs"]), k
        b = _bounds(x, y, wgt, sstd, tb, want)
        err = (pr.brier[:, k].cpu().double() - want["brier"]).abs()
        assert bool((err <= b["brier"] * (1 + 1e-3)).all()), k
        xs = torch.sort(x_phys[:, :, k], dim=1).values
        trip = torch.stack([2 * U * (torch.maximum(xs[:, i].abs(), xs[:, min(i + 1, M - 1)].abs()) + smean.abs()) for i in tb.idx], 1)
        want_q = R.quantiles(x_phys[:, :, k], tb.idx, tb.frac.double().tolist(), dim=1)
        err = (pr.quantile[:, k].cpu().double() - want_q).abs()
        assert bool((err <= (b["quant"] + trip) * (1 + 1e-3)).all()), (k, float((err / (b["quant"] + trip)).max()))
        e_q = (b["quant"] + trip) / sstd
        err = (pr.pinball[:, k].cpu().double() - want["pinball"]).abs()
        assert bool((err <= ((wgt.view(1, 1, -1, 1) * e_q).sum(2) + (_tau(5, w.N) + 4 * U) * want["pinball"]) * (1 + 1e-3)).all()), k
        close = (((y[:, None] - want["quant_std"]).abs() <= e_q) & (wgt != 0).view(1, 1, -1, 1)).sum(2)
        assert bool(((pr.below[:, k].cpu() - want["below"]).abs() <= close).all()), k
    # the accessors
    assert torch.allclose(pr.brier_score(), pr.brier.mean(0)) and pr.brier_score().shape == (E_LEAD, 4)
    fc, freq, count = pr.reliability()
    assert torch.allclose(fc.cpu(), torch.arange(M + 1) / M) and torch.equal(count, pr.rel_count.sum(0))
    assert bool((count.sum(-1) == S * int((wgt != 0).sum())).all())
    filled = count > 0
    assert torch.equal(freq[filled], (pr.rel_obs.sum(0)[filled] / count[filled])) and bool(torch.isnan(freq[~filled]).all())
    assert torch.allclose(pr.pinball_loss(step.state_std), pr.pinball.mean(0) * step.state_std)
    cov = pr.coverage()
    assert cov.shape == (E_LEAD, 5, 5) and bool((cov[:, :-1] <= cov[:, 1:]).all()) and 0.0 <= float(cov.min()) and float(cov.max()) <= 1.0
    # graph replay against the same launches issued eagerly, products included; a shorter run is a prefix
    eager = EnsembleForecast(step, data, E_LEAD, events=list(pr.events), quantiles=ENGINE_LEVELS, use_graph=False, **kw)
    assert _same(second, _snap(eager.run(starts))) and eager.launches_per_lead is None
    short = _snap(ens.run(starts, leads=2))
    assert all(torch.equal(_bits(short[k]), _bits(second[k][:, :2])) for k in short if k != "noise")
    # the recording that reads given noise launches the products too
    given = _snap(ens.run(starts, latent_noise=second["noise"]))
    assert _same(second, given) and len(ens._recorded) == 1 and ens._graph is not graph
    for t in (ens.prob, ens.quantile, ens.brier, ens.pinball):
        t.fill_(float("nan"))
    assert _same(second, _snap(ens.run(starts, latent_noise=second["noise"])))
    # without verification: the same fields, no scores
    fields_only.set_thresholds(thr)
    bare = fields_only.run(starts).products
    assert bare.brier is None and bare.quantile is None and bare.below is None and bare.rel_count is None
    assert torch.equal(_bits(bare.prob), _bits(second["products.prob"]))
    with pytest.raises(ValueError, match="verify"):
        bare.brier_score()
    with pytest.raises(ValueError, match="thresholds"):
        ens.set_thresholds(thr[:2])


@pytest.mark.gpu
def test_a_deterministic_predictor_gives_certain_products(dev, tmp_path):
    """Identical members: every probability is 0 or 1, and every quantile is the member -- Q_j = fma(g, 0, x) = x, so the Q fields
    have the same bits: one fma (one rounding, U |member|) from the standardised state x, where the member field is x std + mean
    through at most two (U |x std| + U |member| <= U (2 |member| + |mean|)): within U (3 |member| + |mean|) of it."""
    from neural_lam_amd.forecast import EnsembleForecast
    from test_ensemble_forecast import _dataset, _graph_lam_step

    w = _graph_lam_step(dev, tmp_path)
    S, M, LEADS = 2, 3, 3
    ens = EnsembleForecast(w.step, _dataset(w), LEADS, members=M, n_starts=S, events=[(1, ">", 0.1), (1, "<", 0.1), (3, ">", -0.4)],
                           quantiles=[0.0, 0.37, 1.0])
    res = ens.run([1, 5])
    pr = res.products
    assert bool(((pr.prob == 0) | (pr.prob == 1)).all()) and 0 < float(pr.prob.mean()) < 1
    assert bool((pr.rel_count[..., 1:M] == 0).all()) and bool((pr.rel_count.sum(-1) == int((w.step.interior_weight != 0).sum())).all())
    assert torch.equal(_bits(pr.quantile[:, :, 0]), _bits(pr.quantile[:, :, 1])) and torch.equal(_bits(pr.quantile[:, :, 0]), _bits(pr.quantile[:, :, 2]))
    member = res.members[:, 0].double()
    bound = U * (3 * member.abs() + w.step.state_mean.double().abs())
    assert bool(((pr.quantile[:, :, 0].double() - member).abs() <= bound * (1 + 1e-3)).all())
    # prob is the indicator of the member itself wherever the member is clear of the threshold
    x1 = res.members[:, 0, :, :, 1]
    clear = (x1 - 0.1).abs() > 1e-3 * float(w.step.state_std[1])
    assert torch.equal(pr.prob[:, :, 0][clear], (x1 > 0.1).float()[clear]) and torch.equal(pr.prob[:, :, 1][clear], (x1 < 0.1).float()[clear])
