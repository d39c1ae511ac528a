"""Neighbourhood probabilities and the fractions skill score of a sampled ensemble (nlam_ens_neighbourhood;
EnsembleForecast(events=..., neighbourhoods=..., grid_shape=...)).  Without a GPU: the C-ABI (exports, struct layout, every argument
check, the workspace function), the brute-force reference against hand-computed cases, and the engine's host validation.  On the
GPU: the launch against the reference -- an exact tier on integers, a budget tier on random states, run-to-run bit identity,
truth = NULL, a lead past the end, the cross-check with nlam_ens_products at radius 0 -- and the engine on the Graph-EFM golden
cases: graph against eager, launch counts, set_radii / set_thresholds, the reference applied to the members, given noise, and a
deterministic predictor with one member."""
import ctypes as C
import subprocess
import types

import numpy as np
import pytest
import torch

import ens_products_ref as PR
import neighbourhood_ref as R
from conftest import ROOT
from neural_lam_amd import _lib as L

U = 2.0 ** -24   # fp32 unit roundoff
NEW_EXPORTS = ["nlam_ens_neighbourhood", "nlam_ens_neighbourhood_workspace_floats"]
POINTERS = ("prev", "truth", "row_weight", "lead", "event_var", "event_sense", "event_thr", "radius", "nprob", "fbs", "fbs_ref", "workspace")
LAUNCHES = 5   # count, rows, cols, eval and, with the truth, finish -- for every S, M, E, W and radius


# ---------------------------------------------------------------------------
# CPU: the C-ABI
# ---------------------------------------------------------------------------
def test_neighbourhood_symbols_are_exported_and_the_struct_matches_c_layout(tmp_path):
    import re

    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert declared == set(L.EXPORTS)
    assert lib.nlam_abi_version() == 8 == L.ABI_VERSION
    fields = [name for name, _ in L.EnsNeighbourhood._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
                   'int main(){printf("%zu", sizeof(nlam_ens_neighbourhood_t));\n'
                   + "".join(f'printf(" %zu", offsetof(nlam_ens_neighbourhood_t, {f}));\n' for f in fields)
                   + 'printf(" %d %d %d %d\\n", NLAM_ABI_VERSION, NLAM_ENS_MAX_MEMBERS, NLAM_ENS_MAX_EVENTS, NLAM_NBR_MAX_SCALES);'
                     ' return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == ([C.sizeof(L.EnsNeighbourhood)] + [getattr(L.EnsNeighbourhood, f).offset for f in fields]
                   + [8, L.ENS_MAX_MEMBERS, L.ENS_MAX_EVENTS, L.NBR_MAX_SCALES])
    assert L.NBR_MAX_SCALES == 8


def test_neighbourhood_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    ws = lib.nlam_ens_neighbourhood_workspace_floats
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    S, M, NX, NY, F, LEAD, E, W = 2, 3, 7, 41, 5, 4, 3, 5
    N = NX * NY
    nws = ws(S, M, NX, NY, F, E, W)
    # the live table and C and O of every (start, event), then two sums per (start, event, scale) and 256 nodes
    assert nws == N * (1 + 2 * S * E) + 2 * S * E * W * -(-N // 256)
    assert ws(1, 1, 1, 1, 1, 1, 1) == 3 + 2
    for bad in ((0, M, NX, NY, F, E, W), (S, 0, NX, NY, F, E, W), (S, M, 0, NY, F, E, W), (S, M, NX, 0, F, E, W), (S, M, NX, NY, 0, E, W),
                (S, M, NX, NY, F, 0, W), (S, M, NX, NY, F, E, 0), (S, M, NX, -3, F, E, W)):
        assert ws(*bad) == -1, bad
    for bad in ((S, 65, NX, NY, F, E, W), (S, M, NX, NY, 257, E, W), (S, M, NX, NY, F, 33, W), (S, M, NX, NY, F, E, 9), (65536, M, NX, NY, F, E, W),
                (S, 1, 4096, 4097, F, E, W), (S, 64, 512, 513, F, E, W), (S, 2, 1 << 30, 1 << 30, F, E, W), (S, 1, 1, (1 << 24) + 1, F, E, W)):
        assert ws(*bad) == -2, bad
    # at the maxima: members * nodes = 2^24 exactly is served
    assert ws(65535, 64, 512, 512, 256, 32, 8) == (1 << 18) * (1 + 2 * 65535 * 32) + 2 * 65535 * 32 * 8 * 1024
    assert ws(1, 1, 1 << 24, 1, 1, 1, 1) == 3 * (1 << 24) + 2 * (1 << 16)

    def args(**kw):
        p = L.EnsNeighbourhood()
        for name in POINTERS:
            setattr(p, name, fake)
        p.workspace_floats, p.starts, p.members, p.nx, p.ny, p.d_state, p.max_lead, p.events, p.scales = nws, S, M, NX, NY, F, LEAD, E, W
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    call = lib.nlam_ens_neighbourhood
    assert call(None, None) == -1
    einval = [{name: None} for name in ("prev", "row_weight", "lead", "event_var", "event_sense", "event_thr", "radius", "nprob", "workspace")]
    einval += [dict(starts=0), dict(members=0), dict(nx=0), dict(ny=0), dict(d_state=0), dict(max_lead=0), dict(events=0), dict(scales=0),
               dict(events=-1), dict(scales=-1), dict(workspace_floats=nws - 1)]
    einval += [dict(fbs=None), dict(fbs_ref=None)]                                                        # truth without both sums
    einval += [dict(truth=None), dict(truth=None, fbs=None), dict(truth=None, fbs_ref=None)]              # a sum without truth
    for kw in einval:
        assert call(args(**kw), None) == -1, kw
    big = 1 << 50
    for kw in (dict(members=65), dict(d_state=257), dict(starts=65536), dict(events=33), dict(scales=9), dict(members=1, nx=4096, ny=4097),
               dict(members=64, nx=512, ny=513), dict(nx=1 << 30, ny=1 << 30)):
        assert call(args(workspace_floats=big, **kw), None) == -2, kw
    # without truth and without the sums everything else is still checked
    assert call(args(truth=None, fbs=None, fbs_ref=None, starts=65536, workspace_floats=big), None) == -2
    assert call(args(truth=None, fbs=None, fbs_ref=None, workspace_floats=nws - 1), None) == -1


# ---------------------------------------------------------------------------
# CPU: the reference
# ---------------------------------------------------------------------------
def _t(v):
    return torch.tensor(v, dtype=torch.float64)


def test_neighbourhood_reference_against_hand_computed_cases():
    # the 1 x 5 grid of the design: one member in the event at j = 1, the truth at j = 3, all live, w = 1/5
    x = _t([0.0, 1.0, 0.0, 0.0, 0.0]).view(1, 1, 5, 1)
    y = _t([0.0, 0.0, 0.0, 1.0, 0.0]).view(1, 5, 1)
    w = torch.full((5,), 0.2, dtype=torch.float64)
    r = R.ens_neighbourhood(x, y, w, [0], [0], [0.5], [0, 1, 2, 4, 9], 1, 5)
    assert r["A"].tolist() == [[1] * 5, [2, 3, 3, 3, 2], [3, 4, 5, 4, 3], [5] * 5, [5] * 5]
    assert r["SC"][0, 0].tolist() == [[0, 1, 0, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 1, 0], [1] * 5, [1] * 5]
    assert r["SO"][0, 0].tolist() == [[0, 0, 0, 1, 0], [0, 0, 1, 1, 1], [0, 1, 1, 1, 1], [1] * 5, [1] * 5]
    f = R.fss(r["fbs"], r["fbs_ref"])[0]
    want = [0.0, 4 / 17, 1 - (2 / 9) / (2 / 9 + 1 / 4 + 2 / 25), 1.0, 1.0]
    assert all(abs(float(a) - b) < 1e-14 for a, b in zip(f, want)), f.tolist()
    # r = 1 by hand: fbs = (1/4 + 1/9 + 0 + 1/9 + 1/4) / 5, fbs_ref = (1/4 + 1/9 + 2/9 + 1/9 + 1/4) / 5
    assert abs(float(r["fbs"][0, 0, 1]) - 13 / 90) < 1e-15 and abs(float(r["fbs_ref"][0, 0, 1]) - 17 / 90) < 1e-15
    # a negative radius acts as 0
    assert torch.equal(R.ens_neighbourhood(x, y, w, [0], [0], [0.5], [-3], 1, 5)["SC"], r["SC"][:, :, :1])
    # shifted slices against explicit windows, a 4 x 6 grid
    g = torch.Generator().manual_seed(3)
    a = torch.randint(0, 5, (4, 6), generator=g)
    for rad in (0, 1, 2, 3, 5, 40):
        got = R.window_sums(a, rad)
        assert all(int(got[i, j]) == R.window_sum_explicit(a, rad, i, j) for i in range(4) for j in range(6)), rad
    # 3 x 3, M = 2, only the centre and one corner live: a dead node inside a window is left out of all three sums, and a window
    # with no live node gives NaN.  Members in the event everywhere (C = 2), the truth in it everywhere.
    x = torch.ones(1, 2, 9, 1, dtype=torch.float64)
    y = torch.ones(1, 9, 1, dtype=torch.float64)
    w = _t([0.0, 0, 0, 0, 1.0, 0, 0, 0, 0.5])
    r = R.ens_neighbourhood(x, y, w, [0], [0], [0.5], [0, 1, 2], 3, 3)
    assert r["A"].tolist() == [[0, 0, 0, 0, 1, 0, 0, 0, 1], [1, 1, 1, 1, 2, 2, 1, 2, 2], [2] * 9]
    assert r["SC"][0, 0].tolist() == [[0, 0, 0, 0, 2, 0, 0, 0, 2], [2, 2, 2, 2, 4, 4, 2, 4, 4], [4] * 9]
    assert r["SO"][0, 0, 1].tolist() == r["A"][1].tolist()
    assert torch.isnan(r["nprob"][0, 0, 0]).tolist() == [True, True, True, True, False, True, True, True, False]
    assert r["nprob"][0, 0, 1].tolist() == [1.0] * 9 and not bool(torch.isnan(r["nprob"][0, 0, 1:]).any())
    assert r["fbs"].abs().max().item() == 0.0 and r["fbs_ref"][0, 0].tolist() == [3.0, 3.0, 3.0]   # (1 + 1) (1 + 0.5)
    # the whole grid dead: every nprob is NaN, nothing is summed, FSS is NaN
    r = R.ens_neighbourhood(x, y, torch.zeros(9, dtype=torch.float64), [0], [0], [0.5], [0, 7], 3, 3)
    assert bool(torch.isnan(r["nprob"]).all()) and r["fbs_ref"].abs().max().item() == 0.0 and bool(torch.isnan(R.fss(r["fbs"], r["fbs_ref"])).all())
    # r = 0 is the point product: count / M and the Brier sum of ens_products_ref (ties on the threshold count in neither sense)
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-2, 3, (2, 3, 12, 2), generator=g).double()
    y = torch.randint(-2, 3, (2, 12, 2), generator=g).double()
    w = torch.tensor([0.0, 0.5, 1.0, 2.0])[torch.randint(0, 4, (12,), generator=g)].double()
    var, sense, thr = [0, 0, 1, 1], [0, 1, 0, 1], [0.0, 0.5, -1.0, 1.0]
    r = R.ens_neighbourhood(x, y, w, var, sense, thr, [0], 3, 4)
    pr = PR.ens_products(x, y, w, var, sense, thr)
    live = w != 0
    assert torch.equal(r["nprob"][:, :, 0][:, :, live], (pr["count"].float() / 3.0)[:, :, live])
    assert torch.equal(r["SC"][:, :, 0][:, :, live], pr["count"][:, :, live]) and bool(torch.isnan(r["nprob"][:, :, 0][:, :, ~live]).all())
    assert bool(((r["fbs"][:, :, 0] - pr["brier"]).abs() <= 1e-14).all())


def test_engine_validates_neighbourhoods_on_the_host():
    from neural_lam_amd.forecast import EnsembleForecast, parse_neighbourhoods

    assert parse_neighbourhoods(None, None, 0, 4) == ([], None)
    assert parse_neighbourhoods([0, 1, 2, 5, 10], (3, 4), 2, 4, 12) == ([0, 1, 2, 5, 10], (3, 4))
    assert parse_neighbourhoods([np.int64(3), 2.0], [3, 4], 1, 4) == ([3, 2], (3, 4))
    # the checks come before anything else is read
    step = types.SimpleNamespace(state_var_names=["t2m", "u10", "v10"], state_mean=torch.zeros(3), interior_weight=torch.ones(12))
    ev = [("t2m", ">", 0.0)]
    bad = [dict(neighbourhoods=[0, 1], grid_shape=(3, 4)),                                    # without events
           dict(events=ev, neighbourhoods=[0, 1]),                                            # without the grid shape
           dict(events=ev, neighbourhoods=[0, 1], grid_shape=(3, 5)), dict(events=ev, neighbourhoods=[0, 1], grid_shape=(12,)),
           dict(events=ev, neighbourhoods=[0, 1], grid_shape=(0, 12)), dict(events=ev, neighbourhoods=[0, 1], grid_shape=(-3, -4)),
           dict(events=ev, neighbourhoods=[0, -1], grid_shape=(3, 4)), dict(events=ev, neighbourhoods=[1.5], grid_shape=(3, 4)),
           dict(events=ev, neighbourhoods=["a"], grid_shape=(3, 4)), dict(events=ev, neighbourhoods=[True], grid_shape=(3, 4)),
           dict(events=ev, neighbourhoods=[], grid_shape=(3, 4)),
           dict(events=ev, neighbourhoods=list(range(9)), grid_shape=(3, 4))]
    for kw in bad:
        with pytest.raises(ValueError, match="EnsembleForecast"):
            EnsembleForecast(step, None, 3, members=4, **kw)
    large = types.SimpleNamespace(state_var_names=["t2m"], state_mean=torch.zeros(1))
    with pytest.raises(ValueError, match="2\\^24"):
        EnsembleForecast(large, None, 3, members=4, events=ev, neighbourhoods=[1], grid_shape=(2048, 2049))
    with pytest.raises(ValueError, match="Forecast needs"):   # the maxima themselves pass on to the next check
        EnsembleForecast(large, None, 3, members=4, events=ev, neighbourhoods=list(range(8)), grid_shape=(2048, 2048))


# ---------------------------------------------------------------------------
# GPU: nlam_ens_neighbourhood at the C-ABI
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


POISON = -7.0   # no output is negative, and NaN is an output


def _nbr_run(dev, x, y, w, events, radii, nx, ny, misalign, K=1, LEAD=3):
    """One nlam_ens_neighbourhood launch at lead K on x (S, M, N, F), y (S, N, F) or None; events = (var, sense, fp32 thr).  The
    outputs of slot K, every other slot checked to keep its poison (all of them when K >= LEAD: None is returned)."""
    lib = L.load()
    put = _misaligned if misalign else (lambda t: t)
    S, M, N, F = x.shape
    var, sense, thr = events
    E, W = len(var), len(radii)
    prev = put(x.reshape(S * M, N, F).float().to(dev))
    truth = None
    if y is not None:
        truth = torch.full((S, M, N, F), float("nan"))
        truth[:, 0] = y.float()   # the truth of member 0 is used
        truth = put(truth.reshape(S * M, N, F).to(dev))
    full = lambda *shape: put(torch.full(shape, POISON, device=dev))   # noqa: E731
    o = types.SimpleNamespace(nprob=full(S, LEAD, E, W, N))
    if y is not None:
        o.fbs, o.fbs_ref = full(S, LEAD, E, W), full(S, LEAD, E, W)
    nws = int(lib.nlam_ens_neighbourhood_workspace_floats(S, M, nx, ny, F, E, W))
    assert nws > 0
    ws = put(torch.full((nws,), float("nan"), device=dev))
    lead = torch.full((1,), K, dtype=torch.int32, device=dev)
    i32 = lambda v: put(torch.tensor(v, dtype=torch.int32, device=dev))   # noqa: E731
    keep = [put(w.float().to(dev)), i32(var), i32(sense), put(thr.float().to(dev)), i32(radii)]
    p = L.EnsNeighbourhood()
    p.prev, p.truth, p.lead, p.workspace, p.workspace_floats = _ptr(prev), _ptr(truth), _ptr(lead), _ptr(ws), nws
    p.row_weight, p.event_var, p.event_sense, p.event_thr, p.radius = (_ptr(t) for t in keep)
    for name, t in vars(o).items():
        setattr(p, name, _ptr(t))
    p.starts, p.members, p.nx, p.ny, p.d_state, p.max_lead, p.events, p.scales = S, M, nx, ny, F, LEAD, E, W
    L.check(lib.nlam_ens_neighbourhood(C.byref(p), _stream()), "nlam_ens_neighbourhood")
    torch.cuda.synchronize()
    assert int(lead) == K   # only read
    others = [k for k in range(LEAD) if k != K]
    got = {}
    for name, t in vars(o).items():
        assert bool((t[:, others] == POISON).all()), name
        if K < LEAD:
            got[name] = t[:, K].cpu().clone()
    return got if K < LEAD else None


RADII = [0, 1, 2, 7, 300]
MEMBERS = [1, 2, 3, 5, 33, 64]
# the issue's grids; then the edges of the scans and of the evaluation, which depend on the grid alone: 4, 8, 16, 32, 64 lanes per
# row and rows of more than one 64-word step (ny = 4, 5, 8, 9, 15, 16, 17, 32, 33, 63 .. 65, 128, 129), eight rows per step of the
# column pass (nx = 7, 8, 9, 16, 17), 256 nodes per workgroup of the evaluation (255, 256, 257 nodes).  The edges of the counting
# pass depend on F and M: _count_edge_grids.
GRIDS = [(1, 1), (1, 7), (7, 1), (3, 5), (5, 64), (4, 65), (3, 257), (70, 3), (30, 27),
         (8, 4), (9, 8), (16, 9), (17, 15), (3, 17), (16, 16), (8, 32), (7, 33), (4, 63), (2, 128), (2, 129), (1, 257), (257, 1)]


def _chunk_nodes(F):
    """Nodes per workgroup of the counting pass: fc_chunk_nodes of nlam_forecast.inc, 4096 elements of whole nodes rounded up to a
    multiple of 4 nodes (1368 at F = 3, 240 at F = 17, 16 at F = 256)."""
    return max(4, (4096 // F + 3) // 4 * 4)


def _piece_nodes(F, M):
    """Nodes per LDS piece of the counting pass: nbr_tile_nodes of nlam_ens_neighbourhood.inc -- what 16384 words less the 96 of
    the tables hold of M + 1 rows, a multiple of 4 where there are that many, at least 1 and at most the chunk."""
    n = (16384 - 96) // ((M + 1) * F)
    if n >= 4:
        n &= ~3
    return min(max(n, 1), _chunk_nodes(F))


def _grid_of(nodes):
    """The most square nx x ny with that many nodes (1 x nodes for a prime)."""
    nx = max(d for d in range(1, int(nodes ** 0.5) + 1) if nodes % d == 0)
    return nx, nodes // nx


def _count_edge_grids(M):
    """(F, nx, ny) with one node less than, exactly and one node more than a counting chunk and, where it is smaller, an LDS piece,
    at F = 3, 17 and 256.  At F = 256 a piece holds fewer than 4 nodes from M = 33 on, is one node at M = 64 -- where that node's
    65 rows need 66 944 bytes of LDS, above the 64 KiB a launch gets unasked -- and never starts on a 16-byte boundary when the
    rows are misaligned; (3, 7) there spans two chunks and several pieces for every M."""
    out = []
    for F in (3, 17, 256):
        cn, tn = _chunk_nodes(F), _piece_nodes(F, M)
        for n in sorted({cn - 1, cn, cn + 1} | ({tn - 1, tn, tn + 1} if tn < cn else set())):
            if n >= 1:
                out.append((F, *_grid_of(n)))
    return out + [(256, 3, 7)]


def _mask(kind, nx, ny, g):
    """Live masks: all live; a frame (the border dead, the interior live); random with a dead 5 x 5 patch, so that the windows of
    radius <= 2 around its centre hold no live node (where the grid is smaller, the patch is cut to it)."""
    m = torch.ones(nx, ny, dtype=torch.bool)
    if kind == "frame":
        m[0], m[-1], m[:, 0], m[:, -1] = False, False, False, False
    elif kind == "random":
        m = torch.rand(nx, ny, generator=g) > 0.3
        i0, j0 = max(0, nx // 2 - 2), max(0, ny // 2 - 2)
        m[i0:i0 + 5, j0:j0 + 5] = False
    return m.reshape(-1)


def _weights(kind, nx, ny, g):
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (nx * ny,), generator=g)].double() * _mask(kind, nx, ny, g)


def _cases(M):
    """(nx, ny, F, S, misaligned, mask).  GRIDS at F = 3 with S in {1, 3}, aligned and misaligned; the counting pass's edges for
    this M with (S = 3, aligned) -- where M N F is no multiple of 4 the starts differ in alignment, so the workgroups decide
    differently about 16-byte loads -- and (S = 1, misaligned).  The three masks go round: every pairing meets every mask."""
    kinds = ("all", "frame", "random")
    i = 0
    for nx, ny in GRIDS:
        for S, misalign in ((1, False), (3, True), (3, False), (1, True)):
            yield nx, ny, 3, S, misalign, kinds[i % 3]
            i += 1
    for F, nx, ny in _count_edge_grids(M):
        for S, misalign in ((3, False), (1, True)):
            yield nx, ny, F, S, misalign, kinds[i % 3]
            i += 1


def _events(F, thresholds):
    """Four events on three variables (the first, the second and the last), two of them on one variable with both senses; (var,
    sense, fp32 thresholds)."""
    var, sense = [0, 0, 1 % F, F - 1], [0, 1, 0, 1]
    return var, sense, torch.tensor(thresholds, dtype=torch.float64).float()


def _budget(ref, w):
    """The budgets of fbs and fbs_ref (test_neighbourhood_within_the_rounding_budget's docstring)."""
    N = w.numel()
    lv = (w != 0).view(1, 1, 1, N)
    zero = torch.zeros((), dtype=torch.float64)
    p, o = torch.where(lv, ref["p"], zero), torch.where(lv, ref["o"], zero)
    d = (p - o).abs()
    wd = w.double().view(1, 1, 1, N)
    b_fbs = (wd * (2 * U * (p + o) * d + 3 * U * d * d)).sum(-1) + (N + 8) * U * ref["fbs"]
    b_ref = (wd * 3 * U * (p * p + o * o)).sum(-1) + (N + 8) * U * ref["fbs_ref"]
    return b_fbs, b_ref


def _check(got, ref, w, what, scores=True):
    nan = torch.isnan(got["nprob"])
    assert torch.equal(nan, (ref["A"] == 0).view(1, 1, *ref["A"].shape).expand_as(nan)), what   # NaN where A = 0 and nowhere else
    assert torch.equal(_bits(got["nprob"])[~nan], _bits(ref["nprob"])[~nan]), what               # bit for bit
    if scores:
        b_fbs, b_ref = _budget(ref, w)
        for k, b in (("fbs", b_fbs), ("fbs_ref", b_ref)):
            err = (got[k].double() - ref[k]).abs()
            print(what, k, "worst error / budget", float((err / b.clamp_min(1e-300)).max()))
            assert bool((err <= b).all()), (what, k, float((err / b.clamp_min(1e-300)).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("M", MEMBERS)
def test_neighbourhood_exact_on_integers(dev, M):
    """The exact tier.  Integer members and truths in [-2, 2], thresholds on half-integers and on integers (ties, which count in
    neither sense).  A, SC and SO are integers, M A <= 2^24, so nprob = (float)SC / (float)(M A) is one correctly rounded division
    of two exact operands: it must equal the reference's fp32 division bit for bit, with NaN where the reference has A = 0 and
    nowhere else.  The two sums are held to the budget of the next test."""
    g = torch.Generator().manual_seed(900 + M)
    seen = dict(tie=False, dead_window=False, whole_grid=False, nan=False)
    assert _chunk_nodes(17) == 240 and _piece_nodes(17, 64) == 12 and _piece_nodes(3, 64) == 80 and _piece_nodes(256, 64) == 1
    for nx, ny, F, S, misalign, kind in _cases(M):
        N = nx * ny
        x = torch.randint(-2, 3, (S, M, N, F), generator=g).double()
        y = torch.randint(-2, 3, (S, N, F), generator=g).double()
        w = _weights(kind, nx, ny, g)
        ev = _events(F, [0.5, 0.0, -0.5, 1.0])
        ref = R.ens_neighbourhood(x, y, w, *ev, RADII, nx, ny)
        got = _nbr_run(dev, x, y, w, ev, RADII, nx, ny, misalign)
        _check(got, ref, w, (M, nx, ny, F, S, misalign, kind))
        seen["tie"] |= bool((x[..., 0] == 0.0).any()) and bool((y[..., 0] == 0.0).any())
        seen["dead_window"] |= bool((ref["A"][2] == 0).any()) and bool((ref["A"][2] > 0).any())   # radius 2, beside live windows
        seen["whole_grid"] |= bool((ref["A"][4] == int((w != 0).sum())).all())
        seen["nan"] |= bool(torch.isnan(got["nprob"]).any())
    assert all(seen.values()), seen


def _random_case(g, M, F, N, S):
    """Random fp32 states with per-variable scales and thresholds moved to the next fp32 value that no member and no truth sits
    on (as test_ensemble_products._random_case does)."""
    scale = torch.logspace(-1, 1, F).double()
    x = (torch.randn(S, M, N, F, generator=g).double() * scale + 0.3 * scale).float().double()
    y = (torch.randn(S, N, F, generator=g).double() * scale).float().double()
    var, sense, _ = _events(F, [0.0] * 4)
    thr = []
    for v, t in zip(var, [0.25, -0.5, 1.0, 0.0]):
        t = np.float32(t * float(scale[v]))
        while bool((x[..., v] == float(t)).any()) or bool((y[..., v] == float(t)).any()):
            t = np.nextafter(t, np.float32(np.inf))
        thr.append(float(t))
    return x, y, (var, sense, torch.tensor(thr, dtype=torch.float64).float())


BUDGET_CASES = [(30, 27, 5, 3, True, "random"), (5, 64, 5, 1, False, "frame"), (3, 257, 1, 3, True, "all"), (17, 15, 17, 1, True, "random"),
                (70, 3, 5, 1, False, "all"), (1, 7, 3, 3, False, "all")]


@pytest.mark.gpu
@pytest.mark.parametrize("M", MEMBERS)
def test_neighbourhood_within_the_rounding_budget(dev, M):
    """The budget tier: random fp32 states against the float64 reference, first order, U = 2^-24.  The thresholds lie on no member
    and no truth, so C and O, and with them A, SC, SO and nprob, are still exact.  Per live node, with p = SC / (M A) and
    o = SO / A the exact fractions: the kernel's p and o carry one rounding each (U p, U o), so their difference is off by U (p + o)
    plus its own rounding U |p - o|; squaring doubles the relative error and rounds once more, the weight rounds once:
        |term - w (p - o)^2|      <= w [2 U (p + o) |p - o| + 3 U (p - o)^2]      (+ U w (p - o)^2, taken from the last term below)
        |term - w (p^2 + o^2)|    <= w 3 U (p^2 + o^2)                             (+ 2 U of it for the addition and the weight)
    Adding N non-negative terms in any order is within (N - 1) U of their sum, which needs nothing from the kernel's geometry:
        fbs      sum_n w_n [2 U (p + o) |p - o| + 3 U (p - o)^2] + (N + 8) U fbs
        fbs_ref  sum_n w_n 3 U (p^2 + o^2) + (N + 8) U fbs_ref
    the 9 U left over in the last term covering the roundings named in brackets."""
    g = torch.Generator().manual_seed(1300 + M)
    for nx, ny, F, S, misalign, kind in BUDGET_CASES:
        N = nx * ny
        x, y, ev = _random_case(g, M, F, N, S)
        for v, t in zip(ev[0], ev[2].double().tolist()):
            assert not bool((x[..., v] == t).any()) and not bool((y[..., v] == t).any())
        w = torch.rand(N, generator=g).float().double() * _mask(kind, nx, ny, g)
        ref = R.ens_neighbourhood(x, y, w, ev[0], ev[1], ev[2].double().tolist(), RADII, nx, ny)
        got = _nbr_run(dev, x, y, w, ev, RADII, nx, ny, misalign)
        _check(got, ref, w, (M, nx, ny, F, S, misalign, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 5, 64])
def test_neighbourhood_bits_repeat_and_need_no_truth_and_stop_at_the_last_lead(dev, M):
    """A second launch gives every output's bits (no floating-point atomics, a fixed order of additions); truth = NULL gives the
    same nprob bits and there is no sum to write; with *lead >= max_lead nothing is written."""
    g = torch.Generator().manual_seed(1700 + M)
    for nx, ny, F, S, misalign, kind in BUDGET_CASES:
        N = nx * ny
        x, y, ev = _random_case(g, M, F, N, S)
        w = torch.rand(N, generator=g).float().double() * _mask(kind, nx, ny, g)
        got = _nbr_run(dev, x, y, w, ev, RADII, nx, ny, misalign)
        again = _nbr_run(dev, x, y, w, ev, RADII, nx, ny, misalign)
        what = (M, nx, ny, F, S, misalign, kind)
        assert set(got) == set(again) == {"nprob", "fbs", "fbs_ref"} and all(torch.equal(_bits(got[k]), _bits(again[k])) for k in got), what
        bare = _nbr_run(dev, x, None, w, ev, RADII, nx, ny, misalign)
        assert set(bare) == {"nprob"} and torch.equal(_bits(bare["nprob"]), _bits(got["nprob"])), what
        for K in (3, 4):
            assert _nbr_run(dev, x, y, w, ev, RADII, nx, ny, misalign, K=K, LEAD=3) is None


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 3, 64])
def test_radius_zero_is_the_point_product_of_nlam_ens_products(dev, M):
    """On the inputs of nlam_ens_products, radius 0: nprob of a live node is prob bit for bit -- the same division (float)c /
    (float)M --, and fbs is the Brier sum within the two launches' budgets (both are within theirs of the same float64 sum)."""
    from test_ensemble_products import Tables, _bounds, _products_run

    g = torch.Generator().manual_seed(2100 + M)
    for nx, ny, F, S, misalign, kind in BUDGET_CASES:
        N = nx * ny
        x, y, ev = _random_case(g, M, F, N, S)
        w = torch.rand(N, generator=g).float().double() * _mask(kind, nx, ny, g)
        mean, std = torch.zeros(F, dtype=torch.float64), torch.ones(F, dtype=torch.float64)
        tb = Tables(var=ev[0], sense=ev[1], thr=ev[2], idx=[], frac=torch.zeros(0), lev=torch.zeros(0))
        point = _products_run(dev, x, y, w, mean, std, tb, misalign)
        got = _nbr_run(dev, x, y, w, ev, [0], nx, ny, misalign)
        live = w != 0
        what = (M, nx, ny, F, S, misalign, kind)
        assert torch.equal(_bits(got["nprob"][:, :, 0][:, :, live]), _bits(point["prob"][:, :, live])), what
        assert bool(torch.isnan(got["nprob"][:, :, 0][:, :, ~live]).all()), what
        want = PR.ens_products(x, y, w, ev[0], ev[1], ev[2].double().tolist())
        ref = R.ens_neighbourhood(x, y, w, ev[0], ev[1], ev[2].double().tolist(), [0], nx, ny)
        both = _bounds(x, y, w, std, tb, want)["brier"] + _budget(ref, w)[0][:, :, 0]
        err = (got["fbs"][:, :, 0].double() - point["brier"].double()).abs()
        assert bool((err <= both).all()), (what, float((err / both.clamp_min(1e-300)).max()))


# ---------------------------------------------------------------------------
# GPU: the engine on the golden cases' graphs and weights
# ---------------------------------------------------------------------------
NBR_FIELDS = ("prob", "brier", "rel_count", "rel_obs", "nprob", "fbs", "fbs_ref")
ENGINE_RADII = [0, 1, 2, 5, 10]


@pytest.fixture(scope="module", params=["efm_hi_81x30", "efm_ms_30x27", "efm_hi_constprior_81x30"])
def efm(request, dev, tmp_path_factory):
    from test_ensemble_forecast import _efm_world

    return _efm_world(request.param, dev, tmp_path_factory.mktemp("neighbourhood_" + request.param))


def _snap(res):
    d = {k: v.clone() for k, v in res._asdict().items() if torch.is_tensor(v)}
    d.update({"products." + k: getattr(res.products, k).clone() for k in NBR_FIELDS
              if res.products is not None and getattr(res.products, k) is not None})
    return d


def _same(a, b, keys=None):
    keys = list(keys or a)
    return set(a) == set(b) and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in keys)


@pytest.mark.gpu
def test_engine_neighbourhoods_against_the_reference_and_its_own_replay(dev, efm):
    """The engine's neighbourhood products on the members it returns.  Thresholds are midpoints of adjacent pooled member / truth
    values more than 1e-3 std apart (test_ensemble_products._midpoint_threshold), so nothing lies within rounding of one: the
    counts, and with them nprob, are exact, and the two sums are held to the launch's budget."""
    from neural_lam_amd.forecast import EnsembleForecast, plan_forecast
    from test_ensemble_forecast import E_LEAD, E_TIMES, _dataset
    from test_ensemble_products import _midpoint_threshold

    w, step = efm, efm.step
    S, M, starts = 2, 3, [1, 4]
    nx, ny = w.ds.nx, w.ds.ny
    assert nx * ny == w.N
    data = _dataset(w)
    events = [(0, ">", 0.0), (0, "<", 0.0), (step.state_var_names[2], ">", 0.0), (4, "<", 0.0)]
    kw = dict(members=M, n_starts=S, seed=11, record_noise=True)
    nb = dict(events=events, neighbourhoods=ENGINE_RADII, grid_shape=(nx, ny))
    ens = EnsembleForecast(step, data, E_LEAD, **nb, **kw)
    plain = EnsembleForecast(step, data, E_LEAD, **kw)
    none = EnsembleForecast(step, data, E_LEAD, events=events, neighbourhoods=None, grid_shape=(nx, ny), **kw)
    assert none.launches_per_lead == plain.launches_per_lead + 2 and not hasattr(none, "nprob") and none._nb is None
    assert ens.launches_per_lead == plain.launches_per_lead + 2 + LAUNCHES
    fields_only = EnsembleForecast(step, data, E_LEAD, members=M, n_starts=S, seed=11, verify=False, **nb)
    assert fields_only.launches_per_lead == EnsembleForecast(step, data, E_LEAD, members=M, n_starts=S, seed=11,
                                                             verify=False).launches_per_lead + 1 + LAUNCHES - 1
    with pytest.raises(ValueError, match="grid_shape"):
        EnsembleForecast(step, data, E_LEAD, events=events, neighbourhoods=[1], grid_shape=(ny + 1, nx), **kw)
    first = _snap(ens.run(starts))
    base = _snap(none.run(starts))
    assert none.run(starts).products.nprob is None and none.run(starts).products.radii == ()
    assert _same(base, {k: v for k, v in first.items() if k not in ("products.nprob", "products.fbs", "products.fbs_ref")})
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
    assert not torch.equal(first["products.prob"], second["products.prob"])     # the tables are shared: both launches moved
    assert not torch.equal(_bits(first["products.nprob"]), _bits(second["products.nprob"]))
    pr = res.products
    W = len(ENGINE_RADII)
    assert pr.radii == tuple(ENGINE_RADII) and pr.nprob.shape == (S, E_LEAD, 4, W, w.N) and pr.fbs.shape == (S, E_LEAD, 4, W) == pr.fbs_ref.shape
    # radius 0 is the point product on the live nodes
    wgt = step.interior_weight.cpu().double()
    live = (wgt != 0).to(dev)
    assert torch.equal(_bits(pr.nprob[:, :, :, 0][..., live]), _bits(pr.prob[..., live]))
    # the reference on the members
    var, sense, thr32 = [0, 0, 2, 4], [0, 1, 0, 1], ens.event_thr.cpu().double().tolist()
    x_phys = res.members.cpu().double()
    for k in range(E_LEAD):
        x = (x_phys[:, :, k] - smean) / sstd
        ref = R.ens_neighbourhood(x, std_truth[:, k], wgt, var, sense, thr32, ENGINE_RADII, nx, ny)
        got = {name: getattr(pr, name)[:, k].cpu() for name in ("nprob", "fbs", "fbs_ref")}
        _check(got, ref, wgt, ("engine", k))
    # the accessor
    fss = pr.fss()
    assert fss.shape == (E_LEAD, 4, W) and float(fss.min()) >= 0.0 and float(fss.max()) <= 1.0
    assert torch.equal(fss, 1.0 - pr.fbs.sum(0) / pr.fbs_ref.sum(0))
    # new radii: no new recording, the forecast and the point products keep their bits, the scales move
    ens.set_radii([0, 2, 3, 5, 10])
    moved = ens.run(starts)
    third = _snap(moved)
    assert ens._graph is graph and len(ens._recorded) == 0 and moved.products.radii == (0, 2, 3, 5, 10)
    assert _same(second, third, plain_keys + ["products.prob", "products.brier", "products.rel_count", "products.rel_obs"])
    for a, b in ((0, 0), (1, 2), (3, 3), (4, 4)):   # scale a of the new ladder is scale b of the old one
        assert torch.equal(_bits(third["products.nprob"][:, :, :, a]), _bits(second["products.nprob"][:, :, :, b]))
        assert torch.equal(_bits(third["products.fbs"][..., a]), _bits(second["products.fbs"][..., b]))
    assert not torch.equal(_bits(third["products.nprob"][:, :, :, 2]), _bits(second["products.nprob"][:, :, :, 2]))
    with pytest.raises(ValueError, match="set_radii"):
        ens.set_radii([0, 1])
    with pytest.raises(ValueError, match="radius"):
        ens.set_radii([0, 1, 2, 5, -1])
    ens.set_radii(ENGINE_RADII)
    assert _same(second, _snap(ens.run(starts)))
    # graph replay against the same launches issued eagerly; a shorter run is a prefix
    eager = EnsembleForecast(step, data, E_LEAD, events=list(pr.events), neighbourhoods=ENGINE_RADII, grid_shape=(nx, ny), use_graph=False, **kw)
    assert _same(second, _snap(eager.run(starts))) and eager.launches_per_lead is None
    short = _snap(ens.run(starts, leads=2))
    assert all(torch.equal(_bits(short[k]), _bits(second[k][:, :2])) for k in short if k != "noise")
    # the recording that reads given noise launches it too
    given = _snap(ens.run(starts, latent_noise=second["noise"]))
    assert _same(second, given) and len(ens._recorded) == 1 and ens._graph is not graph
    for t in (ens.nprob, ens.fbs, ens.fbs_ref):
        t.fill_(POISON)
    assert _same(second, _snap(ens.run(starts, latent_noise=second["noise"])))
    # without verification: the same fields, no scores
    fields_only.set_thresholds(thr)
    bare = fields_only.run(starts).products
    assert bare.fbs is None and bare.fbs_ref is None and bare.brier is None
    assert torch.equal(_bits(bare.nprob), _bits(second["products.nprob"]))
    with pytest.raises(ValueError, match="verify"):
        bare.fss()


@pytest.mark.gpu
def test_a_deterministic_predictor_with_one_member_gives_the_classic_fss(dev, tmp_path):
    """members = 1 on a deterministic predictor: C is the forecast's own event mask, so nprob is the classic neighbourhood
    fraction of one forecast and fss() the classic FSS.  Thresholds are midpoints, as in the engine test, so the reference
    applied to the returned member has the kernel's event masks; radius 0 gives probabilities 0 or 1, and the widest window the
    same fraction at every node."""
    from neural_lam_amd.forecast import EnsembleForecast, plan_forecast
    from test_ensemble_forecast import _dataset, _graph_lam_step
    from test_ensemble_products import _midpoint_threshold

    w = _graph_lam_step(dev, tmp_path)
    S, LEADS, nx, ny = 2, 3, w.ds.nx, w.ds.ny
    radii = [0, 1, 3, 40]
    step = w.step
    sstd, smean = step.state_std.cpu().double(), step.state_mean.cpu().double()
    events = [(1, ">", float(smean[1] + 0.1 * sstd[1])), (3, "<", float(smean[3] - 0.4 * sstd[3]))]
    data = _dataset(w)
    ens = EnsembleForecast(step, data, LEADS, members=1, n_starts=S, events=events, neighbourhoods=radii, grid_shape=(nx, ny))
    starts = [1, 5]
    off, _ = plan_forecast(w.state.shape[0], 1, 1, LEADS)
    t0 = torch.tensor(starts) + off - 1
    truth = torch.stack([w.state[t0.to(dev) + k + 1] for k in range(LEADS)], 1)
    first = ens.run(starts).state.clone()
    ens.set_thresholds([_midpoint_threshold(torch.cat([first[..., v].reshape(-1), truth[..., v].reshape(-1)]).cpu(), float(sstd[v]), target)
                        for v, target in ((1, 0.55), (3, 0.35))])
    res = ens.run(starts)
    assert torch.equal(_bits(res.state), _bits(first))
    pr = res.products
    wgt = step.interior_weight.cpu().double()
    live = wgt != 0
    p0 = pr.nprob[:, :, :, 0].cpu()
    assert bool(((p0 == 0) | (p0 == 1))[..., live].all()) and bool(torch.isnan(p0[..., ~live]).all())
    wide = pr.nprob[:, :, :, 3].cpu()
    assert bool((wide == wide[..., :1]).all()) and 0 < float(wide.mean()) < 1
    y = ((truth - step.state_mean) / step.state_std).cpu().double()
    thr32 = ens.event_thr.cpu().double()
    x = (res.members.cpu().double() - smean) / sstd   # (S, 1, leads, N, F)
    for v, t in zip((1, 3), thr32.tolist()):
        assert bool(((x[..., v] - t).abs() > 1e-4).all()) and bool(((y[..., v] - t).abs() > 1e-4).all())   # nothing near a threshold
    for k in range(LEADS):
        ref = R.ens_neighbourhood(x[:, :, k], y[:, k], wgt, [1, 3], [0, 1], thr32.tolist(), radii, nx, ny)
        got = {name: getattr(pr, name)[:, k].cpu() for name in ("nprob", "fbs", "fbs_ref")}
        _check(got, ref, wgt, ("deterministic", k))
    fss = pr.fss()
    assert fss.shape == (LEADS, 2, 4) and float(fss.min()) >= 0.0 and float(fss.max()) <= 1.0
    want = R.fss(pr.fbs.cpu().double(), pr.fbs_ref.cpu().double())
    assert torch.allclose(fss.cpu().double(), want, rtol=1e-5, atol=1e-6)
