"""The forecast engine (neural_lam_amd/forecast.py; nlam_forecast_init / _head / _tail / _finish): the C-ABI and the host
planning without a GPU, the float64 restatement (tests/forecast_ref.py) pinned against the oracle's ARForecaster on the CPU, and on
the GPU the kernels against the data path, against nlam_step_tail_ext_fwd and against the restatement, the guard on the lead
counter, and the engine against the existing rollout, against itself (graph / eager, horizons, restarts, changed weights, bf16) and
under a trainer's averaged weights."""
import ctypes as C
import subprocess
import types

import numpy as np
import pytest
import torch

import forecast_ref as R
from conftest import ROOT, rel_err
from neural_lam_amd import _lib as L

EPS32 = float(torch.finfo(torch.float32).eps)
NEW_EXPORTS = ["nlam_forecast_init", "nlam_forecast_head", "nlam_forecast_tail", "nlam_forecast_finish",
               "nlam_forecast_workspace_floats"]
WINDOWS = [(1, 1), (3, 0), (0, 2)]
BF16_NOISE_FACTOR = 1.5   # the autocast bar of tests/test_full_size_parity.py: at most this much noisier than the existing route
BF16_NOISE_FLOOR = 1e-3   # under autocast (both against the fp32 route), plus this allowance


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_forecast_symbols_are_exported_and_the_struct_matches_c_layout(tmp_path):
    assert set(NEW_EXPORTS) <= set(L.EXPORTS)
    lib = L.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert lib.nlam_abi_version() == 8
    fields = [name for name, _ in L.Forecast._fields_]
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
        'int main(){printf("%zu", sizeof(nlam_forecast_t));\n'
        + "".join(f'printf(" %zu", offsetof(nlam_forecast_t, {f}));\n' for f in fields)
        + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.Forecast)] + [getattr(L.Forecast, f).offset for f in fields]


def test_forecast_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    B, N, F, DF, LEAD = 3, 37, 5, 2, 4
    nws = lib.nlam_forecast_workspace_floats(B, N, F)
    assert nws >= B * 2 * F
    for bad in ((0, N, F), (B, 0, F), (B, N, 0)):
        assert lib.nlam_forecast_workspace_floats(*bad) == -1, bad
    assert lib.nlam_forecast_workspace_floats(B, N, L.EVAL_MAX_VARS + 1) == -2
    modes = (C.c_int32 * F)(0, 1, 2, 3, 0)
    bad_modes = (C.c_int32 * F)(0, 1, 2, 4, 0)

    def args(std_head=False, verify=True, **kw):
        p = L.Forecast()
        for name in ("state", "forcing", "times", "start", "lead", "state_mean", "state_std", "forcing_mean", "forcing_std", "prev",
                     "prev_prev", "forcing_windowed", "truth", "delta", "dstd", "dmean", "bmask", "row_weight", "clamp_lo", "clamp_hi",
                     "out_state", "valid_times"):
            setattr(p, name, fake)
        p.clamp_mode_host = C.addressof(modes)
        if verify:
            p.sq = p.ab = p.workspace = fake
            p.workspace_floats = nws
        p.n_times, p.nodes, p.d_state, p.d_forcing, p.batch = 16, N, F, DF, B
        p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps, p.delta_ld = LEAD, 1, 1, F
        if std_head:
            p.delta_ld, p.out_std = 2 * F, fake
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    entries = {"init": lib.nlam_forecast_init, "head": lib.nlam_forecast_head, "tail": lib.nlam_forecast_tail,
               "finish": lib.nlam_forecast_finish}
    for fn in entries.values():
        assert fn(None, None) == -1
    sizes = [dict(n_times=0), dict(nodes=0), dict(d_state=0), dict(d_forcing=-1), dict(batch=0), dict(max_lead=0),
             dict(num_past_forcing_steps=-1), dict(num_future_forcing_steps=-1), dict(lead=None)]
    series = [dict(state=None), dict(start=None), dict(state_mean=None), dict(state_std=None), dict(forcing=None),
              dict(forcing_mean=None), dict(forcing_std=None)]
    bad = {"init": sizes + series + [dict(prev=None), dict(prev_prev=None)],
           "head": sizes + series + [dict(truth=None), dict(forcing_windowed=None)],
           "tail": sizes + series + [dict(delta=None), dict(prev=None), dict(prev_prev=None), dict(truth=None), dict(bmask=None),
                                     dict(out_state=None), dict(delta_ld=F + 1), dict(delta_ld=3 * F), dict(delta_ld=2 * F),
                                     dict(out_std=fake), dict(clamp_lo=None), dict(clamp_hi=None),
                                     dict(clamp_mode_host=C.addressof(bad_modes)), dict(row_weight=None), dict(workspace=None),
                                     dict(workspace_floats=nws - 1), dict(ab=None, workspace=None)],
           "finish": sizes + [dict(workspace=None), dict(workspace_floats=nws - 1)]}
    for name, cases in bad.items():
        for kw in cases:
            assert entries[name](args(**kw), None) == -1, (name, kw)
    assert lib.nlam_forecast_tail(args(std_head=True, out_std=None), None) == -1   # a std head needs its output
    for name, fn in entries.items():
        assert fn(args(verify=False, d_state=L.LOSS_MAX_VARS + 1, delta_ld=L.LOSS_MAX_VARS + 1), None) == -2, name
    for name in ("tail", "finish"):   # the verification sums keep the variable limit of nlam_eval_metrics
        assert entries[name](args(d_state=L.EVAL_MAX_VARS + 1, delta_ld=L.EVAL_MAX_VARS + 1, clamp_mode_host=None), None) == -2, name


def test_plan_forecast_against_hand_computed_cases_and_window_len():
    from neural_lam_amd.forecast import check_starts, plan_forecast

    lib = L.load()
    n, lead = 16, 4
    hand = {(1, 1): (2, 10), (3, 0): (3, 10), (0, 2): (2, 9)}   # off = max(2, past); starts = n - (off + lead + future) + 1
    for (past, fut), want in hand.items():
        off, count = plan_forecast(n, past, fut, lead)
        assert (off, count) == want == R.plan(n, past, fut, lead)
        assert count == lib.nlam_window_len(n, n, lead, past, fut)
        for i in (0, count - 1):   # the first and the last valid start read inside the series, unclamped
            t0 = i + off - 1
            assert t0 - 1 >= 0
            for k in range(lead):
                window = [t0 + k + 1 - past + w for w in range(past + fut + 1)]
                assert 0 <= min(window) and max(window) <= n - 1 and t0 + k + 1 <= n - 1
                assert R.lead_times(t0, k, past, fut, n) == (t0 + k + 1, window)
        assert check_starts([0, -1, count - 1], count).tolist() == [0, count - 1, count - 1]
        for i in (count, -count - 1):
            with pytest.raises(IndexError):
                check_starts([0, i], count)
    assert plan_forecast(5, 1, 1, 4) == (2, 0)   # too short a series: no valid start
    with pytest.raises(ValueError):
        plan_forecast(16, 1, 1, 0)


def _graph_of(ds, hier=False):
    from neural_lam_amd import graph as G

    ext = ds.get_xy_extent("state")
    raw = G.create_regular_grid_graph(ds.get_xy("state"), n_max_levels=3 if hier else None, hierarchical=hier)
    return G.normalise_graph(raw, max(ext[1] - ext[0], ext[3] - ext[2]))


def _clamp_kw(ds):
    names = ds.get_vars_names("state")   # one variable per mode: lower, both, upper (physical limits around the series)
    return dict(output_clamping_lower={names[0]: -3.0, names[2]: -4.0}, output_clamping_upper={names[2]: 4.0, names[4]: 3.0})


@pytest.mark.parametrize("options", ["plain", "clamps_std"])
def test_restatement_equals_the_oracle_rollout_on_the_cpu(tmp_path, options):
    """head -> oracle network -> float64 tail, four leads, against oracle.models.ARForecaster fed by oracle.data: 1e-6 of the max.
    The raw network output is read off the oracle predictor's output_map (its forward returns the finished state)."""
    from neural_lam_amd.datastore import SyntheticDatastore
    from oracle import data as od
    from oracle import models as om

    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)
    kw = dict(_clamp_kw(ds), output_std=True) if options == "clamps_std" else {}
    torch.manual_seed(3)
    predictor = om.GraphLAM(ds, _graph_of(ds), hidden_dim=8, processor_layers=1, **kw)
    forecaster = om.ARForecaster(predictor, ds)
    N, leads, past, fut, idx = ds.num_grid_points, 4, 1, 1, 2
    rng = np.random.default_rng(5)
    state = rng.standard_normal((12, N, 5)).astype(np.float32)
    forcing = rng.standard_normal((12, N, 2)).astype(np.float32)
    eps = torch.finfo(torch.float32).eps
    st, fs = ds.get_standardization_dataarray("state"), ds.get_standardization_dataarray("forcing")
    stats = {"state_mean": torch.tensor(st.state_mean.values, dtype=torch.float32),
             "state_std": torch.clamp(torch.tensor(st.state_std.values, dtype=torch.float32), min=eps),
             "forcing_mean": torch.tensor(fs.forcing_mean.values, dtype=torch.float32),
             "forcing_std": torch.clamp(torch.tensor(fs.forcing_std.values, dtype=torch.float32), min=eps)}
    item = od.build_item(state, forcing, None, idx, leads, past, fut)
    init, target, forc = od.standardize_item(*item[:3], *(stats[k].numpy() for k in ("state_mean", "state_std", "forcing_mean",
                                                                                      "forcing_std")), past + fut + 1)
    with torch.no_grad():
        want, want_std = forecaster(*(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None] for a in (init, forc, target)))
    captured = {}
    hook = predictor.output_map.register_forward_hook(lambda m, i, o: captured.__setitem__("delta", o))

    def net(prev, pprev, fw):
        with torch.no_grad():
            predictor(prev, pprev, fw)
        return captured["delta"]

    modes, lo, hi = R.clamp_tables(predictor)
    assert sorted(modes) == ([0, 0, 1, 2, 3] if options == "clamps_std" else [0] * 5)
    off, _ = R.plan(12, past, fut, leads)
    got = R.rollout(net, torch.from_numpy(state), torch.from_numpy(forcing), [idx + off - 1], leads, past, fut, stats,
                    predictor.diff_std, predictor.diff_mean, forecaster.boundary_mask.reshape(-1), modes, lo, hi)
    hook.remove()
    assert rel_err(got["new"], want.to(torch.float64)) <= 1e-6
    mean, std = stats["state_mean"].to(torch.float64), stats["state_std"].to(torch.float64)
    assert rel_err(got["out_state"], want.to(torch.float64) * std + mean) <= 1e-6
    if options == "clamps_std":
        assert rel_err(got["out_std"], want_std.to(torch.float64) * std) <= 1e-6


def test_forecast_refuses_what_it_does_not_serve(tmp_path, monkeypatch):
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore
    from neural_lam_amd.forecast import Forecast

    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)
    graph = _graph_of(ds)
    step = hm.ForecasterStep(hm.ARForecaster(hm.GraphLAM(ds, graph=graph, hidden_dim=8, processor_layers=1), ds), ds)
    plain = types.SimpleNamespace(kernel="nlam_window_batch", device=torch.device("cpu"))
    with pytest.raises(ValueError, match="ensemble"):
        Forecast(step, types.SimpleNamespace(kernel="nlam_window_batch_ens"), 4)
    with pytest.raises(ValueError, match="max_lead"):
        Forecast(step, plain, 0)
    with pytest.raises(RuntimeError, match="GPU"):   # CPU tensors raise, as everywhere else in the product
        Forecast(step, plain, 4)
    clamped = hm.ForecasterStep(hm.ARForecaster(hm.GraphLAM(ds, graph=graph, hidden_dim=8, processor_layers=1, **_clamp_kw(ds)), ds), ds)
    monkeypatch.setattr(hm, "FUSED_CLAMPED_TAIL", False)
    with pytest.raises(ValueError, match="raw network output"):
        Forecast(clamped, plain, 4)
    monkeypatch.undo()
    step.forecaster.predictor.diff_std = step.forecaster.predictor.diff_std.reshape(1, -1)   # a per-node diff_std has two dims
    with pytest.raises(ValueError, match="raw network output"):
        Forecast(step, plain, 4)
    with pytest.raises(ValueError, match="ARForecaster"):
        Forecast(torch.nn.Linear(2, 2), plain, 4)


# ---------------------------------------------------------------------------
# GPU: the kernels
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _misaligned(t):
    """The same values at a 4-byte offset: a contiguous view whose data pointer is not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


N_TIMES, NODES, NVARS, BATCH, LEAD = 16, 37, 5, 3, 4


def _series(dev, d_forcing, nodes=NODES, seed=0, nvars=NVARS):
    g = torch.Generator().manual_seed(seed)
    state = (torch.randn(N_TIMES, nodes, nvars, generator=g) * 2.0 + 0.5).to(dev)
    forcing = (torch.randn(N_TIMES, nodes, d_forcing, generator=g) * 3.0 - 1.0).to(dev) if d_forcing else None
    stats = {"state_mean": torch.randn(nvars, generator=g).to(dev), "state_std": (torch.rand(nvars, generator=g) + 0.5).to(dev)}
    if d_forcing:
        stats.update(forcing_mean=torch.randn(d_forcing, generator=g).to(dev), forcing_std=(torch.rand(d_forcing, generator=g) + 0.5).to(dev))
    times = (torch.arange(N_TIMES, dtype=torch.int64) * 3_600_000_000_000 + 1_700_000_000_000_000_000).to(dev)
    return state, forcing, times, stats


def _series_args(state, forcing, times, stats, start, lead, past, fut, max_lead=LEAD):
    p = L.Forecast()
    p.state, p.forcing, p.times, p.start, p.lead = _ptr(state), _ptr(forcing), _ptr(times), _ptr(start), _ptr(lead)
    p.state_mean, p.state_std = _ptr(stats["state_mean"]), _ptr(stats["state_std"])
    p.forcing_mean, p.forcing_std = _ptr(stats.get("forcing_mean")), _ptr(stats.get("forcing_std"))
    p.n_times, p.nodes, p.d_state, p.batch = state.shape[0], state.shape[1], state.shape[2], start.numel()
    p.d_forcing = 0 if forcing is None else forcing.shape[2]
    p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps = max_lead, past, fut
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("d_forcing", [2, 0])
@pytest.mark.parametrize("past,fut", WINDOWS)
def test_head_and_init_give_the_bits_of_the_data_path(dev, past, fut, d_forcing, misalign):
    """Every lead's forcing window and boundary truth, and the two initial states, against DeviceWeatherDataset.batch at
    ar_steps = max_lead (nlam_window_batch with statistics): bit-equal.  nodes = 37: the second and third forecast's rows start off
    a 16-byte boundary; misalign: every buffer does."""
    from neural_lam_amd.data import DeviceWeatherDataset
    from neural_lam_amd.forecast import plan_forecast

    lib = L.load()
    put = _misaligned if misalign else (lambda t: t)
    state, forcing, times, stats = _series(dev, d_forcing)
    state, forcing = put(state), (put(forcing) if forcing is not None else None)
    data = DeviceWeatherDataset(state, forcing, times, ar_steps=LEAD, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                                standardization=stats)
    off, count = plan_forecast(N_TIMES, past, fut, LEAD)
    assert count == len(data)
    starts = torch.tensor([0, count // 2, count - 1], dtype=torch.int64)
    init, target, forc, target_times = data.batch(starts, standardize=True)
    start = (starts + off - 1).to(dev)
    lead = torch.full((1,), 7, dtype=torch.int32, device=dev)
    window = past + fut + 1
    nan = lambda *shape: put(torch.full(shape, float("nan"), device=dev))   # noqa: E731
    prev, pprev, truth, fw = nan(BATCH, NODES, NVARS), nan(BATCH, NODES, NVARS), nan(BATCH, NODES, NVARS), nan(BATCH, NODES, d_forcing * window)
    p = _series_args(state, forcing, times, stats, start, lead, past, fut)
    p.prev, p.prev_prev, p.truth, p.forcing_windowed = _ptr(prev), _ptr(pprev), _ptr(truth), (_ptr(fw) if d_forcing else None)
    L.check(lib.nlam_forecast_init(C.byref(p), _stream()), "nlam_forecast_init")
    assert int(lead) == 0
    assert torch.equal(_bits(pprev), _bits(init[:, 0])) and torch.equal(_bits(prev), _bits(init[:, 1]))
    for k in range(LEAD):
        lead.fill_(k)
        truth.fill_(float("nan"))
        fw.fill_(float("nan"))
        L.check(lib.nlam_forecast_head(C.byref(p), _stream()), "nlam_forecast_head")
        assert torch.equal(_bits(truth), _bits(target[:, k])), k
        if d_forcing:
            assert torch.equal(_bits(fw), _bits(forc[:, k])), k
        assert int(lead) == k   # the head only reads the counter
    # the restatement's indexing gives the same values (float64 division against IEEE fp32: a rounding apart)
    fw64, truth64 = R.head(state.cpu(), None if forcing is None else forcing.cpu(), start.tolist(), LEAD - 1, past, fut,
                           *(stats[k].cpu() for k in ("state_mean", "state_std")),
                           *((stats[k].cpu() for k in ("forcing_mean", "forcing_std")) if d_forcing else ()))
    assert rel_err(truth.cpu().to(torch.float64), truth64) <= 2 * EPS32
    if d_forcing:
        assert rel_err(fw.cpu().to(torch.float64), fw64) <= 2 * EPS32


def _tail_case(dev, nodes, clamp, std_head, misalign, with_times, seed=1, nvars=NVARS, batch=BATCH):
    """Inputs of one tail launch at lead K of LEAD, every output NaN / -1 filled; `nvars` variables, `batch` forecasts."""
    from neural_lam_amd.ops import ClampTables

    put = _misaligned if misalign else (lambda t: t)
    g = torch.Generator().manual_seed(seed)
    state, _, times, stats = _series(dev, 0, nodes=nodes, nvars=nvars)
    ld = 2 * nvars if std_head else nvars
    c = types.SimpleNamespace(nodes=nodes, ld=ld, stats=stats, state=state, times=times if with_times else None, nvars=nvars, batch=batch)
    c.delta = put(torch.randn(batch * nodes, ld, generator=g).to(dev))
    c.prev0 = (torch.randn(batch, nodes, nvars, generator=g) * 0.7).to(dev)
    c.pprev0 = torch.randn(batch, nodes, nvars, generator=g).to(dev)
    c.truth = put((torch.randn(batch, nodes, nvars, generator=g) * 0.7).to(dev))
    c.dstd = (torch.rand(nvars, generator=g) * 0.5 + 0.1).to(dev)
    c.dmean = (torch.randn(nvars, generator=g) * 0.1).to(dev)
    c.bmask = (torch.rand(nodes, generator=g) < 0.3).to(torch.float32).to(dev)
    interior = 1.0 - c.bmask
    c.row_weight = interior / interior.sum()
    c.clamp = None
    if clamp:   # NONE, BOTH, LOWER and UPPER on different variables: the five-variable table, repeated over the variables
        cyc = lambda v: (v * (nvars // 5 + 1))[:nvars]   # noqa: E731
        lo = torch.tensor(cyc([0.0, -1.5, -1.2, 0.0, 0.0])).to(dev)
        hi = torch.tensor(cyc([0.0, 1.5, 0.0, 1.3, 0.0])).to(dev)
        c.clamp = ClampTables(cyc([L.CLAMP_NONE, L.CLAMP_BOTH, L.CLAMP_LOWER, L.CLAMP_UPPER, L.CLAMP_NONE]), lo, hi)
    c.start = torch.tensor([1, 6, 9, 4, 7, 2][:batch], dtype=torch.int64, device=dev)
    c.lead = torch.zeros(1, dtype=torch.int32, device=dev)
    return c, put


def _tail_buffers(c, put, slots, verify):
    dev = c.delta.device
    B, F = c.batch, c.nvars
    nan = lambda *shape: put(torch.full(shape, float("nan"), device=dev))   # noqa: E731
    b = types.SimpleNamespace()
    b.prev, b.pprev = put(c.prev0.clone()), put(c.pprev0.clone())
    b.out_state = nan(B, slots, c.nodes, F)
    b.out_std = nan(B, slots, c.nodes, F) if c.ld == 2 * F else None
    b.valid_times = torch.full((B, slots), -1, dtype=torch.int64, device=dev)
    b.sq = nan(B, slots, F) if verify else None
    b.ab = nan(B, slots, F) if verify else None
    b.workspace = torch.full((int(L.load().nlam_forecast_workspace_floats(B, c.nodes, F)),), float("nan"), device=dev) if verify else None
    return b


def _tail_args(c, b, max_lead):
    p = _series_args(c.state, None, c.times, c.stats, c.start, c.lead, 1, 1, max_lead=max_lead)
    p.prev, p.prev_prev, p.truth, p.delta = _ptr(b.prev), _ptr(b.pprev), _ptr(c.truth), _ptr(c.delta)
    p.dstd, p.dmean, p.bmask, p.row_weight = _ptr(c.dstd), _ptr(c.dmean), _ptr(c.bmask), _ptr(c.row_weight)
    if c.clamp is not None:
        p.clamp_mode_host, p.clamp_lo, p.clamp_hi = C.addressof(c.clamp.mode), _ptr(c.clamp.lo), _ptr(c.clamp.hi)
    p.out_state, p.out_std, p.valid_times = _ptr(b.out_state), _ptr(b.out_std), _ptr(b.valid_times)
    p.sq, p.ab, p.workspace = _ptr(b.sq), _ptr(b.ab), _ptr(b.workspace)
    p.workspace_floats = 0 if b.workspace is None else b.workspace.numel()
    p.delta_ld = c.ld
    return p


def _run_tail(c, b, max_lead, k):
    lib = L.load()
    p = _tail_args(c, b, max_lead)
    c.lead.fill_(k)
    L.check(lib.nlam_forecast_tail(C.byref(p), _stream()), "nlam_forecast_tail")
    L.check(lib.nlam_forecast_finish(C.byref(p), _stream()), "nlam_forecast_finish")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("nodes", [NODES, 1721])   # one chunk of nodes per forecast; three chunks (820 nodes each at F = 5)
@pytest.mark.parametrize("clamp,std_head", [(False, False), (True, False), (False, True), (True, True)])
def test_tail_against_the_step_tail_and_the_restatement(dev, clamp, std_head, nodes, misalign):
    from neural_lam_amd.ops import StepTailExtFunction

    K = 2
    c, put = _tail_case(dev, nodes, clamp, std_head, misalign, with_times=not misalign)
    pred, pred_std, _ = StepTailExtFunction.apply(c.delta.view(BATCH, nodes, c.ld), c.prev0, c.truth, None, c.dstd, c.dmean, c.bmask,
                                                  None, None, 1.0, None, c.clamp)
    b = _tail_buffers(c, put, LEAD, verify=True)
    _run_tail(c, b, LEAD, K)
    # the state: the bits of nlam_step_tail_ext_fwd(target = NULL), rotated in place
    assert torch.equal(_bits(b.prev), _bits(pred))
    assert torch.equal(_bits(b.pprev), _bits(c.prev0))
    assert int(c.lead) == K + 1
    # slot K in physical units: a multiply and an add, or one FMA; every other slot keeps its sentinel
    mean, std = c.stats["state_mean"].double(), c.stats["state_std"].double()
    want = pred.double() * std + mean
    bound = 2 * EPS32 * ((pred.double() * std).abs() + mean.abs())
    assert bool(((b.out_state[:, K].double() - want).abs() <= bound).all())
    others = [k for k in range(LEAD) if k != K]
    assert bool(torch.isnan(b.out_state[:, others]).all())
    if std_head:
        want_std = pred_std.double() * std
        assert bool(((b.out_std[:, K].double() - want_std).abs() <= EPS32 * want_std.abs()).all())   # one multiply
        assert bool(torch.isnan(b.out_std[:, others]).all())
    t_valid = c.start + K + 1
    assert torch.equal(b.valid_times[:, K], c.times[t_valid] if c.times is not None else t_valid)
    assert bool((b.valid_times[:, others] == -1).all())
    # against the float64 formulas: the state, and the verification sums over the interior weights
    modes = list(c.clamp.modes) if clamp else [R.CLAMP_NONE] * NVARS
    lo, hi = (c.clamp.lo.cpu(), c.clamp.hi.cpu()) if clamp else (torch.zeros(NVARS), torch.zeros(NVARS))
    ref = R.tail(c.delta.cpu().view(BATCH, nodes, c.ld), c.prev0.cpu(), c.truth.cpu(), c.dstd.cpu(), c.dmean.cpu(), c.bmask.cpu(),
                 modes, lo, hi, c.stats["state_mean"].cpu(), c.stats["state_std"].cpu())
    assert rel_err(b.prev.cpu().double(), ref["new"]) <= 1e-5
    if std_head:
        assert rel_err(b.out_std[:, K].cpu().double(), ref["out_std"]) <= 1e-5
    sq64, ab64 = R.masked_sums(b.prev.cpu(), c.truth.cpu(), c.row_weight.cpu())   # the sums of the values the kernel held
    tol = (nodes + 8) * EPS32
    for got, want64 in ((b.sq, sq64), (b.ab, ab64)):
        assert bool(((got[:, K].cpu().double() - want64).abs() <= tol * want64.abs()).all())
        assert bool(torch.isnan(got[:, others]).all())
    # a second run from the same inputs: the same bits
    b2 = _tail_buffers(c, put, LEAD, verify=True)
    _run_tail(c, b2, LEAD, K)
    assert torch.equal(_bits(b.sq[:, K]), _bits(b2.sq[:, K])) and torch.equal(_bits(b.ab[:, K]), _bits(b2.ab[:, K]))
    assert torch.equal(_bits(b.out_state[:, K]), _bits(b2.out_state[:, K]))
    # without the sums nothing else changes
    b3 = _tail_buffers(c, put, LEAD, verify=False)
    _run_tail(c, b3, LEAD, K)
    assert torch.equal(_bits(b3.prev), _bits(b.prev)) and torch.equal(_bits(b3.out_state), _bits(b.out_state))
    assert int(c.lead) == K + 1


@pytest.mark.gpu
@pytest.mark.parametrize("std_head", [False, True])
def test_a_replay_too_many_writes_nothing(dev, std_head):
    """max_lead + 1 slots allocated, max_lead passed, the counter at max_lead: head, tail and finish leave every buffer as it was (a
    broken guard would land in the spare slot, never out of bounds)."""
    lib = L.load()
    c, put = _tail_case(dev, NODES, True, std_head, False, with_times=True)
    b = _tail_buffers(c, put, LEAD + 1, verify=True)
    truth_head = torch.full((BATCH, NODES, NVARS), float("nan"), device=dev)
    before = {k: v.clone() for k, v in vars(b).items() if v is not None}
    p = _tail_args(c, b, LEAD)
    c.lead.fill_(LEAD)
    p.truth = _ptr(truth_head)
    L.check(lib.nlam_forecast_head(C.byref(p), _stream()), "nlam_forecast_head")
    p.truth = _ptr(c.truth)
    L.check(lib.nlam_forecast_tail(C.byref(p), _stream()), "nlam_forecast_tail")
    L.check(lib.nlam_forecast_finish(C.byref(p), _stream()), "nlam_forecast_finish")
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(_bits(getattr(b, k)), _bits(v)), k
    assert bool(torch.isnan(truth_head).all())
    assert int(c.lead) == LEAD


# ---------------------------------------------------------------------------
# GPU: the engine
# ---------------------------------------------------------------------------
E_TIMES, E_LEAD, E_BATCH = 20, 6, 2
E_STARTS = [1, 5]


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """One 30 x 27 SyntheticDatastore (boundary="random"), its flat and hierarchical graphs and a 20-step analysis series."""
    from neural_lam_amd.datastore import SyntheticDatastore

    root = tmp_path_factory.mktemp("forecast")
    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=root, boundary="random", seed=1)
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(11)
    w = types.SimpleNamespace(ds=ds, N=N, graphs={})
    w.state = torch.randn(E_TIMES, N, 5, generator=g).to(dev)
    w.forcing = torch.randn(E_TIMES, N, 2, generator=g).to(dev)
    w.times = (torch.arange(E_TIMES, dtype=torch.int64) * 10 + 1000).to(dev)
    return w


def _make_step(world, dev, model="graph_lam", seed=1, **kw):
    from neural_lam_amd import models as hm

    hier = model != "graph_lam"
    if hier not in world.graphs:
        world.graphs[hier] = _graph_of(world.ds, hier)
    torch.manual_seed(seed)
    predictor = hm.MODELS[model](world.ds, graph=world.graphs[hier], hidden_dim=16, processor_layers=2, **kw)
    return hm.ForecasterStep(hm.ARForecaster(predictor, world.ds), world.ds).to(dev)


def _dataset(world, step, ar_steps=E_LEAD):
    from neural_lam_amd.data import DeviceWeatherDataset

    return DeviceWeatherDataset(world.state, world.forcing, world.times, ar_steps=ar_steps, standardization=step.standardization_stats())


def _snapshot(res):
    return {k: (None if v is None else v.clone()) for k, v in res._asdict().items()}


def _same(a, b, leads=None):
    for k in a:
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and not torch.equal(_bits(a[k][:, :leads]), _bits(b[k][:, :leads])):
            return False
    return True


MODELS = {"graph_lam": ("graph_lam", {}), "graph_lam_clamps_std": ("graph_lam", "clamps_std"), "hi_lam": ("hi_lam", {})}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_matches_the_existing_rollout_and_evaluate(dev, world, name):
    from neural_lam_amd.forecast import Forecast

    model, kw = MODELS[name]
    if kw == "clamps_std":
        kw = dict(_clamp_kw(world.ds), output_std=True)
    step = _make_step(world, dev, model, **kw)
    data = _dataset(world, step)
    fc = Forecast(step, data, E_LEAD, batch_size=E_BATCH, verify=True)
    res = fc.run(E_STARTS)
    init, target, forcing, target_times = data.batch(E_STARTS, standardize=True)
    with torch.no_grad():
        want, want_std = step.forecaster(init, forcing, target)
    ev = step.evaluate(init, target, forcing, phase="test", standardize=False)
    torch.cuda.synchronize()
    got = (res.state - step.state_mean) / step.state_std   # the engine's standardised trajectory
    assert rel_err(got, want) <= 1e-4
    assert torch.equal(res.valid_times, target_times)
    if kw:
        # both routes run the same tail function on the same inputs: the standardised state is bit-identical
        assert torch.equal(_bits(fc.prev), _bits(want[:, -1])) and torch.equal(_bits(fc.prev_prev), _bits(want[:, -2]))
        assert rel_err(res.std / step.state_std, want_std) <= 1e-4
    else:
        assert res.std is None
    tol = (world.N + 8) * EPS32
    assert bool(((res.sq - ev.entry_mse).abs() <= tol * ev.entry_mse.abs()).all())
    assert bool(((res.ab - ev.entry_mae).abs() <= tol * ev.entry_mae.abs()).all())
    assert torch.equal(res.rmse(step.state_std), torch.sqrt(res.sq.mean(dim=0)) * step.state_std)
    # and against the float64 restatement of the sums on the engine's own trajectory
    bt = got.reshape(E_BATCH * E_LEAD, world.N, 5).cpu()
    sq64, _ = R.masked_sums(bt, target.reshape(E_BATCH * E_LEAD, world.N, 5).cpu(), step.interior_weight.cpu())
    assert rel_err(res.sq.reshape(-1, 5).cpu().double(), sq64) <= 1e-4


@pytest.mark.gpu
def test_engine_behaviour(dev, world):
    """Graph and eager give the same bits; a second run resets the counter and the state; a longer horizon starts with the shorter
    one's leads; the recorded step does not grow with the horizon; weights changed in place are honoured."""
    from neural_lam_amd.forecast import Forecast

    step = _make_step(world, dev)
    data = _dataset(world, step)
    mk = lambda lead=E_LEAD, **kw: Forecast(step, data, lead, batch_size=E_BATCH, verify=True, **kw)   # noqa: E731
    fc = mk()
    first = _snapshot(fc.run(E_STARTS))
    assert _same(first, _snapshot(mk(use_graph=False).run(E_STARTS)))
    other = _snapshot(fc.run([7, 0]))
    assert not _same(first, other)
    assert _same(other, _snapshot(mk().run(torch.tensor([7, 0], device=dev))))   # a device index tensor is used as it is
    assert _same(first, _snapshot(fc.run(E_STARTS)))
    long = mk(12)
    assert _same(first, _snapshot(long.run(E_STARTS)), leads=E_LEAD)
    short = _snapshot(long.run(E_STARTS, leads=3))
    assert _same(first, short, leads=3)
    assert fc.launches_per_lead == long.launches_per_lead and fc.launches_per_lead > 4
    assert mk(use_graph=False).launches_per_lead is None
    with pytest.raises(IndexError):
        fc.run([0, fc.n_starts])
    with pytest.raises(ValueError):
        fc.run([0])
    with pytest.raises(ValueError):
        fc.run(E_STARTS, leads=E_LEAD + 1)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for p in step.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(dev))
    changed = _snapshot(fc.run(E_STARTS))
    assert not _same(first, changed)
    assert _same(changed, _snapshot(mk().run(E_STARTS)))


@pytest.mark.gpu
def test_engine_under_bf16_autocast_stays_within_the_autocast_bar(dev, world):
    from neural_lam_amd.forecast import Forecast

    step = _make_step(world, dev)
    data = _dataset(world, step)
    init, target, forcing, _ = data.batch(E_STARTS, standardize=True)
    with torch.no_grad():
        fp32, _ = step.forecaster(init, forcing, target)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            existing, _ = step.forecaster(init, forcing, target)
    res = Forecast(step, data, E_LEAD, batch_size=E_BATCH, autocast_dtype=torch.bfloat16).run(E_STARTS)
    got = (res.state - step.state_mean) / step.state_std
    e_engine, e_existing = rel_err(got, fp32), rel_err(existing.float(), fp32)
    print(f"bf16 autocast: engine {e_engine:.3e}, existing route {e_existing:.3e}")
    assert e_engine <= BF16_NOISE_FACTOR * e_existing + BF16_NOISE_FLOOR


@pytest.mark.gpu
def test_engine_inside_ema_weights_equals_a_module_loaded_from_the_average(dev, world):
    from neural_lam_amd.forecast import Forecast
    from neural_lam_amd.trainer import Trainer

    step = _make_step(world, dev)
    data = _dataset(world, step, ar_steps=2)
    tr = Trainer(step, lr=1e-2, use_graph=False, ema_decay=0.5)
    for i in (0, 3):
        init, target, forcing, _ = data.batch([i, i + 1], standardize=True)
        tr.step(init, target, forcing)
    fc = Forecast(step, data, E_LEAD, batch_size=E_BATCH, verify=True)
    raw = _snapshot(fc.run(E_STARTS))
    ema_sd = tr.ema_state_dict()
    with tr.ema_weights():
        inside = _snapshot(fc.run(E_STARTS))
    assert not _same(raw, inside)
    assert _same(raw, _snapshot(fc.run(E_STARTS)))   # the weights came back
    fresh = _make_step(world, dev, seed=9)
    fresh.load_state_dict(ema_sd)
    assert _same(inside, _snapshot(Forecast(fresh, data, E_LEAD, batch_size=E_BATCH, verify=True).run(E_STARTS)))
