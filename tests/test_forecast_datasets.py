"""The forecast engines on forecast-type and ensemble datasets (nlam_forecast_init_strided / _head_strided; Forecast and
EnsembleForecast over a DeviceWeatherDataset of any layout): the C-ABI and the planner without a GPU; on the GPU the two kernels
against DeviceWeatherDataset.batch at ar_steps = max_lead, bit for bit, and the engines against the plain-series engines on the
matching series, bit for bit, and against the existing rollout."""
import ctypes as C
import subprocess
import types

import pytest
import torch

from conftest import ROOT, rel_err
from neural_lam_amd import _lib as L
from test_forecast import WINDOWS, _clamp_kw, _graph_of

EPS32 = float(torch.finfo(torch.float32).eps)
NEW_EXPORTS = ["nlam_forecast_init_strided", "nlam_forecast_head_strided"]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_strided_symbols_are_exported_and_the_struct_matches_c_layout(tmp_path):
    header = (ROOT / "include" / "nlam_hip.h").read_text()
    lib = L.load()
    for name in NEW_EXPORTS:
        assert f"int32_t {name}(" in header and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_abi_version() == 8
    fields = [name for name, _ in L.ForecastSrc._fields_]
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
        'int main(){printf("%zu", sizeof(nlam_forecast_src_t));\n'
        + "".join(f'printf(" %zu", offsetof(nlam_forecast_src_t, {f}));\n' for f in fields)
        + 'printf("\\n"); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.ForecastSrc)] + [getattr(L.ForecastSrc, f).offset for f in fields]


def test_strided_entry_points_reject_bad_arguments_without_a_gpu():
    lib = L.load()
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    B, N, F, DF, LEAD, PAST, FUT = 3, 37, 5, 2, 4, 3, 1
    off = max(2, PAST)

    def args(**kw):
        p = L.Forecast()
        for name in ("lead", "state_mean", "state_std", "forcing_mean", "forcing_std", "prev", "prev_prev", "forcing_windowed", "truth"):
            setattr(p, name, fake)
        p.nodes, p.d_state, p.d_forcing, p.batch = N, F, DF, B
        p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps, p.delta_ld = LEAD, PAST, FUT, F
        s = L.ForecastSrc()
        s.state = s.forcing = s.sample_idx = fake
        s.state_stride_sample, s.state_stride_step, s.state_stride_member = 7 * 3 * N * F, 3 * N * F, N * F
        s.forcing_stride_sample, s.forcing_stride_step, s.forcing_stride_member = 8 * N * DF, N * DF, 0
        s.n_times, s.state_steps, s.forcing_steps, s.is_forecast, s.members = 4, off + LEAD, off + LEAD + FUT, 1, 3
        for k, v in kw.items():   # src_*: a field of the source, anything else one of nlam_forecast_t
            setattr(s, k[4:], v) if k.startswith("src_") else setattr(p, k, v)
        return C.byref(p), C.byref(s)

    entries = {"init": lib.nlam_forecast_init_strided, "head": lib.nlam_forecast_head_strided}
    for name, fn in entries.items():
        p, s = args()
        assert fn(None, s, None) == -1 and fn(p, None, None) == -1, name
    sizes = [dict(src_n_times=0), dict(nodes=0), dict(d_state=0), dict(d_forcing=-1), dict(batch=0), dict(max_lead=0),
             dict(num_past_forcing_steps=-1), dict(num_future_forcing_steps=-1), dict(src_members=0), dict(src_is_forecast=2)]
    pointers = [dict(lead=None), dict(src_state=None), dict(src_forcing=None), dict(src_sample_idx=None), dict(state_mean=None),
                dict(state_std=None), dict(forcing_mean=None), dict(forcing_std=None)]
    strides = [{f"src_{series}_stride_{axis}": -1} for series in ("state", "forcing") for axis in ("sample", "step", "member")]
    short = [dict(src_state_steps=off + LEAD - 1), dict(src_forcing_steps=off + LEAD + FUT - 1)]   # the lead-time axis of forecast data
    bad = {"init": sizes + pointers + strides + short + [dict(prev=None), dict(prev_prev=None)],
           "head": sizes + pointers + strides + short + [dict(truth=None), dict(forcing_windowed=None)]}
    for name, cases in bad.items():
        for kw in cases:
            assert entries[name](*args(**kw), None) == -1, (name, kw)
    # analysis data has one time axis: the sample stride is the step stride
    for name, fn in entries.items():
        ok = dict(src_is_forecast=0, src_n_times=16, src_state_stride_sample=3 * N * F, src_forcing_stride_sample=N * DF)
        assert fn(*args(**{**ok, "src_state_stride_sample": 7 * 3 * N * F}), None) == -1, name
        assert fn(*args(**{**ok, "src_forcing_stride_sample": 8 * N * DF}), None) == -1, name
    # the limits of the plain entry points
    for name, fn in entries.items():
        assert fn(*args(d_state=L.LOSS_MAX_VARS + 1), None) == -2, name
        assert fn(*args(d_forcing=L.LOSS_MAX_VARS + 1), None) == -2, name
        assert fn(*args(batch=65536), None) == -2, name
        assert fn(*args(nodes=(1 << 31) // F + 1), None) == -2, name


def test_dataset_planner_against_hand_computed_cases():
    from neural_lam_amd.data import plan_layout
    from neural_lam_amd.forecast import plan_forecast_dataset

    N, F = 37, 5
    # forecast data, past = 3 (off = 3), 4 analysis times x 3 members, resident for ar_steps = 4: every sample is a start
    lay = plan_layout((4, 9, 3, N, F), (4, 9, N, 2), is_forecast=True, ar_steps=4, num_past_forcing_steps=3, num_future_forcing_steps=1)
    assert (lay.state_steps, lay.forcing_steps) == (7, 8)
    assert plan_forecast_dataset(lay, 3, 1, 4, 4) == (3, 12, 3)      # max_lead == ar_steps
    assert plan_forecast_dataset(lay, 3, 1, 2, 4) == (3, 12, 3)      # a shorter horizon: the same starts
    with pytest.raises(ValueError, match="ar_steps"):
        plan_forecast_dataset(lay, 3, 1, 5, 4)                       # max_lead == ar_steps + 1
    lay = plan_layout((4, 9, 3, N, F), None, is_forecast=True, ar_steps=4, num_past_forcing_steps=1, num_future_forcing_steps=1)
    assert plan_forecast_dataset(lay, 1, 1, 4, 4) == (2, 12, 3)
    # analysis data with 3 members, 12 times: 12 - (2 + 4 + 1) + 1 = 6 starts per member, whatever ar_steps the dataset has
    lay = plan_layout((12, 3, N, F), (12, N, 2), ar_steps=1)
    assert plan_forecast_dataset(lay, 1, 1, 4, 1) == (2, 18, 3)
    assert plan_forecast_dataset(lay, 3, 0, 4, 1) == (3, 18, 3)      # 12 - (3 + 4 + 0) + 1 = 6
    assert plan_forecast_dataset(lay, 0, 2, 4, 1) == (2, 15, 3)      # 12 - (2 + 4 + 2) + 1 = 5
    assert plan_forecast_dataset(lay, 1, 1, 10, 1) == (2, 0, 3)      # too short a series: no valid start
    # load_single_member: member 0 only, the flat index is the sample
    with pytest.warns(UserWarning):
        lay = plan_layout((12, 3, N, F), (12, N, 2), ar_steps=1, load_single_member=True)
    assert plan_forecast_dataset(lay, 1, 1, 4, 1) == (2, 6, 1)
    with pytest.warns(UserWarning):
        lay = plan_layout((4, 9, 3, N, F), None, is_forecast=True, ar_steps=4, load_single_member=True)
    assert plan_forecast_dataset(lay, 1, 1, 4, 4) == (2, 4, 1)
    with pytest.raises(ValueError):
        plan_forecast_dataset(lay, 1, 1, 0, 4)


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


ANALYSES, MEMBERS, TIMES, NVARS, LEAD = 4, 3, 12, 5, 4


def _strided_dataset(dev, layout, forcing, past, fut, nodes, misalign, seed=0):
    """(A = 4, E, M = 3, N, 5) forecast data or (T = 12, M = 3, N, 5) analysis data; the lead-time axes are exactly as long as
    the dataset keeps resident, so that it keeps the tensors it is given (and their alignment)."""
    from neural_lam_amd.data import DeviceWeatherDataset

    g = torch.Generator().manual_seed(seed)
    off = max(2, past)
    d_forcing = 0 if forcing == "none" else 2
    lead_axes = lambda steps: (ANALYSES, steps) if layout == "forecast" else (TIMES,)   # noqa: E731
    put = _misaligned if misalign else (lambda t: t)
    state = put((torch.randn(*lead_axes(off + LEAD), MEMBERS, nodes, NVARS, generator=g) * 2.0 + 0.5).to(dev))
    forc = None
    if d_forcing:
        member_axis = (MEMBERS,) if forcing == "members" else ()
        forc = put((torch.randn(*lead_axes(off + LEAD + fut), *member_axis, nodes, d_forcing, generator=g) * 3.0 - 1.0).to(dev))
    stats = {"state_mean": torch.randn(NVARS, generator=g).to(dev), "state_std": (torch.rand(NVARS, generator=g) + 0.5).to(dev)}
    if d_forcing:
        stats.update(forcing_mean=torch.randn(d_forcing, generator=g).to(dev), forcing_std=(torch.rand(d_forcing, generator=g) + 0.5).to(dev))
    data = DeviceWeatherDataset(state, forc, ar_steps=LEAD, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                                standardization=stats, is_forecast=layout == "forecast")
    assert data.kernel == "nlam_window_batch_ens" and data.members == MEMBERS
    assert data.state.data_ptr() == state.data_ptr() and (forc is None or data.forcing.data_ptr() == forc.data_ptr())
    return data, stats, d_forcing


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,misalign", [(37, False), (36, False), (36, True)])
@pytest.mark.parametrize("forcing", ["members", "shared", "none"])
@pytest.mark.parametrize("layout", ["forecast", "analysis"])
@pytest.mark.parametrize("past,fut", WINDOWS)
def test_strided_head_and_init_give_the_bits_of_the_data_path(dev, past, fut, layout, forcing, nodes, misalign):
    """Every lead's forcing window and boundary truth, and the two initial states, against DeviceWeatherDataset.batch at
    ar_steps = max_lead (nlam_window_batch_ens with statistics): bit-equal.  nodes = 37: blocks of 185 floats, every other member's
    rows start off a 16-byte boundary (single elements); nodes = 36: blocks of 180 floats, the 16-byte path; misalign: the same with
    every base and every destination one float off (the fallback).  Indices outside the dataset read the rows of the clamped index."""
    from neural_lam_amd.forecast import dataset_source, plan_forecast_dataset

    lib = L.load()
    data, stats, d_forcing = _strided_dataset(dev, layout, forcing, past, fut, nodes, misalign)
    assert (data.state.data_ptr() % 16 == 4) == misalign and (nodes * NVARS % 4 == 0) == (nodes == 36)
    off, count, members = plan_forecast_dataset(data.layout, past, fut, LEAD, data.ar_steps)
    assert count == len(data) and members == MEMBERS and off == max(2, past)
    put = _misaligned if misalign else (lambda t: t)
    window = past + fut + 1
    B = 3
    nan = lambda *shape: put(torch.full(shape, float("nan"), device=dev))   # noqa: E731
    prev, pprev, truth, fw = nan(B, nodes, NVARS), nan(B, nodes, NVARS), nan(B, nodes, NVARS), nan(B, nodes, d_forcing * window)
    idx = torch.zeros(B, dtype=torch.int64, device=dev)
    lead = torch.full((1,), 7, dtype=torch.int32, device=dev)
    p = L.Forecast()
    p.lead = _ptr(lead)
    p.state_mean, p.state_std = _ptr(stats["state_mean"]), _ptr(stats["state_std"])
    p.forcing_mean, p.forcing_std = _ptr(stats.get("forcing_mean")), _ptr(stats.get("forcing_std"))
    p.prev, p.prev_prev, p.truth, p.forcing_windowed = _ptr(prev), _ptr(pprev), _ptr(truth), (_ptr(fw) if d_forcing else None)
    p.nodes, p.d_state, p.d_forcing, p.batch = nodes, NVARS, d_forcing, B
    p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps = LEAD, past, fut
    s = dataset_source(data, idx)
    inside = [1, count // 2, count - 1]   # three distinct (sample, member), the last valid one among them
    assert len({(i // MEMBERS, i % MEMBERS) for i in inside}) == 3 and len({i % MEMBERS for i in inside}) >= 2
    for given, read in ((inside, inside), ([count + 7, -5, count], [count - 1, 0, count - 1])):
        init, target, forc, _ = data.batch(read, standardize=True)
        idx.copy_(torch.tensor(given, dtype=torch.int64))
        lead.fill_(7)
        for t in (prev, pprev):
            t.fill_(float("nan"))
        L.check(lib.nlam_forecast_init_strided(C.byref(p), C.byref(s), _stream()), "nlam_forecast_init_strided")
        assert int(lead) == 0
        assert torch.equal(_bits(pprev), _bits(init[:, 0])) and torch.equal(_bits(prev), _bits(init[:, 1]))
        for k in range(LEAD):
            lead.fill_(k)
            truth.fill_(float("nan"))
            fw.fill_(float("nan"))
            L.check(lib.nlam_forecast_head_strided(C.byref(p), C.byref(s), _stream()), "nlam_forecast_head_strided")
            assert torch.equal(_bits(truth), _bits(target[:, k])), (given, k)
            if d_forcing:
                assert torch.equal(_bits(fw), _bits(forc[:, k])), (given, k)
            assert int(lead) == k   # the head only reads the counter
    # a replay too many writes nothing, and only init writes the counter
    lead.fill_(LEAD)
    truth.fill_(float("nan"))
    fw.fill_(float("nan"))
    L.check(lib.nlam_forecast_head_strided(C.byref(p), C.byref(s), _stream()), "nlam_forecast_head_strided")
    assert bool(torch.isnan(truth).all()) and bool(torch.isnan(fw).all()) and int(lead) == LEAD


# ---------------------------------------------------------------------------
# GPU: the engines
# ---------------------------------------------------------------------------
E_TIMES, E_LEAD, E_ANALYSES, E_MEMBERS = 13, 4, 4, 3
E_PICKS = [(1, 2), (3, 0)]   # (analysis time, member) of the two forecasts of a batch; the second is the last analysis time


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """The 30 x 27 SyntheticDatastore of the existing engine tests and one plain 13-step series X_m per member, with its forcing."""
    from neural_lam_amd.datastore import SyntheticDatastore

    root = tmp_path_factory.mktemp("forecast_datasets")
    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=root, boundary="random", seed=1)
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(23)
    w = types.SimpleNamespace(ds=ds, N=N, root=root)
    w.state = torch.randn(E_MEMBERS, E_TIMES, N, 5, generator=g).to(dev)     # X_m
    w.forcing = torch.randn(E_MEMBERS, E_TIMES, N, 2, generator=g).to(dev)
    w.dt = 10
    w.times = (torch.arange(E_TIMES, dtype=torch.int64) * w.dt + 1000).to(dev)
    return w


def _datasets(world, step, layout, shared_forcing, ar_steps=E_LEAD):
    """The strided dataset and the plain dataset of every member.  forecast: block (a, e, m) is X_m[a * 2 + e], so that flat sample
    a * M + m is plain start 2 a of X_m; analysis: block (t, m) is X_m[t], flat sample s * M + m is plain start s of X_m.  A shared
    forcing is member 0's for every member."""
    from neural_lam_amd.data import DeviceWeatherDataset

    stats = step.standardization_stats()
    forcing = world.forcing[:1].expand(E_MEMBERS, -1, -1, -1) if shared_forcing else world.forcing
    plain = [DeviceWeatherDataset(world.state[m].contiguous(), forcing[m].contiguous(), world.times, ar_steps=ar_steps, standardization=stats)
             for m in range(E_MEMBERS)]
    if layout == "analysis":
        st, fo = world.state.transpose(0, 1), forcing.transpose(0, 1)                     # (T, M, N, F)
        data = DeviceWeatherDataset(st.contiguous(), fo[:, 0].contiguous() if shared_forcing else fo.contiguous(), world.times,
                                    ar_steps=ar_steps, standardization=stats)
        return data, plain, lambda a, m: (a * E_MEMBERS + m, a)
    E = 2 + ar_steps + 1
    rows = (torch.arange(E_ANALYSES)[:, None] * 2 + torch.arange(E)[None]).to(world.state.device)   # (A, E): the time a * 2 + e
    st, fo = world.state[:, rows].permute(1, 2, 0, 3, 4), forcing[:, rows].permute(1, 2, 0, 3, 4)   # (A, E, M, N, F)
    data = DeviceWeatherDataset(st.contiguous(), fo[:, :, 0].contiguous() if shared_forcing else fo.contiguous(),
                                world.times[::2][:E_ANALYSES].contiguous(), ar_steps=ar_steps, standardization=stats, is_forecast=True,
                                elapsed=torch.arange(E, dtype=torch.int64) * world.dt)
    return data, plain, lambda a, m: (a * E_MEMBERS + m, 2 * a)


def _make_step(world, dev, options, seed=1):
    from neural_lam_amd import models as hm

    if "graph" not in vars(world):
        world.graph = _graph_of(world.ds)
    kw = dict(_clamp_kw(world.ds), output_std=True) if options == "clamps_std" else {}
    torch.manual_seed(seed)
    predictor = hm.MODELS["graph_lam"](world.ds, graph=world.graph, hidden_dim=16, processor_layers=2, **kw)
    return hm.ForecasterStep(hm.ARForecaster(predictor, world.ds), world.ds).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["forecast", "analysis"])
@pytest.mark.parametrize("options", ["plain", "clamps_std"])
def test_engine_on_a_strided_dataset_equals_the_plain_engine_and_the_rollout(dev, world, options, layout):
    """Forecast.run from (a, m) of a strided dataset against the plain engine on X_m from the matching start, in the same batch
    position: state, std, sq and ab bit-identical, the valid times those of dataset.batch, as many launches per lead.  Against
    step.forecaster and step.evaluate on dataset.batch: the bars of test_engine_matches_the_existing_rollout_and_evaluate."""
    from neural_lam_amd.forecast import Forecast

    step = _make_step(world, dev, options)
    data, plain, match = _datasets(world, step, layout, shared_forcing=options == "clamps_std")
    fc = Forecast(step, data, E_LEAD, batch_size=2, verify=True)
    assert fc.n_starts == (len(data) if layout == "forecast" else (E_TIMES - (2 + E_LEAD + 1) + 1) * E_MEMBERS)
    flat = [match(a, m)[0] for a, m in E_PICKS]
    res = fc.run(flat)
    init, target, forcing, target_times = data.batch(flat, standardize=True)
    assert torch.equal(res.valid_times, target_times)
    stamps = torch.tensor([[1000 + world.dt * (match(a, m)[1] + 2 + k) for k in range(E_LEAD)] for a, m in E_PICKS])
    assert torch.equal(res.valid_times.cpu(), stamps)
    assert (res.std is not None) == (options == "clamps_std")
    for b, (a, m) in enumerate(E_PICKS):
        ref = Forecast(step, plain[m], E_LEAD, batch_size=2, verify=True)
        starts = [0, 0]
        starts[b] = match(a, m)[1]
        want = ref.run(starts)
        assert ref.launches_per_lead == fc.launches_per_lead
        for name in ("state", "std", "sq", "ab", "valid_times"):
            got_t, want_t = getattr(res, name), getattr(want, name)
            if want_t is None:
                assert got_t is None
                continue
            assert torch.equal(_bits(got_t[b]), _bits(want_t[b])), (name, b)
    # the existing rollout and evaluation on the dataset's own batch
    with torch.no_grad():
        want, want_std = step.forecaster(init, forcing, target)
    ev = step.evaluate(init, target, forcing, phase="test", standardize=False)
    torch.cuda.synchronize()
    got = (res.state - step.state_mean) / step.state_std
    assert rel_err(got, want) <= 1e-4
    if options == "clamps_std":
        assert rel_err(res.std / step.state_std, want_std) <= 1e-4
    tol = (world.N + 8) * EPS32
    assert bool(((res.sq - ev.entry_mse).abs() <= tol * ev.entry_mse.abs()).all())
    assert bool(((res.ab - ev.entry_mae).abs() <= tol * ev.entry_mae.abs()).all())


@pytest.mark.gpu
def test_engine_refusals_and_indices_on_strided_datasets(dev, world):
    from neural_lam_amd.forecast import Forecast

    step = _make_step(world, dev, "plain")
    data, _, match = _datasets(world, step, "forecast", shared_forcing=False, ar_steps=2)
    with pytest.raises(ValueError, match="ar_steps"):
        Forecast(step, data, 3, batch_size=2)              # forecast data keeps ar_steps lead times resident
    fc = Forecast(step, data, 2, batch_size=2, use_graph=False)
    assert fc.n_starts == len(data) == E_ANALYSES * E_MEMBERS
    with pytest.raises(IndexError):
        fc.run([0, fc.n_starts])
    with pytest.raises(IndexError):
        fc.run([-fc.n_starts - 1, 0])
    last = fc.run([-1, 0]).state.clone()                   # negative host indices count from the end
    assert torch.equal(_bits(last), _bits(fc.run(torch.tensor([fc.n_starts - 1, 0], device=dev)).state))
    data, _, _ = _datasets(world, step, "analysis", shared_forcing=True, ar_steps=1)
    fc = Forecast(step, data, E_LEAD, batch_size=1, use_graph=False)    # analysis data: the dataset's ar_steps is ignored
    assert fc.n_starts == (E_TIMES - (2 + E_LEAD + 1) + 1) * E_MEMBERS
    with pytest.raises(IndexError):
        fc.run([fc.n_starts])


ENS_LEAD, ENS_MODEL_MEMBERS = 3, 3


@pytest.mark.gpu
def test_ensemble_engine_on_a_strided_dataset(dev, world):
    """EnsembleForecast with a Graph-EFM, 2 starts x 3 members, 3 leads, on forecast-type data with 3 data members.  Given
    latent_noise: bit-identical to the plain engine on the matching series, start by start (the same batch position).  With the
    generator: a start's members have the same bits alone and in a batch with another start, with and without the graph."""
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm
    from neural_lam_amd.forecast import EnsembleForecast

    G.save_graph(world.root / "graph" / "hierarchical",
                 G.create_regular_grid_graph(world.ds.get_xy("state"), n_max_levels=3, hierarchical=True))
    torch.manual_seed(5)
    model = graph_efm.GraphEFM(world.ds, hidden_dim=8)
    step = hm.ForecasterStep(hm.ARForecaster(model, world.ds), world.ds).to(dev)
    data, plain, match = _datasets(world, step, "forecast", shared_forcing=False, ar_steps=ENS_LEAD)
    S, M = len(E_PICKS), ENS_MODEL_MEMBERS
    flat = [match(a, m)[0] for a, m in E_PICKS]
    mk = lambda ds, n_starts=S, **kw: EnsembleForecast(step, ds, ENS_LEAD, members=M, n_starts=n_starts, seed=11, **kw)   # noqa: E731
    ens = mk(data)
    g = torch.Generator().manual_seed(3)
    noise = torch.randn(ENS_LEAD, S * M, *ens.latent.shape[1:], generator=g).to(dev)
    res = ens.run(flat, latent_noise=noise)
    _, _, _, target_times = data.batch(flat, standardize=True)
    assert torch.equal(res.valid_times, target_times)
    per_batch = ("state", "sq", "ab")
    per_start = ("mean", "spread", "ens_sq", "ens_var", "ens_abs", "ens_pair", "rank_hist")
    for s, (a, m) in enumerate(E_PICKS):
        ref = mk(plain[m])
        starts = [0, 0]
        starts[s] = match(a, m)[1]
        want = ref.run(starts, latent_noise=noise)
        assert ref.launches_per_lead == ens.launches_per_lead
        for name in per_batch:
            assert torch.equal(_bits(getattr(res, name)[s * M:(s + 1) * M]), _bits(getattr(want, name)[s * M:(s + 1) * M])), (name, s)
        for name in per_start:
            assert torch.equal(_bits(getattr(res, name)[s]), _bits(getattr(want, name)[s])), (name, s)
    # the generator: counted by (lead, member, flat sample index)
    both = ens.run(flat).members.clone()
    assert not torch.equal(_bits(both[0, 0]), _bits(both[0, 1]))                        # the members differ
    assert torch.equal(_bits(both), _bits(mk(data, use_graph=False).run(flat).members))
    alone = mk(data, n_starts=1)
    for s in range(S):
        assert torch.equal(_bits(both[s]), _bits(alone.run([flat[s]]).members[0])), s
    swapped = ens.run(flat[::-1]).members
    assert torch.equal(_bits(both), _bits(swapped.flip(0)))
