"""Per-lead DCT variance spectra from the forecast engines (Forecast / EnsembleForecast(spectra=..., grid_shape=...,
spectra_window=...)) on small lattices of their own (13 x 11 and 9 x 12 nodes) with statistics that are not (0, 1).

The launch reads the standardised state of the lead; the engine returns the physical fields.  Where the launch's exact input is
at hand -- the ensemble mean slots, and ``engine.prev`` / ``engine.truth`` after the last lead -- the spectrum is held to the
budget of spectra_ref.py alone.  Where the reference starts from the returned physical field x = fl(fl(prev * std) + mean) (or
the analysis, standardised by the head launch as fl((x - mean) / std)), the input of reference and launch differ by those
roundings: at most 3 u (|x| + |mean|) / std in standardised units, which through the transform is at most
e_in = 3 u |Cx| ((|x| + |mean|) / std) |Cy^T| per coefficient, that is std^2 / (cx cy) sum_bin (2 |G| e_in + e_in^2) more per bin."""
import types

import numpy as np
import pytest
import scipy.fft
import torch

import spectra_ref as R
from neural_lam_amd import _lib as L

LEADS = 3
MEAN = [0.3, -1.0, 0.0, 2.0, 0.1]
STD = [2.0, 0.5, 1.0, 3.0, 0.25]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _world(dev, root, nx, ny, efm=False, times=12):
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    ds = SyntheticDatastore(nx, ny, 5, 2, 1, root_path=root, boundary="random", seed=1)
    assert (ds.nx, ds.ny) == (nx, ny)
    ext = ds.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))
    torch.manual_seed(1)
    if efm:
        predictor = graph_efm.GraphEFMMultiScale(ds, graph=graph, hidden_dim=16, latent_dim=4)
    else:
        predictor = hm.MODELS["graph_lam"](ds, graph=graph, hidden_dim=16, processor_layers=2)
    step = hm.ForecasterStep(hm.ARForecaster(predictor, ds), ds).to(dev)
    step.state_mean.copy_(torch.tensor(MEAN))
    step.state_std.copy_(torch.tensor(STD))
    g = torch.Generator().manual_seed(11)
    w = types.SimpleNamespace(ds=ds, step=step, N=nx * ny, nx=nx, ny=ny)
    w.state = torch.randn(times, w.N, 5, generator=g).to(dev) * step.state_std + step.state_mean
    w.forcing = torch.randn(times, w.N, 2, generator=g).to(dev)
    w.times = (torch.arange(times, dtype=torch.int64) * 10 + 1000).to(dev)
    return w


def _reference(field, f, win, scale_std, phys_input):
    """``field`` (nx, ny) float64 in the units the launch reads (standardised: ``scale_std`` True, or physical).  ``phys_input``:
    the physical field the standardised one was computed from, when the reference did not get the launch's own input."""
    i0, i1, j0, j1 = win
    g = field[i0:i1, j0:j1]
    cx, cy = g.shape
    nb, bins = min(cx, cy), R.bins_ref(cx, cy)
    scale = STD[f] ** 2 if scale_std else 1.0
    spec, budget = R.spectra_ref(g, bins, nb, scale)
    if phys_input is not None:
        G = np.abs(scipy.fft.dctn(g, type=2, norm="ortho"))
        dx = 3 * R.U * (np.abs(phys_input[i0:i1, j0:j1]) + abs(MEAN[f])) / STD[f]
        e_in = np.abs(R.basis_ref(cx)) @ dx @ np.abs(R.basis_ref(cy)).T
        per = (2 * G * e_in + e_in ** 2) * (scale / (cx * cy))
        budget = budget + np.bincount(bins[bins >= 0], weights=per[bins >= 0], minlength=nb)
    return spec, budget, scale * g.var()


def _check(got, fields, var, win, nx, ny, what, standardised=None):
    """``got`` (B, V, nb) device; ``fields`` (B, N, F): physical (``standardised`` None: the reference standardises them in float64
    and allows for the launch's fp32 input roundings), or with ``standardised`` True / False the launch's own input."""
    got = got.cpu().double().numpy()
    x = fields.cpu().double().numpy().reshape(fields.shape[0], nx, ny, -1)
    worst = 0.0
    for b in range(x.shape[0]):
        for v, f in enumerate(var):
            if standardised is None:
                spec, budget, var_ref = _reference((x[b, ..., f] - MEAN[f]) / STD[f], f, win, True, x[b, ..., f])
            else:
                spec, budget, var_ref = _reference(x[b, ..., f], f, win, standardised, None)
            err = np.abs(got[b, v] - spec)
            worst = max(worst, float((err / budget).max()))
            assert bool((err <= budget).all()), (what, b, v, float((err / budget).max()))
            assert bool((budget <= 0.05 * spec).all()), (what, b, v)   # the budget is no free pass
            # the bins add up to the variance of the window (Parseval), within the summed budgets
            assert abs(got[b, v].sum() - var_ref) <= budget.sum() + 1e-12 * var_ref, (what, b, v)
    print(f"spectra engine {what}: worst error / budget {worst:.3e}")


def _analysis(w, fc, starts, k):
    """The analysis rows of lead k (physical) of the dataset."""
    from neural_lam_amd.forecast import plan_forecast

    off, _ = plan_forecast(w.state.shape[0], 1, 1, fc.max_lead)
    t0 = torch.tensor(starts) + off - 1
    return w.state[t0.to(w.state.device) + k + 1]


@pytest.mark.gpu
def test_forecast_spectra_against_the_reference_graph_and_eager(dev, tmp_path):
    from neural_lam_amd.forecast import Forecast
    from test_ensemble_forecast import _dataset

    nx, ny, win, moved = 13, 11, (1, 12, 2, 10), (2, 13, 1, 9)
    w = _world(dev, tmp_path, nx, ny)
    step, data = w.step, _dataset(w)
    names = step.state_var_names
    var = [3, 0]
    kw = dict(batch_size=2, verify=True)
    sp_kw = dict(spectra=[names[3], 0], grid_shape=(nx, ny), spectra_window=win)
    fc = Forecast(step, data, LEADS, **sp_kw, **kw)
    plain = Forecast(step, data, LEADS, **kw)
    none = Forecast(step, data, LEADS, spectra=None, grid_shape=(nx, ny), spectra_window=win, **kw)
    assert Forecast.SPECTRA_LAUNCHES == 3
    assert none.launches_per_lead == plain.launches_per_lead and none._sp is None and not hasattr(none, "spectra_workspace")
    assert fc.launches_per_lead == plain.launches_per_lead + 3
    starts = [1, 4]
    res = fc.run(starts)
    sp = res.spectra
    nb = 8
    assert plain.run(starts).spectra is None
    assert sp.forecast.shape == (2, LEADS, 2, nb) == sp.analysis.shape and sp.mean is None and sp.variables == (3, 0)
    assert sp.window == win and torch.equal(sp.wavenumber[:-1], torch.arange(1, nb, dtype=torch.float64) / nb)
    assert bool(torch.isnan(sp.wavenumber[-1])) and float(sp.wavelength(2.5)[0]) == 2 * 2.5 * nb
    assert torch.equal(_bits(res.state), _bits(plain.run(starts).state))   # the forecast itself keeps its bits
    for k in range(LEADS):
        _check(sp.forecast[:, k], res.state[:, k], var, win, nx, ny, ("forecast", k))
        _check(sp.analysis[:, k], _analysis(w, fc, starts, k), var, win, nx, ny, ("analysis", k))
    # after the last lead the engine's buffers are the launch's own input: the budget alone
    _check(sp.forecast[:, LEADS - 1], fc.prev, var, win, nx, ny, "forecast, own input", standardised=True)
    _check(sp.analysis[:, LEADS - 1], fc.truth, var, win, nx, ny, "analysis, own input", standardised=True)
    # graph and eager issue the same launches: equal bits
    first = {k: getattr(sp, k).clone() for k in ("forecast", "analysis")}
    eager = Forecast(step, data, LEADS, use_graph=False, **sp_kw, **kw)
    es = eager.run(starts).spectra
    assert eager.launches_per_lead is None
    assert all(torch.equal(_bits(first[k]), _bits(getattr(es, k))) for k in first)
    # fewer leads: cut
    fc.spec_out["forecast"].fill_(-7.0)
    short = fc.run(starts, leads=2).spectra
    assert short.forecast.shape == (2, 2, 2, nb) == short.analysis.shape
    assert torch.equal(_bits(short.forecast), _bits(first["forecast"][:, :2])) and bool((fc.spec_out["forecast"][:, 2] == -7.0).all())
    # a moved window of the same size: no new recording
    graph = fc._graph
    fc.set_spectra_window(moved)
    res2 = fc.run(starts)
    assert fc._graph is graph and res2.spectra.window == moved
    assert not torch.equal(_bits(res2.spectra.forecast), _bits(first["forecast"]))
    for k in range(LEADS):
        _check(res2.spectra.forecast[:, k], res2.state[:, k], var, moved, nx, ny, ("moved forecast", k))
        _check(res2.spectra.analysis[:, k], _analysis(w, fc, starts, k), var, moved, nx, ny, ("moved analysis", k))
    for bad in ((1, 12, 2, 11), (0, 12, 2, 10), (1, 12, 2, 10, 0), (3, 14, 2, 10)):
        with pytest.raises(ValueError, match="spectra_window"):
            fc.set_spectra_window(bad)
    with pytest.raises(ValueError, match="without spectra"):
        plain.set_spectra_window(win)
    fc.set_spectra_window(win)
    assert torch.equal(_bits(fc.run(starts).spectra.forecast), _bits(first["forecast"]))


@pytest.mark.gpu
def test_launches_grow_by_three_at_another_size(dev, tmp_path):
    from neural_lam_amd.forecast import Forecast
    from test_ensemble_forecast import _dataset

    w = _world(dev, tmp_path, 9, 12)
    data = _dataset(w)
    plain = Forecast(w.step, data, LEADS, batch_size=1)
    for kw in (dict(spectra=[0, 1, 2, 3, 4]), dict(spectra=[2], spectra_window=(0, 2, 3, 5))):
        fc = Forecast(w.step, data, LEADS, batch_size=1, grid_shape=(9, 12), **kw)
        assert fc.launches_per_lead == plain.launches_per_lead + Forecast.SPECTRA_LAUNCHES
    whole = Forecast(w.step, data, LEADS, batch_size=1, grid_shape=(9, 12), spectra=[4, 1])
    res = whole.run([2])
    for k in range(LEADS):
        _check(res.spectra.forecast[:, k], res.state[:, k], [4, 1], (0, 9, 0, 12), 9, 12, ("9 x 12 whole", k))


@pytest.mark.gpu
def test_ensemble_spectra_members_mean_and_analysis(dev, tmp_path):
    from neural_lam_amd.forecast import EnsembleForecast
    from test_ensemble_forecast import _dataset

    nx, ny, win = 13, 11, (1, 12, 1, 10)
    w = _world(dev, tmp_path, nx, ny, efm=True)
    step, data = w.step, _dataset(w)
    S, M, starts, var = 2, 3, [1, 4], [1, 4, 2]
    kw = dict(members=M, n_starts=S, seed=5)
    extra = dict(events=[(0, ">", 0.5), (3, "<", 1.0)], neighbourhoods=[0, 2], grid_shape=(nx, ny))
    ens = EnsembleForecast(step, data, LEADS, spectra=var, spectra_window=win, **extra, **kw)
    assert ens.samples
    plain = EnsembleForecast(step, data, LEADS, **kw)
    both = EnsembleForecast(step, data, LEADS, **extra, **kw)
    only = EnsembleForecast(step, data, LEADS, spectra=var, grid_shape=(nx, ny), spectra_window=win, **kw)
    assert EnsembleForecast(step, data, LEADS, spectra=None, **kw).launches_per_lead == plain.launches_per_lead
    assert only.launches_per_lead == plain.launches_per_lead + 3
    assert ens.launches_per_lead == both.launches_per_lead + 3   # composed with the products and the neighbourhoods
    res = ens.run(starts)
    sp = res.spectra
    nb = 9
    assert sp.forecast.shape == (S * M, LEADS, 3, nb) and sp.analysis.shape == (S, LEADS, 3, nb) == sp.mean.shape
    base = both.run(starts)
    assert base.spectra is None
    assert torch.equal(_bits(res.state), _bits(base.state)) and torch.equal(_bits(res.products.nprob), _bits(base.products.nprob))
    assert torch.equal(_bits(only.run(starts).spectra.forecast), _bits(sp.forecast))
    for k in range(LEADS):
        _check(sp.forecast[:, k], res.state[:, k], var, win, nx, ny, ("members", k))
        _check(sp.mean[:, k], res.mean[:, k], var, win, nx, ny, ("mean", k), standardised=False)   # the launch's own input
        _check(sp.analysis[:, k], _analysis(w, ens, starts, k), var, win, nx, ny, ("analysis", k))
    # the members keep variance the mean has lost
    assert bool((sp.forecast.view(S, M, LEADS, 3, nb).sum(-1).mean(1) >= (1 - 1e-5) * sp.mean.sum(-1)).all())
    short = ens.run(starts, leads=1).spectra
    assert short.mean.shape == (S, 1, 3, nb) and torch.equal(_bits(short.mean), _bits(sp.mean[:, :1]))
    with pytest.raises(ValueError, match="grid_shape"):   # one grid_shape serves neighbourhoods and spectra, and it must hold the nodes
        EnsembleForecast(step, data, LEADS, spectra=var, grid_shape=(ny, nx + 1), **kw)
