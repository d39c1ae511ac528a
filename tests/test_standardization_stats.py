"""Standardization statistics on the device data path (neural_lam_amd.stats, nlam_window_moments).

The reference (neural_lam/datastore/npyfilesmeps/compute_standardization_stats.py) cannot run here (it needs xarray), so
it is restated in this file, in two forms:
  * numpy float64 over the raw series (independent of the dataset code): per-sample means and second moments of the
    ar_steps + 2 state rows and of the ar_steps forcing rows (window 1: rows 2 ... ar_steps + 1); the mean of the
    per-sample means; std = sqrt(mean of second moments - mean^2) clamped at 0; standardized one-step differences
    ((x - mean) / std in fp32, exactly the reference's inline standardisation, then consecutive differences of the rows
    k, k + step, ... < used for every k < step, used = ((ar_steps + 2) // step) * step) reduced in float64; the flux as
    the mean over batches of batch_size consecutive samples of each batch's mean.
  * the reference's own fp32 torch formulas on the CPU over the dataset's batches (what its script would write).
Tolerances of the float64 comparison: |got - want| <= 1e-6 * (|want| + spread) for means and 1e-5 * want for stds, the
spread being the std of the quantity (a mean near 0 is judged against the scale of the data, not against itself).
"""
import os
import socket
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


# ---- host-only (no GPU) ----
def _layout(**kw):
    from neural_lam_amd.stats import stats_layout

    args = dict(state_shape=(4, 9, 2, 30, 5), forcing_shape=(4, 9, 2, 30, 3), is_forecast=True, ar_steps=7)
    args.update(kw)
    return stats_layout(args.pop("state_shape"), args.pop("forcing_shape"), **args)


def test_plan_statistics_rejects_what_the_reference_would_not_compute():
    from neural_lam_amd.stats import plan_statistics

    ok = _layout()
    with pytest.raises(ValueError, match="num_past_forcing_steps"):
        plan_statistics(_layout(num_past_forcing_steps=1))
    with pytest.raises(ValueError, match="num_past_forcing_steps"):
        plan_statistics(_layout(num_future_forcing_steps=1, forcing_shape=(4, 10, 2, 30, 3)))
    with pytest.raises(ValueError, match="step_length"):
        plan_statistics(ok, step_length=0)
    with pytest.raises(ValueError, match="no consecutive pair"):
        plan_statistics(ok, step_length=5)   # 9 rows // 5 = 1 row per sub-sequence
    plan_statistics(ok, step_length=4)       # 9 // 4 = 2: one pair
    with pytest.raises(ValueError, match="flux_index"):
        plan_statistics(ok, flux_index=3)
    with pytest.raises(ValueError, match="flux_index"):
        plan_statistics(ok, flux_index=-1)
    plan_statistics(_layout(forcing_shape=None), flux_index=7)   # no forcing: no flux
    with pytest.raises(ValueError, match="batch_size"):
        plan_statistics(ok, batch_size=0)
    with pytest.raises(ValueError, match="257 state features"):
        plan_statistics(_layout(state_shape=(4, 9, 2, 30, 257)))
    with pytest.raises(ValueError, match="300 forcing features"):
        plan_statistics(_layout(forcing_shape=(4, 9, 2, 30, 300)))


def test_plan_statistics_flux_batches_and_rows():
    from neural_lam_amd.stats import plan_statistics

    # 5 analysis times x 2 members = 10 samples; batches of 4 leave a short last batch
    plan = plan_statistics(_layout(state_shape=(5, 9, 2, 30, 5), forcing_shape=(5, 9, 30, 3)), step_length=3,
                           batch_size=4)
    assert plan.n_samples == 10
    assert plan.flux_batches == ((0, 4), (4, 8), (8, 10))
    assert plan.diff_rows_per_sample == 3 and plan.pairs == 2   # 9 rows: sub-sequences of 3 rows
    with pytest.warns(UserWarning, match="only using first ensemble member"):
        single = plan_statistics(_layout(state_shape=(5, 9, 2, 30, 5), load_single_member=True,
                                         forcing_shape=(5, 9, 2, 30, 3)), batch_size=32)
    assert single.n_samples == 5 and single.flux_batches == ((0, 5),)
    # analysis data: len = T - (ar + 2) + 1
    ana = plan_statistics(_layout(state_shape=(20, 30, 5), forcing_shape=(20, 30, 3), is_forecast=False), step_length=1)
    assert ana.n_samples == 20 - 9 + 1 and ana.pairs == 8


def test_save_load_round_trip_in_the_reference_layout(tmp_path):
    from neural_lam_amd.stats import load_standardization_stats, save_standardization_stats

    d = 17
    stats = {
        "state_mean": torch.linspace(-3, 3, d), "state_std": torch.linspace(0.5, 2, d),
        "state_diff_mean_standardized": torch.linspace(-0.1, 0.1, d), "state_diff_std_standardized": torch.linspace(0.2, 1, d),
        "forcing_mean": torch.arange(6.0), "forcing_std": torch.arange(1.0, 7.0), "flux_stats": torch.tensor([1.5, 0.25]),
    }
    static = tmp_path / "static"
    save_standardization_stats(static, stats)
    assert sorted(p.name for p in static.iterdir()) == sorted(
        ["parameter_mean.pt", "parameter_std.pt", "diff_mean.pt", "diff_std.pt", "flux_stats.pt"])
    # what the reference's store reads (store.py get_standardization_dataarray: torch.load(weights_only=True).numpy())
    for name, key in (("parameter_mean.pt", "state_mean"), ("parameter_std.pt", "state_std"),
                      ("diff_mean.pt", "state_diff_mean_standardized"), ("diff_std.pt", "state_diff_std_standardized")):
        t = torch.load(static / name, weights_only=True)
        assert t.dtype == torch.float32 and t.shape == (d,) and t.device.type == "cpu"
        assert torch.equal(t, stats[key])
        assert t.numpy().dtype == np.float32
    flux = torch.load(static / "flux_stats.pt", weights_only=True)
    assert flux.dtype == torch.float32 and flux.shape == (2,) and torch.equal(flux, stats["flux_stats"])

    back = load_standardization_stats(static, num_forcing=6)
    for key in ("state_mean", "state_std", "state_diff_mean_standardized", "state_diff_std_standardized"):
        assert back[key].dtype == torch.float32 and torch.equal(back[key], stats[key])
    # the MEPS forcing rule: flux first, then mean 0 / std 1
    assert torch.equal(back["forcing_mean"], torch.tensor([1.5, 0, 0, 0, 0, 0]))
    assert torch.equal(back["forcing_std"], torch.tensor([0.25, 1, 1, 1, 1, 1]))
    no_forcing = load_standardization_stats(static, num_forcing=0)
    assert "forcing_mean" not in no_forcing and torch.equal(no_forcing["state_std"], stats["state_std"])


def test_synthetic_datastore_takes_forcing_stats():
    from neural_lam_amd.datastore import SyntheticDatastore

    default = SyntheticDatastore(6, 5, 4, 3, 1)
    fs = default.get_standardization_dataarray("forcing")
    assert np.array_equal(fs.forcing_mean.values, np.zeros(3, np.float32))
    assert np.array_equal(fs.forcing_std.values, np.ones(3, np.float32))
    st = default.get_standardization_dataarray("state")
    assert np.array_equal(st.state_std.values, np.ones(4, np.float32))

    ds = SyntheticDatastore(6, 5, 4, 3, 1, forcing_stats={"forcing_mean": [1.0, 2.0, 3.0], "forcing_std": torch.tensor([4.0, 5.0, 6.0])})
    fs = ds.get_standardization_dataarray("forcing")
    assert fs.forcing_mean.values.dtype == np.float32 and np.array_equal(fs.forcing_mean.values, [1, 2, 3])
    assert np.array_equal(fs.forcing_std.values, [4, 5, 6])
    assert np.array_equal(ds.get_standardization_dataarray("state").state_mean.values, np.zeros(4, np.float32))


# ---- the float64 restatement ----
def _samples(state, forcing, is_forecast, ar, single):
    """(state rows (ar + 2, N, F), forcing rows (ar, N, Ff) or None) of every flat sample, in dataset order."""
    lead = 1 if is_forecast else 0
    sm = state.ndim == 4 + lead
    M = state.shape[lead + 1] if sm and not single else 1
    fm = forcing is not None and forcing.ndim == 4 + lead
    if is_forecast:
        base = state.shape[0]
    else:
        T = state.shape[0] if forcing is None else min(state.shape[0], forcing.shape[0])
        base = T - (ar + 2) + 1
    out = []
    for idx in range(base * M):
        s, m = divmod(idx, M)
        st = np.take(state, m, axis=lead + 1) if sm else state
        seq = st[s, : ar + 2] if is_forecast else st[s : s + ar + 2]
        frc = None
        if forcing is not None:
            fo = np.take(forcing, m, axis=lead + 1) if fm else forcing
            frc = fo[s, 2 : ar + 2] if is_forecast else fo[s + 2 : s + ar + 2]
        out.append((seq, frc))
    return out


def _mean_std64(means, sqs):
    mean = means.mean(0)
    return mean, np.sqrt(np.maximum(sqs.mean(0) - mean * mean, 0.0))


def restate64(state, forcing, *, is_forecast, ar, step, batch_size, flux_index=0, single=False):
    samples = _samples(state, forcing, is_forecast, ar, single)
    red = lambda x: (x.astype(np.float64).mean(axis=(0, 1)), (x.astype(np.float64) ** 2).mean(axis=(0, 1)))  # noqa: E731
    vals = [red(s) for s, _ in samples]
    mean, std = _mean_std64(np.stack([v[0] for v in vals]), np.stack([v[1] for v in vals]))
    m32, s32 = mean.astype(np.float32), std.astype(np.float32)
    used = ((ar + 2) // step) * step
    dm, dq = [], []
    for seq, _ in samples:
        z = (seq.astype(np.float32) - m32) / s32          # fp32, as the reference standardizes inline
        for k in range(step):
            sub = z[k:used:step]
            d = sub[1:] - sub[:-1]                          # fp32 difference
            dm.append(red(d)[0])
            dq.append(red(d)[1])
    out = {"state_mean": mean, "state_std": std}
    out["state_diff_mean_standardized"], out["state_diff_std_standardized"] = _mean_std64(np.stack(dm), np.stack(dq))
    if forcing is not None:
        fv = [red(f) for _, f in samples]
        fmeans, fsqs = np.stack([v[0] for v in fv]), np.stack([v[1] for v in fv])
        out["forcing_mean"], out["forcing_std"] = _mean_std64(fmeans, fsqs)
        n = len(samples)
        bm = [fmeans[b : b + batch_size, flux_index].mean() for b in range(0, n, batch_size)]
        bq = [fsqs[b : b + batch_size, flux_index].mean() for b in range(0, n, batch_size)]
        fl_m = np.mean(bm)
        out["flux_stats"] = np.array([fl_m, np.sqrt(max(np.mean(bq) - fl_m * fl_m, 0.0))])
    return out


def _check64(got, want, mean_tol=1e-6, std_tol=1e-5):
    for key, spread_key in (("state_mean", "state_std"), ("state_diff_mean_standardized", "state_diff_std_standardized"),
                            ("forcing_mean", "forcing_std")):
        if key not in want:
            assert key not in got
            continue
        g, w = got[key].double().numpy(), want[key]
        assert got[key].dtype == torch.float32 and got[key].shape == w.shape
        err = np.abs(g - w)
        assert (err <= mean_tol * (np.abs(w) + want[spread_key]) + 1e-30).all(), (key, err.max())
        gs, ws = got[spread_key].double().numpy(), want[spread_key]
        assert (np.abs(gs - ws) <= std_tol * ws + 1e-30).all(), (spread_key, np.abs(gs - ws).max())
    if "flux_stats" in want:
        g, w = got["flux_stats"].double().numpy(), want["flux_stats"]
        assert abs(g[0] - w[0]) <= mean_tol * (abs(w[0]) + w[1]) and abs(g[1] - w[1]) <= std_tol * w[1], (g, w)


def _data(shape, seed, offsets, scale=1.0):
    """fp32 normal data with a per-feature offset (offsets[f] * scale + N(0, scale^2))."""
    rng = np.random.default_rng(seed)
    F = shape[-1]
    off = np.asarray(offsets, dtype=np.float64)[:F] if offsets is not None else np.zeros(F)
    return (rng.standard_normal(shape) * scale + off * scale).astype(np.float32)


def _dataset(state, forcing, is_forecast, ar, single=False):
    from neural_lam_amd.data import DeviceWeatherDataset

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)   # load_single_member's "only using first ensemble member"
        return DeviceWeatherDataset(state, forcing, ar_steps=ar, num_past_forcing_steps=0, num_future_forcing_steps=0,
                                    device="cuda", is_forecast=is_forecast, load_single_member=single)


OFFSETS = [0.0, 5.0, -3.0, 100.0, 0.5, 2.0, -40.0, 7.0, 1.0, 0.0, 12.0, -1.0, 3.0, 0.0, 9.0, -6.0, 250.0, 1.0, 0.0, 4.0]

# (is_forecast, state shape, forcing shape or None, ar_steps, step_length, batch_size, load_single_member)
CASES = {
    "forecast_members": (True, (3, 9, 2, 37, 5), (3, 9, 2, 37, 3), 7, 3, 32, False),
    "forecast_no_members": (True, (4, 8, 41, 4), (4, 8, 41, 2), 6, 1, 32, False),
    "forecast_shared_forcing_short_batch": (True, (5, 7, 3, 29, 6), (5, 7, 29, 4), 5, 2, 4, False),
    "forecast_single_member": (True, (3, 9, 2, 33, 5), (3, 9, 2, 33, 3), 7, 3, 2, True),
    "analysis": (False, (20, 43, 5), (20, 43, 3), 4, 3, 5, False),
    "analysis_members": (False, (15, 2, 31, 4), (15, 2, 31, 2), 3, 2, 32, False),
    "step_not_dividing": (True, (3, 9, 2, 35, 5), (3, 9, 35, 3), 7, 4, 32, False),   # 9 rows, step 4: used 8
    "d_state_17_unaligned": (True, (3, 8, 2, 33, 17), (3, 8, 33, 6), 6, 3, 3, False),
    "no_forcing": (False, (12, 27, 3), None, 4, 2, 32, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_matches_float64_restatement(case):
    from neural_lam_amd.stats import compute_standardization_stats

    fc, s_shape, f_shape, ar, step, bs, single = CASES[case]
    state = _data(s_shape, 1, OFFSETS, 1.5)
    forcing = None if f_shape is None else _data(f_shape, 2, OFFSETS[3:], 0.8)
    ds = _dataset(state, forcing, fc, ar, single)
    got = compute_standardization_stats(ds, step_length=step, batch_size=bs, flux_index=1 if forcing is not None else 0)
    want = restate64(state, forcing, is_forecast=fc, ar=ar, step=step, batch_size=bs, flux_index=1 if forcing is not None else 0,
                     single=single)
    assert set(got) == ({"state_mean", "state_std", "state_diff_mean_standardized", "state_diff_std_standardized"} |
                        (set() if forcing is None else {"forcing_mean", "forcing_std", "flux_stats"}))
    for v in got.values():
        assert v.device.type == "cpu" and v.dtype == torch.float32
    _check64(got, want)


@pytest.mark.gpu
def test_known_answers_ramp_and_constant():
    from neural_lam_amd.stats import compute_standardization_stats

    # analysis ramp x[t, n, f] = a_f * t + b_f: sample s reads t = s ... s + R - 1 (R = ar + 2), n samples
    T, N, ar, step = 24, 50, 5, 2
    R, n = ar + 2, T - (ar + 2) + 1
    a = np.array([0.5, 2.0, -1.0], np.float32)
    b = np.array([2.0, -10.0, 100.0], np.float32)
    t = np.arange(T, dtype=np.float32)
    state = np.broadcast_to((t[:, None, None] * a + b), (T, N, 3)).astype(np.float32).copy()
    forcing = np.full((T, N, 2), 3.0, np.float32)
    forcing[..., 1] = 0.1
    got = compute_standardization_stats(_dataset(state, forcing, False, ar), step_length=step, batch_size=4)
    mean = a.astype(np.float64) * ((n - 1) / 2 + (R - 1) / 2) + b
    std = np.abs(a.astype(np.float64)) * np.sqrt((n * n - 1) / 12 + (R * R - 1) / 12)   # Var(s + j), s and j uniform
    np.testing.assert_allclose(got["state_mean"].numpy(), mean, rtol=1e-6)
    np.testing.assert_allclose(got["state_std"].numpy(), std, rtol=1e-6)
    # every step-spaced difference is a * step / std: a constant, its std 0 up to the fp32 rounding of the standardisation
    dm = a.astype(np.float64) * step / got["state_std"].double().numpy()
    np.testing.assert_allclose(got["state_diff_mean_standardized"].numpy(), dm, rtol=1e-5)
    assert (got["state_diff_std_standardized"].double().numpy() <= 1e-5 * np.abs(dm)).all()
    # a constant field: std 0, not NaN (the reference's fp32 sqrt(E[x^2] - mean^2) can go negative)
    assert got["forcing_mean"][0] == 3.0 and got["forcing_std"][0] == 0.0
    assert torch.isfinite(got["forcing_std"]).all() and got["forcing_std"][1] <= 1e-6
    assert torch.equal(got["flux_stats"], torch.tensor([3.0, 0.0]))


def _reference_fp32(ds, step, batch_size, flux_index=0):
    """compute_standardization_stats.py's loop and save_stats, in its fp32 torch formulas on the CPU."""
    n = len(ds)
    means, squares, flux_means, flux_squares = [], [], [], []
    batches = []
    for b0 in range(0, n, batch_size):
        init, target, forcing, _ = ds.batch(list(range(b0, min(n, b0 + batch_size))))
        batches.append((init.cpu(), target.cpu(), forcing.cpu()))
    for init, target, forcing in batches:
        batch = torch.cat((init, target), dim=1)
        means.append(torch.mean(batch, dim=(1, 2)))
        squares.append(torch.mean(batch**2, dim=(1, 2)))
        flux = forcing[:, :, :, flux_index]
        flux_means.append(torch.mean(flux))
        flux_squares.append(torch.mean(flux**2))
    mean = torch.mean(torch.cat(means), dim=0)
    std = torch.sqrt(torch.mean(torch.cat(squares), dim=0) - mean**2)
    fl_m = torch.mean(torch.tensor(flux_means))
    fl_s = torch.sqrt(torch.mean(torch.tensor(flux_squares)) - fl_m**2)
    used = ((ds.ar_steps + 2) // step) * step
    dms, dqs = [], []
    for init, target, _ in batches:
        batch = torch.cat(((init - mean) / std, (target - mean) / std), dim=1)
        stepped = torch.cat([batch[:, k:used:step] for k in range(step)], dim=0)
        diffs = stepped[:, 1:] - stepped[:, :-1]
        dms.append(torch.mean(diffs, dim=(1, 2)))
        dqs.append(torch.mean(diffs**2, dim=(1, 2)))
    dmean = torch.mean(torch.cat(dms), dim=0)
    dstd = torch.sqrt(torch.mean(torch.cat(dqs), dim=0) - dmean**2)
    return {"state_mean": mean, "state_std": std, "state_diff_mean_standardized": dmean, "state_diff_std_standardized": dstd,
            "flux_stats": torch.stack((fl_m, fl_s))}


@pytest.mark.gpu
def test_matches_the_reference_fp32_formulas():
    """What the reference's script would write, to fp32 tolerances: its per-sample means are fp32 sums of ~10^4 values
    (relative error ~1e-6 of the magnitude), and its std comes from E[x^2] - mean^2 in fp32, whose cancellation
    multiplies that error by (mean^2 + std^2) / std^2 -- hence the std bar 2e-5 * (1 + (mean / std)^2)."""
    from neural_lam_amd.stats import compute_standardization_stats

    state = _data((4, 9, 2, 333, 5), 7, [0.0, 3.0, -2.0, 10.0, 1.0], 1.0)
    forcing = _data((4, 9, 333, 2), 8, [4.0, 0.0], 1.0)
    ds = _dataset(state, forcing, True, 7)
    got = compute_standardization_stats(ds, step_length=3, batch_size=3)
    ref = _reference_fp32(ds, 3, 3)
    for mk, sk in (("state_mean", "state_std"), ("state_diff_mean_standardized", "state_diff_std_standardized")):
        m, s = ref[mk].double(), ref[sk].double()
        assert ((got[mk].double() - m).abs() <= 2e-6 * (m.abs() + s)).all(), mk
        assert ((got[sk].double() - s).abs() <= 2e-5 * s * (1 + (m / s) ** 2)).all(), sk
    fm, fs = ref["flux_stats"].double()
    assert abs(float(got["flux_stats"][0]) - fm) <= 2e-6 * (abs(fm) + fs)
    assert abs(float(got["flux_stats"][1]) - fs) <= 2e-5 * fs * (1 + (fm / fs) ** 2)


def _stats_case():
    state = _data((7, 8, 2, 45, 17), 11, OFFSETS, 2.0)
    forcing = _data((7, 8, 45, 6), 12, OFFSETS[2:], 1.0)
    return state, forcing


@pytest.mark.gpu
def test_bit_identical_run_to_run():
    from neural_lam_amd.stats import compute_standardization_stats

    state, forcing = _stats_case()
    ds = _dataset(state, forcing, True, 6)
    a = compute_standardization_stats(ds, step_length=3, batch_size=4)
    b = compute_standardization_stats(ds, step_length=3, batch_size=4)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from neural_lam_amd.stats import compute_standardization_stats

    state, forcing = _stats_case()
    res = compute_standardization_stats(_dataset(state, forcing, True, 6), step_length=3, batch_size=4)
    torch.save(res, f"{out_dir}/rank{rank}.pt")
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_gloo_ranks_bit_identical_to_one(tmp_path):
    import torch.multiprocessing as mp

    from neural_lam_amd.stats import compute_standardization_stats

    state, forcing = _stats_case()   # 7 analysis times x 2 members = 14 samples: 7 per rank
    one = compute_standardization_stats(_dataset(state, forcing, True, 6), step_length=3, batch_size=4)
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        got = torch.load(tmp_path / f"rank{r}.pt", weights_only=True)
        assert got.keys() == one.keys()
        for k in one:
            assert torch.equal(got[k], one[k]), (r, k)


@pytest.mark.gpu
def test_end_to_end_files_datastore_model_and_standardized_batches(tmp_path):
    from neural_lam_amd import graph as G
    from neural_lam_amd import models as hm
    from neural_lam_amd.data import DeviceWeatherDataset
    from neural_lam_amd.datastore import SyntheticDatastore
    from neural_lam_amd.stats import compute_standardization_stats, load_standardization_stats, save_standardization_stats

    nx, ny, d_state, d_forcing, ar = 9, 9, 4, 3, 4
    N = nx * ny
    state = _data((5, ar + 2, 2, N, d_state), 21, [1.0, -4.0, 20.0, 0.0], 3.0)
    forcing = _data((5, ar + 2, N, d_forcing), 22, [2.0, 0.0, -1.0], 0.5)
    ds = _dataset(state, forcing, True, ar)
    stats = compute_standardization_stats(ds, step_length=2, batch_size=4)
    save_standardization_stats(tmp_path / "static", stats)
    files = load_standardization_stats(tmp_path / "static", d_forcing)
    for k in ("state_mean", "state_std", "state_diff_mean_standardized", "state_diff_std_standardized", "flux_stats"):
        assert torch.equal(files[k], stats[k]), k
    state_keys = ("state_mean", "state_std", "state_diff_mean_standardized", "state_diff_std_standardized")
    store = SyntheticDatastore(nx, ny, d_state, d_forcing, 1, root_path=tmp_path, boundary="random", seed=1,
                               state_stats={k: files[k] for k in state_keys},
                               forcing_stats={k: files[k] for k in ("forcing_mean", "forcing_std")})
    ext = store.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(store.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))
    fc = hm.ARForecaster(hm.GraphLAM(store, graph=graph, hidden_dim=16, processor_layers=1), store)
    step = hm.ForecasterStep(fc, store, standardize=True)
    got = step.standardization_stats()
    for k in ("state_mean", "state_std", "forcing_mean", "forcing_std"):
        assert torch.equal(got[k].cpu(), files[k]), k

    # the dataset standardizes with the computed statistics: every feature has mean ~0 and std ~1 over all samples
    sds = DeviceWeatherDataset(state, forcing, ar_steps=ar, num_past_forcing_steps=0, num_future_forcing_steps=0,
                               device="cuda", is_forecast=True, standardization=stats)
    init, target, _, _ = sds.batch(list(range(len(sds))), standardize=True)
    x = torch.cat((init, target), dim=1).double()
    m = x.mean(dim=(0, 1, 2))
    s = ((x * x).mean(dim=(0, 1, 2)) - m * m).sqrt()
    assert (m.abs() <= 1e-5).all(), m
    assert ((s - 1).abs() <= 1e-5).all(), s


@pytest.mark.gpu
def test_meps_size_forecast_matches_float64_on_the_device():
    """A MEPS-shaped forecast (63 784 nodes, 17 state / 6 forcing variables, 65 lead times, 2 members) against a
    float64 torch computation on the GPU, to the bars of the float64 restatement."""
    from neural_lam_amd.stats import compute_standardization_stats

    A, L_, M, N, ds_, df_, ar, step = 2, 65, 2, 63784, 17, 6, 63, 3
    g = torch.Generator(device="cuda").manual_seed(5)
    off = torch.tensor(OFFSETS[:ds_], device="cuda")
    state = torch.randn((A, L_, M, N, ds_), device="cuda", generator=g) * 2.0 + off
    forcing = torch.randn((A, L_, N, df_), device="cuda", generator=g) + off[:df_]
    ds = _dataset(state, forcing, True, ar)
    got = compute_standardization_stats(ds, step_length=step, batch_size=3)

    vm, vq, fm, fq = [], [], [], []
    for s in range(A):
        for m in range(M):
            x = state[s, :, m].double()
            vm.append(x.mean(dim=(0, 1)))
            vq.append((x * x).mean(dim=(0, 1)))
            f = forcing[s, 2:].double()
            fm.append(f.mean(dim=(0, 1)))
            fq.append((f * f).mean(dim=(0, 1)))
    vm, vq, fm, fq = map(torch.stack, (vm, vq, fm, fq))
    mean = vm.mean(0)
    std = (vq.mean(0) - mean * mean).clamp_min(0).sqrt()
    m32, s32 = mean.float(), std.float()
    used = (L_ // step) * step
    dm, dq = [], []
    for s in range(A):
        for m in range(M):
            z = (state[s, :, m] - m32) / s32
            for k in range(step):
                sub = z[k:used:step]
                d = (sub[1:] - sub[:-1]).double()
                dm.append(d.mean(dim=(0, 1)))
                dq.append((d * d).mean(dim=(0, 1)))
    dmean = torch.stack(dm).mean(0)
    dstd = (torch.stack(dq).mean(0) - dmean * dmean).clamp_min(0).sqrt()
    fmean = fm.mean(0)
    fstd = (fq.mean(0) - fmean * fmean).clamp_min(0).sqrt()
    bm = torch.stack([fm[b : b + 3, 0].mean() for b in range(0, A * M, 3)])
    bq = torch.stack([fq[b : b + 3, 0].mean() for b in range(0, A * M, 3)])
    flm = bm.mean()
    want = {"state_mean": mean, "state_std": std, "state_diff_mean_standardized": dmean, "state_diff_std_standardized": dstd,
            "forcing_mean": fmean, "forcing_std": fstd,
            "flux_stats": torch.stack((flm, (bq.mean() - flm * flm).clamp_min(0).sqrt()))}
    _check64(got, {k: v.cpu().numpy() for k, v in want.items()})
