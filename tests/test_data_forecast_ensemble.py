"""Forecast-type and ensemble datasets on the device data path (neural_lam_amd.data.DeviceWeatherDataset with
``is_forecast`` / a member axis / ``load_single_member`` -> nlam_window_batch_ens).

The reference semantics (neural_lam/weather_dataset.py) restated in numpy here, with off = max(2, past):
  * len: analysis as today (min over state and forcing of T - (off + ar + future) + 1); forecast: analysis_time.size,
    a ValueError when the lead-time axis is shorter than off + ar (state) or off + ar + future (forcing) (:135-180);
    times the number of members unless load_single_member=True (:198-200), which warns "only using first ensemble
    member" (:85-90).
  * flat index -> (sample, member) = divmod(idx, members), time-major (:399-409); forcing with a member axis follows the
    member, forcing without one is shared; a state without a member axis reads forcing member 0 (:399-418).
  * state rows: analysis times sample + max(0, past - 2) ... sample + off + ar - 1 (:255-264); forecast analysis
    `sample`, leads max(0, past - 2) ... off + ar - 1 (:235-254).
  * forcing window of target step k: analysis times sample + off + k - past ... + future (:343-374); forecast leads
    off + k - past ... off + k + future of analysis `sample` (:303-342); stacked feature-major / window-minor (:443-445).
  * target_times: analysis times[sample + off + k]; forecast analysis_time[sample] + elapsed[off + k] (:248-253, :438).
The known-answer data encode position in the value as the reference's EnsembleDummyDatastore does
(tests/dummy_datastore.py:483-769): analysis state t*100 + m, forcing 10000 + t*100 + m (with members) or 20000 + t*100;
forecast state a*1000 + e*10 + m, forcing 10000 + a*1000 + e*10 + m or 20000 + a*1000 + e*10.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

T0 = np.datetime64("2021-01-01T00:00:00", "ns").astype(np.int64)
HOUR = 3600 * 10**9


# ---- the numpy restatement ----
def _has_members(shape, is_forecast):
    return len(shape) == (5 if is_forecast else 4)


def ref_len(state_shape, forcing_shape, is_forecast, ar, past, fut, single=False):
    off = max(2, past)
    if is_forecast:
        base = state_shape[0]
    else:
        n = state_shape[0] - (off + ar + fut) + 1
        if forcing_shape is not None:
            n = min(n, forcing_shape[0] - (off + ar + fut) + 1)
        base = max(0, n)
    if _has_members(state_shape, is_forecast) and not single:
        base *= state_shape[-3]
    return base


def ref_item(state, forcing, times, elapsed, idx, is_forecast, ar, past, fut, single=False):
    n = ref_len(state.shape, None if forcing is None else forcing.shape, is_forecast, ar, past, fut, single)
    if idx < 0:
        idx += n
    if not 0 <= idx < n:
        raise IndexError(idx)
    sm = _has_members(state.shape, is_forecast)
    M = state.shape[-3] if sm and not single else 1
    s, m = divmod(idx, M)
    lead = 1 if is_forecast else 0
    st = np.take(state, m, axis=lead + 1) if sm else state
    off = max(2, past)
    if is_forecast:
        seq = st[s, max(0, past - 2) : off + ar]
        tt = np.arange(off, off + ar, dtype=np.int64) if times is None else times[s] + elapsed[off : off + ar]
    else:
        seq = st[s + max(0, past - 2) : s + off + ar]
        tt = np.arange(s + off, s + off + ar, dtype=np.int64) if times is None else times[s + off : s + off + ar]
    N = state.shape[-2]
    if forcing is None:
        frc = np.empty((ar, N, 0), np.float32)
    else:
        fo = np.take(forcing, m, axis=lead + 1) if _has_members(forcing.shape, is_forecast) else forcing
        steps = []
        for k in range(ar):
            w = fo[s, off + k - past : off + k + fut + 1] if is_forecast else fo[s + off + k - past : s + off + k + fut + 1]
            steps.append(np.transpose(w, (1, 2, 0)).reshape(N, -1))
        frc = np.stack(steps)
    return seq[:2], seq[2:], frc, np.asarray(tt, dtype=np.int64)


def dummy(is_forecast, members=3, forcing_members=True, n_times=10, n_analysis=4, n_leads=6):
    """EnsembleDummyDatastore's arrays (one node, one feature); members=None: no member axis."""
    if is_forecast:
        a = np.arange(n_analysis).reshape(-1, 1, 1, 1, 1)
        e = np.arange(n_leads).reshape(1, -1, 1, 1, 1)
        m = np.arange(members or 1).reshape(1, 1, -1, 1, 1)
        state = (a * 1000 + e * 10 + m).astype(np.float32)
        forcing = (10000 + a * 1000 + e * 10 + m).astype(np.float32) if forcing_members else \
            (20000 + a * 1000 + e * 10).astype(np.float32)[:, :, 0]
        if members is None:
            state = state[:, :, 0]
            forcing = forcing[:, :, 0] if forcing_members else forcing
        times = T0 + np.arange(n_analysis, dtype=np.int64) * HOUR
        elapsed = np.arange(n_leads, dtype=np.int64) * HOUR
        return state, forcing, times, elapsed
    t = np.arange(n_times).reshape(-1, 1, 1, 1)
    m = np.arange(members or 1).reshape(1, -1, 1, 1)
    state = (t * 100 + m).astype(np.float32)
    forcing = (10000 + t * 100 + m).astype(np.float32) if forcing_members else (20000 + t * 100).astype(np.float32)[:, 0]
    if members is None:
        state = state[:, 0]
        forcing = forcing[:, 0] if forcing_members else forcing
    return state, forcing, T0 + np.arange(n_times, dtype=np.int64) * HOUR, None


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _np(t):
    return t.cpu().numpy()


# ---- CPU: the C-ABI and the host-side layout ----
def test_abi_exports_the_strided_window_entry():
    from neural_lam_amd import _lib as L

    lib = L.load()
    assert "nlam_window_batch_ens" in L.EXPORTS and hasattr(lib, "nlam_window_batch_ens")
    # 13 pointers, 7 int64, 12 int32: include/nlam_hip.h nlam_window_ens_t
    assert C.sizeof(L.WindowEns) == 13 * 8 + 7 * 8 + 12 * 4
    assert L.WindowEns.n_times.offset == 13 * 8 + 6 * 8 and L.WindowEns.members.offset == 13 * 8 + 7 * 8 + 3 * 4


def test_abi_window_batch_ens_rejects_bad_arguments_before_launching():
    from neural_lam_amd import _lib as L

    lib = L.load()
    EINVAL = -1   # include/nlam_hip.h: NLAM_EINVAL
    assert lib.nlam_window_batch_ens(None, None) == EINVAL
    assert lib.nlam_window_batch_ens(C.byref(L.WindowEns()), None) == EINVAL      # no pointers at all
    buf = (C.c_float * 4)()
    a = C.cast(buf, C.c_void_p)

    def good():   # a forecast problem with an empty batch: valid, nothing to launch
        p = L.WindowEns()
        p.state = p.forcing = p.sample_idx = p.init_states = p.target_states = p.forcing_windowed = a
        p.state_stride_sample, p.state_stride_step, p.state_stride_member = 60, 6, 1
        p.forcing_stride_sample, p.forcing_stride_step = 60, 6
        p.n_times, p.state_steps, p.forcing_steps, p.is_forecast, p.members = 4, 5, 6, 1, 3
        p.nodes, p.d_state, p.d_forcing, p.batch = 1, 1, 1, 0
        p.ar_steps, p.num_past_forcing_steps, p.num_future_forcing_steps = 3, 1, 1
        return p

    assert lib.nlam_window_batch_ens(C.byref(good()), None) == 0
    bad = {
        "members < 1": dict(members=0),
        "state lead-time axis too short": dict(state_steps=4),
        "forcing lead-time axis too short": dict(forcing_steps=5),
        "analysis times without elapsed": dict(times=a),
        "elapsed without analysis times": dict(elapsed=a),
        "mean without std": dict(state_mean=a),
        "state statistics without forcing statistics": dict(state_mean=a, state_std=a),
        "forcing width without forcing": dict(forcing=None),
        "forcing width without output": dict(forcing_windowed=None),
        "no state": dict(state=None),
        "no indices": dict(sample_idx=None),
        "negative stride": dict(state_stride_step=-6),
        "unknown kind": dict(is_forecast=2),
        "no ar steps": dict(ar_steps=0),
        "negative past": dict(num_past_forcing_steps=-1),
        "no analysis times": dict(n_times=0),
        "elapsed with analysis data": dict(is_forecast=0, n_times=10, elapsed=a),
        "analysis series shorter than one sample": dict(is_forecast=0, n_times=5),
    }
    for what, fields in bad.items():
        p = good()
        for k, v in fields.items():
            setattr(p, k, v)
        assert lib.nlam_window_batch_ens(C.byref(p), None) == EINVAL, what
    p = good()
    p.is_forecast, p.n_times = 0, 6   # analysis: 6 time steps = exactly one sample (2 + 3 + 1)
    assert lib.nlam_window_batch_ens(C.byref(p), None) == 0


@pytest.mark.parametrize("past,future,ar_steps,reduction", [(0, 0, 1, 2), (2, 0, 1, 2), (0, 2, 1, 4), (4, 0, 1, 4), (0, 0, 5, 6), (3, 3, 2, 7)])
def test_layout_lengths_match_reference(past, future, ar_steps, reduction):
    """tests/test_datasets.py:259-296 of the reference, for plain and ensemble analysis data and forecasts."""
    from neural_lam_amd.data import plan_layout

    kw = dict(ar_steps=ar_steps, num_past_forcing_steps=past, num_future_forcing_steps=future)
    assert plan_layout((10, 1, 1), (10, 1, 1), **kw).length == 10 - reduction
    assert plan_layout((10, 3, 1, 1), (10, 1, 1), **kw).length == 3 * (10 - reduction)
    assert plan_layout((10, 3, 1, 1), (10, 3, 1, 1), **kw).length == ref_len((10, 3, 1, 1), (10, 3, 1, 1), False, ar_steps, past, future)
    leads = max(2, past) + ar_steps + future
    lay = plan_layout((4, leads + 7, 2, 5, 3), (4, leads, 5, 2), is_forecast=True, **kw)
    assert lay.length == 8 and lay.members == 2 and lay.base_len == 4
    assert lay.state_steps == max(2, past) + ar_steps and lay.forcing_steps == leads   # only what a sample reads is resident


def test_ensemble_len_scales_with_members_and_single_member_warns():
    """test_ensemble_len_scales_with_default_all_members / test_forecast_ensemble_len_scales_with_default_all_members
    (tests/test_datasets.py:324-350, :454-481 of the reference)."""
    from neural_lam_amd.data import plan_layout

    kw = dict(ar_steps=2, num_past_forcing_steps=1, num_future_forcing_steps=1)
    for is_forecast, shape, fshape in ((False, (10, 3, 1, 1), (10, 1, 1)), (True, (4, 6, 3, 1, 1), (4, 6, 3, 1, 1))):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            full = plan_layout(shape, fshape, is_forecast=is_forecast, **kw)
        with pytest.warns(UserWarning, match="only using first ensemble member"):
            single = plan_layout(shape, fshape, is_forecast=is_forecast, load_single_member=True, **kw)
        assert full.length == 3 * single.length and single.members == 1
        assert not single.keep_state_members and not single.keep_forcing_members   # member 0 only stays resident
    assert plan_layout((4, 6, 3, 1, 1), None, is_forecast=True, **kw).length == 12
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no member axis: nothing to warn about
        assert plan_layout((4, 6, 1, 1), None, is_forecast=True, load_single_member=True, **kw).length == 4


def test_layout_rejects_short_lead_axes_and_mismatched_series():
    from neural_lam_amd.data import plan_layout

    kw = dict(is_forecast=True, ar_steps=3, num_past_forcing_steps=3, num_future_forcing_steps=1)
    with pytest.raises(ValueError, match=r"forecast steps available \(5\) is less than the required 6"):
        plan_layout((4, 5, 2, 1, 1), None, **kw)
    with pytest.raises(ValueError, match=r"forcing forecast steps available \(6\) is less than the required 7"):
        plan_layout((4, 6, 2, 1, 1), (4, 6, 1, 1), **kw)
    plan_layout((4, 6, 2, 1, 1), (4, 7, 1, 1), **kw)
    with pytest.raises(ValueError, match="analysis times"):
        plan_layout((4, 6, 2, 1, 1), (5, 7, 1, 1), **kw)
    with pytest.raises(ValueError, match="ensemble members"):
        plan_layout((4, 6, 2, 1, 1), (4, 7, 3, 1, 1), **kw)
    with pytest.raises(ValueError, match="same nodes"):
        plan_layout((4, 6, 2, 3, 1), (4, 7, 2, 1, 1), **kw)
    with pytest.raises(ValueError, match="state must be"):
        plan_layout((4, 6, 1), None, **kw)
    with pytest.raises(ValueError, match="state must be"):
        plan_layout((4, 6, 1, 2, 3, 1), None, is_forecast=False)


def test_new_keywords_still_need_a_gpu():
    from neural_lam_amd.data import DeviceWeatherDataset

    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    s, f, t, e = dummy(True)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        DeviceWeatherDataset(s, f, t, elapsed=e, is_forecast=True, device="cpu")


# ---- GPU: known answers ----
@pytest.mark.gpu
@pytest.mark.parametrize("forcing_members", [True, False])
@pytest.mark.parametrize("past,fut", [(0, 0), (1, 1), (2, 0), (3, 1), (0, 1), (3, 0)])
def test_forecast_known_answers(past, fut, forcing_members):
    _gpu()
    from neural_lam_amd.data import DeviceWeatherDataset

    ar, M = 2, 3
    state, forcing, times, elapsed = dummy(True, M, forcing_members)
    ds = DeviceWeatherDataset(state, forcing, times, ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                              is_forecast=True, elapsed=elapsed)
    assert len(ds) == 4 * M and ds.kernel == "nlam_window_batch_ens"
    off = max(2, past)
    for idx in range(len(ds)):
        a, m = divmod(idx, M)
        init, target, frc, tt = (_np(x) for x in ds[idx])
        e0 = max(0, past - 2)
        assert init[:, 0, 0].tolist() == [a * 1000 + e * 10 + m for e in (e0, e0 + 1)]
        assert target[:, 0, 0].tolist() == [a * 1000 + e * 10 + m for e in range(off, off + ar)]
        exp = [[(10000 + a * 1000 + e * 10 + m) if forcing_members else (20000 + a * 1000 + e * 10)
                for e in range(off + k - past, off + k + fut + 1)] for k in range(ar)]
        assert frc[:, 0, :].tolist() == exp
        assert tt.tolist() == [T0 + (a + e) * HOUR for e in range(off, off + ar)]


@pytest.mark.gpu
@pytest.mark.parametrize("forcing_members", [True, False])
@pytest.mark.parametrize("past,fut", [(0, 0), (1, 1), (2, 0), (3, 1), (0, 1), (3, 0)])
def test_analysis_ensemble_known_answers(past, fut, forcing_members):
    _gpu()
    from neural_lam_amd.data import DeviceWeatherDataset

    ar, M, T = 2, 3, 10
    state, forcing, times, _ = dummy(False, M, forcing_members, n_times=T)
    ds = DeviceWeatherDataset(state, forcing, times, ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut)
    off = max(2, past)
    n = T - (off + ar + fut) + 1
    assert len(ds) == n * M and ds.kernel == "nlam_window_batch_ens"
    for idx in range(len(ds)):
        t, m = divmod(idx, M)
        init, target, frc, tt = (_np(x) for x in ds[idx])
        t0 = t + max(0, past - 2)
        assert init[:, 0, 0].tolist() == [(t0 + r) * 100 + m for r in range(2)]
        assert target[:, 0, 0].tolist() == [(t + off + k) * 100 + m for k in range(ar)]
        exp = [[(10000 + u * 100 + m) if forcing_members else (20000 + u * 100)
                for u in range(t + off + k - past, t + off + k + fut + 1)] for k in range(ar)]
        assert frc[:, 0, :].tolist() == exp
        assert tt.tolist() == [T0 + (t + off + k) * HOUR for k in range(ar)]


@pytest.mark.gpu
@pytest.mark.parametrize("is_forecast", [False, True])
def test_reference_ensemble_properties(is_forecast):
    """tests/test_datasets.py:383-452 of the reference: time-major member mapping, forcing follows the member when it has
    the axis and is shared when it has not; a state without a member axis reads forcing member 0."""
    _gpu()
    from neural_lam_amd.data import DeviceWeatherDataset

    kw = dict(ar_steps=2, num_past_forcing_steps=1, num_future_forcing_steps=1, is_forecast=is_forecast)
    s, f, t, e = dummy(is_forecast, 3, False)
    if is_forecast:
        kw["elapsed"] = e
    ds = DeviceWeatherDataset(s, f, t, **kw)
    i0, _, f0, t0 = ds[0]
    i1, _, f1, t1 = ds[1]
    assert torch.equal(t0, t1) and not torch.equal(i0, i1) and torch.equal(f0, f1)   # shared forcing
    s, f, t, e = dummy(is_forecast, 3, True)
    ds = DeviceWeatherDataset(s, f, t, **kw)
    i0, _, f0, t0 = ds[0]
    i1, _, f1, t1 = ds[1]
    i3, _, _, t3 = ds[3]
    assert torch.equal(t0, t1) and not torch.equal(f0, f1) and not torch.equal(t0, t3)   # member follows; index 3 = next sample
    assert torch.equal(f1 - f0, torch.ones_like(f0)) and torch.equal(i1 - i0, torch.ones_like(i0))
    # state without a member axis, forcing with one: member 0 of the forcing (and only member 0 is kept resident)
    s0 = s[:, :, 0] if is_forecast else s[:, 0]
    ds = DeviceWeatherDataset(s0, f, t, **kw)
    assert len(ds) == ref_len(s0.shape, f.shape, is_forecast, 2, 1, 1) and ds.forcing.dim() == (4 if is_forecast else 3)
    for idx in range(len(ds)):
        ref = ref_item(s0, f, t, e, idx, is_forecast, 2, 1, 1)
        assert all(np.array_equal(_np(g), r) for g, r in zip(ds[idx], ref))
    # load_single_member: member 0 only, the length of one member
    with pytest.warns(UserWarning, match="only using first ensemble member"):
        ds1 = DeviceWeatherDataset(s, f, t, load_single_member=True, **kw)
    assert len(ds1) * 3 == len(DeviceWeatherDataset(s, f, t, **kw))
    for idx in range(len(ds1)):
        ref = ref_item(s, f, t, e, idx, is_forecast, 2, 1, 1, single=True)
        assert all(np.array_equal(_np(g), r) for g, r in zip(ds1[idx], ref))


# ---- GPU: random shapes against the restatement ----
def _random(is_forecast, n0, leads, M, N, ds, df, fm, seed):
    rng = np.random.default_rng(seed)
    lead = (leads,) if is_forecast else ()
    mem = (M,) if M else ()
    state = rng.normal(size=(n0,) + lead + mem + (N, ds)).astype(np.float32)
    forcing = rng.normal(size=(n0,) + lead + (mem if fm else ()) + (N, df)).astype(np.float32) if df else None
    times = T0 + np.arange(n0, dtype=np.int64) * 6 * HOUR
    elapsed = np.arange(leads, dtype=np.int64) * HOUR if is_forecast else None
    return state, forcing, times, elapsed


CASES = [  # is_forecast, n0, leads, members, N, d_state, d_forcing, forcing has members, ar, past, future
    (True, 5, 12, 2, 37, 5, 2, True, 3, 1, 1),
    (True, 3, 9, 3, 130, 17, 5, False, 2, 3, 1),
    (True, 4, 7, 0, 65, 3, 0, False, 4, 0, 0),
    (True, 2, 10, 2, 2049, 7, 3, True, 1, 4, 2),
    (False, 12, 0, 2, 37, 5, 2, True, 3, 1, 1),
    (False, 15, 0, 3, 301, 6, 4, False, 2, 2, 1),
    (False, 11, 0, 2, 5, 2, 3, True, 1, 4, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_every_sample_matches_the_restatement(case):
    """Every sample, raw: bit-exact (a gather).  N not a multiple of 4 and odd widths run the scalar tails."""
    _gpu()
    from neural_lam_amd.data import DeviceWeatherDataset

    fc, n0, leads, M, N, dst, df, fm, ar, past, fut = case
    state, forcing, times, elapsed = _random(fc, n0, leads, M, N, dst, df, fm, seed=n0 + N)
    ds = DeviceWeatherDataset(state, forcing, times, ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                              is_forecast=fc, elapsed=elapsed)
    n = ref_len(state.shape, None if forcing is None else forcing.shape, fc, ar, past, fut)
    assert len(ds) == n and n > 0
    got = ds.batch(list(range(n)))
    for i in range(n):
        ref = ref_item(state, forcing, times, elapsed, i, fc, ar, past, fut)
        for g, r in zip(got, ref):
            assert np.array_equal(_np(g[i]), r), (i,)
    for i in (-1, -n):
        ref = ref_item(state, forcing, times, elapsed, i, fc, ar, past, fut)
        assert all(np.array_equal(_np(g), r) for g, r in zip(ds[i], ref))
    assert ds[-1][2].shape == (ar, N, df * (past + fut + 1))
    with pytest.raises(IndexError):
        ds[n]
    with pytest.raises(IndexError):
        ds[-n - 1]
    with pytest.raises(IndexError):
        ds.batch([0, n])
    with pytest.raises(IndexError):
        ds.check_indices(torch.tensor([0, n], device="cuda"))
    # an unvalidated device index out of range is clamped to the first / last sample instead of faulting
    clamped = ds.batch(torch.tensor([-3, n + 5], device="cuda"))
    assert all(torch.equal(a, b) for a, b in zip(clamped, ds.batch([0, n - 1])))
    # without time stamps: time indices (analysis) or lead-time indices (forecast)
    bare = DeviceWeatherDataset(state, forcing, None, ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                                is_forecast=fc)
    tt = _np(bare.batch(list(range(n)))[3])
    for i in range(n):
        assert np.array_equal(tt[i], ref_item(state, forcing, None, None, i, fc, ar, past, fut)[3])


@pytest.mark.gpu
@pytest.mark.parametrize("is_forecast", [False, True])
def test_fused_standardization_and_out_buffers(is_forecast):
    """batch(standardize=True) == on_after_batch_transfer on the raw sample: bit-equal to numpy fp32."""
    _gpu()
    from neural_lam_amd.data import DeviceWeatherDataset

    dst, df, ar, past, fut = 6, 4, 3, 2, 1
    state, forcing, times, elapsed = _random(is_forecast, 6 if is_forecast else 16, 9, 2, 301, dst, df, True, seed=3)
    rng = np.random.default_rng(4)
    stats = {"state_mean": rng.normal(size=dst).astype(np.float32), "state_std": (0.3 + rng.random(dst)).astype(np.float32),
             "forcing_mean": rng.normal(size=df).astype(np.float32), "forcing_std": (0.3 + rng.random(df)).astype(np.float32)}
    ds = DeviceWeatherDataset(state, forcing, times, ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                              standardization=stats, is_forecast=is_forecast, elapsed=elapsed)
    perm = ds.epoch_permutation(seed=1)
    assert sorted(perm.cpu().tolist()) == list(range(len(ds)))
    idx = perm[:5]
    init, target, frc, tt = ds.batch(idx, standardize=True)
    W = past + fut + 1
    for k, i in enumerate(idx.cpu().tolist()):
        raw = ref_item(state, forcing, times, elapsed, i, is_forecast, ar, past, fut)
        assert np.array_equal(_np(init[k]), (raw[0] - stats["state_mean"]) / stats["state_std"])
        assert np.array_equal(_np(target[k]), (raw[1] - stats["state_mean"]) / stats["state_std"])
        assert np.array_equal(_np(frc[k]), (raw[2] - np.repeat(stats["forcing_mean"], W)) / np.repeat(stats["forcing_std"], W))
        assert np.array_equal(_np(tt[k]), raw[3])
    out = tuple(torch.zeros_like(t) for t in (init, target, frc, tt))
    ds.batch(idx, standardize=True, out=out)
    assert all(torch.equal(a, b) for a, b in zip(out, (init, target, frc, tt)))
    with pytest.raises(ValueError):
        ds.batch(idx, out=(init[:, :1], target, frc, tt))


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,dst,df,ar,past,fut", [(12, 37, 5, 2, 3, 1, 1), (20, 130, 17, 5, 4, 2, 1), (15, 64, 3, 0, 2, 1, 1),
                                                    (11, 5, 2, 3, 1, 4, 2), (24, 63784, 17, 6, 1, 1, 1)])
def test_strided_kernel_equals_the_analysis_kernel(T, N, dst, df, ar, past, fut):
    """One member of analysis data: nlam_window_batch_ens is bit-identical to nlam_window_batch, raw and standardised,
    with and without time stamps, on the same series and (clamped) device indices."""
    _gpu()
    from neural_lam_amd.data import DeviceWeatherDataset

    state, forcing, times, _ = _random(False, T, 0, 0, N, dst, df, False, seed=T + N)
    rng = np.random.default_rng(7)
    stats = {"state_mean": rng.normal(size=dst).astype(np.float32), "state_std": (0.3 + rng.random(dst)).astype(np.float32),
             "forcing_mean": rng.normal(size=max(df, 1)).astype(np.float32), "forcing_std": (0.3 + rng.random(max(df, 1))).astype(np.float32)}
    for tms in (times, None):
        ds = DeviceWeatherDataset(state, forcing, tms, ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                                  standardization=stats)
        assert ds.kernel == "nlam_window_batch"
        idx = torch.arange(len(ds) - 1, -1, -1, device="cuda")
        for stdz in (False, True):
            a = [t.clone() for t in ds.batch(idx, standardize=stdz)]
            ds.kernel = "nlam_window_batch_ens"
            b = ds.batch(idx, standardize=stdz)
            ds.kernel = "nlam_window_batch"
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (stdz, tms is None)


@pytest.mark.gpu
def test_residency_and_chunked_uploads(tmp_path, monkeypatch):
    """Only off + ar (state) / + future (forcing) lead times stay on the device; host, memmap (chunked) and device sources
    give the same series and the same samples."""
    _gpu()
    from neural_lam_amd import data as D

    A, L, M, N, dst, df, ar, past, fut = 5, 65, 2, 67, 3, 2, 3, 1, 1
    state, forcing, times, elapsed = _random(True, A, L, M, N, dst, df, False, seed=11)
    kw = dict(ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut, is_forecast=True, elapsed=elapsed)
    ref = D.DeviceWeatherDataset(state, forcing, times, **kw)
    off = max(2, past)
    assert tuple(ref.state.shape) == (A, off + ar, M, N, dst) and tuple(ref.forcing.shape) == (A, off + ar + fut, N, df)
    assert tuple(ref.elapsed.shape) == (off + ar,)
    assert torch.equal(ref.state.cpu(), torch.from_numpy(state[:, : off + ar].copy()))
    p = tmp_path / "state.npy"
    np.save(p, state)
    mm = np.load(p, mmap_mode="r")
    monkeypatch.setattr(D, "UPLOAD_CHUNK_BYTES", 4 * (off + ar) * M * N * dst * 2 + 12)   # two analysis times per chunk
    chunked = D.DeviceWeatherDataset(mm, torch.from_numpy(forcing), times, **kw)
    on_dev = D.DeviceWeatherDataset(torch.from_numpy(state).cuda(), torch.from_numpy(forcing).cuda(), times, **kw)
    for ds in (chunked, on_dev):
        assert torch.equal(ds.state, ref.state) and torch.equal(ds.forcing, ref.forcing)
    idx = list(range(len(ref)))
    want = ref.batch(idx)
    for ds in (chunked, on_dev):
        assert all(torch.equal(a, b) for a, b in zip(ds.batch(idx), want))
    # datetime64 / timedelta64 stamps are the same nanoseconds
    dt = D.DeviceWeatherDataset(state, forcing, times.astype("datetime64[ns]"), **dict(kw, elapsed=elapsed.astype("timedelta64[ns]")))
    assert torch.equal(dt.batch(idx)[3], want[3])
    # load_single_member keeps member 0 only
    with pytest.warns(UserWarning, match="only using first ensemble member"):
        one = D.DeviceWeatherDataset(mm, forcing, times, load_single_member=True, **kw)
    assert tuple(one.state.shape) == (A, off + ar, N, dst) and len(one) == A
    assert torch.equal(one.state, ref.state[:, :, 0])


@pytest.mark.gpu
def test_full_size_forecast_ensemble_properties():
    """MEPS size (63 784 nodes, 17 + 5 variables, 2 members, 10 lead times): shift / overlap properties and determinism."""
    _gpu()
    from neural_lam_amd.data import DeviceWeatherDataset

    A, L, M, N, dst, df, ar, past, fut = 3, 10, 2, 63784, 17, 5, 4, 1, 1
    g = torch.Generator(device="cuda").manual_seed(0)
    state = torch.randn(A, L, M, N, dst, device="cuda", generator=g)
    forcing = torch.randn(A, L, M, N, df, device="cuda", generator=g)
    ds = DeviceWeatherDataset(state, forcing, None, ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                              is_forecast=True)
    assert len(ds) == A * M
    idx = torch.arange(len(ds), device="cuda")
    init, target, frc, tt = ds.batch(idx)
    again = ds.batch(idx)
    assert all(torch.equal(a, b) for a, b in zip((init, target, frc, tt), again))
    off, W = max(2, past), past + fut + 1
    a_of, m_of = idx // M, idx % M
    assert torch.equal(init[:, 0], state[a_of, 0, m_of]) and torch.equal(init[:, 1], state[a_of, 1, m_of])
    for t in range(ar):
        assert torch.equal(target[:, t], state[a_of, off + t, m_of])
        assert torch.equal(tt[:, t], torch.full_like(tt[:, t], off + t))   # lead-time index without stamps
        fr = frc[:, t].reshape(len(ds), N, df, W)
        for w in range(W):
            assert torch.equal(fr[..., w], forcing[a_of, off + t - past + w, m_of])
    # the two members of one analysis time differ exactly by their member's series
    assert torch.equal(target[1::2], state[:, off : off + ar, 1]) and torch.equal(target[0::2], state[:, off : off + ar, 0])
    fr = frc.reshape(len(ds), ar, N, df, W)
    assert torch.equal(fr[:, 1:, ..., 0], fr[:, :-1, ..., 1])   # window slot w + 1 of step k is slot w of step k + 1


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_training_from_a_forecast_ensemble_dataset(tmp_path, use_graph):
    """Trainer.step_from on a forecast-ensemble dataset (eager and captured) == Trainer.step on the batches batch() hands
    over: identical losses and parameters, step after step."""
    _gpu()
    from neural_lam_amd import graph as G
    from neural_lam_amd import models as hm
    from neural_lam_amd.data import DeviceWeatherDataset
    from neural_lam_amd.datastore import SyntheticDatastore
    from neural_lam_amd.trainer import Trainer

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    dstore = SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1,
                                state_stats={"state_mean": rng.normal(size=5) * 2, "state_std": rng.uniform(0.5, 3.0, size=5)})
    dstore._forcing_stats.forcing_mean.values = rng.normal(size=2).astype(np.float32)
    dstore._forcing_stats.forcing_std.values = rng.uniform(0.5, 2.0, size=2).astype(np.float32)
    ext = dstore.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(dstore.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))

    def make(std_in_module):
        torch.manual_seed(3)
        fc = hm.ARForecaster(hm.GraphLAM(dstore, graph=graph, hidden_dim=16, processor_layers=2), dstore)
        return Trainer(hm.ForecasterStep(fc, dstore, standardize=std_in_module).to(dev), lr=1e-3, use_graph=use_graph)

    t_ref, t_dev = make(True), make(False)
    N, T, past, fut = dstore.num_grid_points, 2, 1, 1
    state, forcing, times, elapsed = _random(True, 4, 8, 2, N, 5, 2, True, seed=9)
    data = DeviceWeatherDataset(state, forcing, times, ar_steps=T, num_past_forcing_steps=past, num_future_forcing_steps=fut,
                                standardization=t_dev.module.standardization_stats(), is_forecast=True, elapsed=elapsed)
    assert len(data) == 8
    perm = data.epoch_permutation(seed=2)
    B = 2
    for k in range(3):
        idx = perm[k * B : (k + 1) * B]
        raw = data.batch(idx)
        l_ref = float(t_ref.step(raw[0], raw[1], raw[2]))
        l_dev = float(t_dev.step_from(data, idx))
        assert l_ref == l_dev, (k, l_ref, l_dev)
        assert torch.equal(t_ref.fp.flat, t_dev.fp.flat)
        assert torch.equal(t_dev.batch_times, raw[3])
    assert (t_dev._graph is not None) == use_graph
