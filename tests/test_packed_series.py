"""Resident series as packed int16 (DeviceWeatherDataset(storage="int16"), data.PackedSeries; nlam_series_range,
nlam_series_pack_q16, nlam_window_batch_q16, nlam_window_moments_q16, nlam_forecast_init_q16 / _head_q16).

Without a GPU: the numpy restatement of the format (tests/packed_ref.py) against its own properties, the validation of
PackedSeries, the ctypes struct against the header, the exports and the argument checks of the new entries.  On the GPU every
parity check is torch.equal: a packed dataset against an fp32 dataset built from its decoded series (ds.decoded(), which is
itself pinned to the numpy decode), with no tolerance anywhere.

Launch geometry: the _q16 kernels keep the fp32 kernels' (256 threads, four elements per thread, at most two sweeps' worth of
workgroups per row).  The first shape's 137 x 9 = 1233-element block is odd, no multiple of 4, and longer than the 1024
elements one workgroup covers per sweep."""
import ctypes as C
import subprocess
import types

import numpy as np
import pytest
import torch

import packed_ref as R
from conftest import ROOT
from neural_lam_amd import _lib as L

NEW_EXPORTS = ["nlam_series_range_workspace_words", "nlam_series_range", "nlam_series_pack_q16", "nlam_window_batch_q16",
               "nlam_window_moments_q16", "nlam_forecast_init_q16", "nlam_forecast_head_q16"]
SHAPES = [(137, 9, 3), (64, 8, 4), (5, 1, 0)]   # (nodes, d_state, d_forcing)
WINDOWS = [(1, 1), (0, 0), (3, 0)]              # (past, future); past = 3 moves the first state row
LAYOUTS = ["plain", "analysis_members", "forecast", "forecast_members"]
T_ANALYSIS, N_ANALYSES, N_LEADS, MEMBERS = 14, 4, 12, 2


# ---------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------
def _awkward(rng, n=4001):
    """(n, 6): random features of different magnitudes, surface pressure (around 101 325, range 8 000), a feature in
    [0, 1e-3], all zeros."""
    x = np.empty((n, 6), dtype=np.float32)
    x[:, 0] = rng.normal(size=n) * 3 + 1
    x[:, 1] = rng.normal(size=n) * 1e4 - 5e4
    x[:, 2] = rng.uniform(-1, 1, size=n) * 1e-6
    x[:, 3] = 101325 + rng.uniform(-4000, 4000, size=n)
    x[:, 4] = rng.uniform(0, 1e-3, size=n)
    x[:, 5] = 0
    return x


def test_restatement_round_trip_extrema_and_constant_features():
    rng = np.random.default_rng(0)
    x = _awkward(rng)
    scale, offset = R.default_tables(x)
    assert scale.dtype == offset.dtype == np.float32 and (scale > 0).all()
    q = R.encode(x, scale, offset)
    assert q.dtype == np.int16 and q.min() >= -32767 and q.max() <= 32767
    back = R.decode(q, scale, offset)
    err = np.abs(back.astype(np.float64) - x.astype(np.float64))
    assert (err <= R.roundtrip_bound(x, scale, offset)).all(), float((err / R.roundtrip_bound(x, scale, offset)).max())
    for f in range(5):   # the extrema land on the last or the last but one level
        assert q[np.argmax(x[:, f]), f] in (32767, 32766), f
        assert q[np.argmin(x[:, f]), f] in (-32767, -32766), f
    # a constant feature: scale 1, its value as the offset, exact both ways
    assert scale[5] == 1 and offset[5] == 0 and (q[:, 5] == 0).all() and (back[:, 5] == 0).all()
    c = np.full((7, 1), 273.15, dtype=np.float32)
    sc, of = R.default_tables(c)
    assert sc[0] == 1 and of[0] == c[0, 0] and np.array_equal(R.decode(R.encode(c, sc, of), sc, of), c)
    # the resolution: (max - min) / 65534
    assert abs(float(scale[3]) - (float(x[:, 3].max()) - float(x[:, 3].min())) / 65534) <= 2.0 ** -23 * float(scale[3])


def test_restatement_rounds_half_to_even_and_clamps():
    scale, offset = np.array([0.5], np.float32), np.array([10.0], np.float32)
    x = np.array([[10.25], [10.75], [11.25], [9.75], [1e9], [-1e9], [10.0 + 0.5 * 32767], [10.0 - 0.5 * 32768]], np.float32)
    assert R.encode(x, scale, offset)[:, 0].tolist() == [0, 2, 2, 0, 32767, -32767, 32767, -32767]
    assert R.decode(np.array([[-32768]], np.int16), scale, offset)[0, 0] == np.float32(10.0 - 16384.0)   # no special meaning


def test_the_library_default_tables_are_the_restatement():
    from neural_lam_amd.data import default_tables

    x = _awkward(np.random.default_rng(1))
    scale, offset = default_tables(x.min(axis=0), x.max(axis=0))
    want = R.default_tables(x)
    assert np.array_equal(scale, want[0]) and np.array_equal(offset, want[1])


# ---------------------------------------------------------------------------
# CPU: validation, layout, ABI
# ---------------------------------------------------------------------------
def test_packed_series_validation_and_layout():
    from neural_lam_amd.data import PackedSeries, plan_layout

    q = np.zeros((6, 5, 3), np.int16)
    ok = PackedSeries(q, [1.0, 2.0, 3.0], np.zeros(3))
    assert ok.shape == (6, 5, 3) and ok.scale.dtype == np.float32 and ok.offset.dtype == np.float32
    PackedSeries(torch.zeros((6, 5, 3), dtype=torch.int16), torch.ones(3), torch.zeros(3))
    with pytest.raises(TypeError, match="int16"):
        PackedSeries(q.astype(np.int32), np.ones(3), np.zeros(3))
    with pytest.raises(TypeError, match="int16"):
        PackedSeries(q.astype(np.float32), np.ones(3), np.zeros(3))
    for scale, offset in ((np.ones(2), np.zeros(3)), (np.ones(3), np.zeros(4)), ([1.0, 0.0, 1.0], np.zeros(3)),
                          ([1.0, -1.0, 1.0], np.zeros(3)), ([1.0, np.nan, 1.0], np.zeros(3)), ([1.0, np.inf, 1.0], np.zeros(3)),
                          (np.ones(3), [0.0, np.nan, 0.0])):
        with pytest.raises(ValueError):
            PackedSeries(q, scale, offset)
    # the resident layout does not depend on the storage: packed and fp32 inputs of one shape plan alike
    for is_forecast, st, fo in ((False, (14, 2, 137, 9), (14, 137, 3)), (True, (4, 12, 2, 137, 9), (4, 12, 2, 137, 3))):
        packed = PackedSeries(np.zeros(st, np.int16), np.ones(st[-1]), np.zeros(st[-1]))
        kw = dict(is_forecast=is_forecast, ar_steps=3, num_past_forcing_steps=3, num_future_forcing_steps=1)
        assert plan_layout(packed.shape, fo, **kw) == plan_layout(np.zeros(st, np.float32).shape, fo, **kw)


def test_q16_symbols_are_exported_and_the_struct_matches_c_layout(tmp_path):
    header = (ROOT / "include" / "nlam_hip.h").read_text()
    lib = L.load()
    for name in NEW_EXPORTS:
        assert f"{name}(" in header and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_abi_version() == L.ABI_VERSION == 8
    fields = [name for name, _ in L.Q16Src._fields_]
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
        'int main(){printf("%zu", sizeof(nlam_q16_src_t));\n'
        + "".join(f'printf(" %zu", offsetof(nlam_q16_src_t, {f}));\n' for f in fields)
        + 'printf(" %d %zu %zu %zu\\n", NLAM_ABI_VERSION, sizeof(nlam_window_ens_t), sizeof(nlam_moments_t), sizeof(nlam_forecast_src_t));'
        " return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.Q16Src)] + [getattr(L.Q16Src, f).offset for f in fields] + [
        8, C.sizeof(L.WindowEns), C.sizeof(L.Moments), C.sizeof(L.ForecastSrc)]


def test_q16_entries_reject_bad_arguments_before_any_launch():
    """A missing decode table, a series that is in neither place, negative strides and the fp32 entries' size checks: NLAM_EINVAL
    with a null stream and pointers that are never dereferenced."""
    lib = L.load()
    fake = 1 << 20
    N, F, DF = 37, 5, 2

    def q16(**kw):
        q = L.Q16Src()
        for name in ("state", "forcing", "state_scale", "state_offset", "forcing_scale", "forcing_offset"):
            setattr(q, name, fake)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def window(**kw):
        p = L.WindowEns()
        p.sample_idx = p.init_states = p.target_states = p.forcing_windowed = fake
        p.state_stride_sample = p.state_stride_step = N * F
        p.forcing_stride_sample = p.forcing_stride_step = N * DF
        p.n_times, p.members, p.nodes, p.d_state, p.d_forcing, p.batch = 16, 1, N, F, DF, 2
        p.ar_steps, p.num_past_forcing_steps, p.num_future_forcing_steps = 3, 1, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    tables = [dict(state_scale=None), dict(state_offset=None), dict(forcing_scale=None), dict(forcing_offset=None)]
    nowhere = [dict(state=None), dict(forcing=None)]   # not packed, and no float pointer in the parameter struct either
    for kw in tables + nowhere:
        assert lib.nlam_window_batch_q16(C.byref(window()), C.byref(q16(**kw)), None) == -1, kw
    assert lib.nlam_window_batch_q16(C.byref(window()), None, None) == -1
    assert lib.nlam_window_batch_q16(None, C.byref(q16()), None) == -1
    for name in ("state_stride_sample", "state_stride_step", "state_stride_member", "forcing_stride_sample", "forcing_stride_step",
                 "forcing_stride_member"):
        assert lib.nlam_window_batch_q16(C.byref(window(**{name: -1})), C.byref(q16()), None) == -1, name
    for kw in (dict(d_state=0), dict(ar_steps=0), dict(members=0), dict(n_times=0), dict(n_times=5), dict(is_forecast=2),
               dict(init_states=None), dict(sample_idx=None), dict(forcing_windowed=None),
               dict(is_forecast=1, state_steps=4, forcing_steps=16), dict(is_forecast=1, state_steps=16, forcing_steps=5)):
        assert lib.nlam_window_batch_q16(C.byref(window(**kw)), C.byref(q16()), None) == -1, kw
    assert lib.nlam_window_batch_q16(C.byref(window(batch=65536)), C.byref(q16()), None) == -2
    assert lib.nlam_window_batch_q16(C.byref(window(nodes=(1 << 31) // F + 1)), C.byref(q16()), None) == -2

    def moments(**kw):
        p = L.Moments()
        p.workspace = p.out_mean = p.out_sq = fake
        p.workspace_doubles = 1 << 40
        p.stride_sample = p.stride_step = N * F
        p.n_times, p.count, p.members, p.nodes, p.nvars, p.nrows = 16, 2, 1, N, F, 5
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    for series, scale, offset in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.nlam_window_moments_q16(C.byref(moments()), series, scale, offset, None) == -1
    for kw in (dict(stride_sample=-1), dict(stride_step=-1), dict(stride_member=-1), dict(nvars=0), dict(count=0), dict(step=1),
               dict(is_forecast=1, steps=4), dict(workspace_doubles=1)):
        assert lib.nlam_window_moments_q16(C.byref(moments(**kw)), fake, fake, fake, None) == -1, kw
    assert lib.nlam_window_moments_q16(C.byref(moments(nvars=L.MOMENTS_MAX_VARS + 1)), fake, fake, fake, None) == -2

    def forecast(**kw):
        p = L.Forecast()
        for name in ("lead", "state_mean", "state_std", "forcing_mean", "forcing_std", "prev", "prev_prev", "forcing_windowed", "truth"):
            setattr(p, name, fake)
        p.nodes, p.d_state, p.d_forcing, p.batch = N, F, DF, 3
        p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps, p.delta_ld = 4, 3, 1, F
        s = L.ForecastSrc()
        s.sample_idx = fake
        s.state_stride_sample, s.state_stride_step, s.state_stride_member = 7 * 3 * N * F, 3 * N * F, N * F
        s.forcing_stride_sample, s.forcing_stride_step = 8 * N * DF, N * DF
        s.n_times, s.state_steps, s.forcing_steps, s.is_forecast, s.members = 4, 7, 8, 1, 3
        for k, v in kw.items():
            setattr(s, k[4:], v) if k.startswith("src_") else setattr(p, k, v)
        return C.byref(p), C.byref(s)

    for fn in (lib.nlam_forecast_init_q16, lib.nlam_forecast_head_q16):
        for kw in tables + nowhere:
            assert fn(*forecast(), C.byref(q16(**kw)), None) == -1, kw
        assert fn(*forecast(), None, None) == -1
        for series in ("state", "forcing"):
            for axis in ("sample", "step", "member"):
                assert fn(*forecast(**{f"src_{series}_stride_{axis}": -1}), C.byref(q16()), None) == -1, (series, axis)
        for kw in (dict(lead=None), dict(state_mean=None), dict(src_sample_idx=None), dict(src_state_steps=6), dict(src_forcing_steps=7),
                   dict(src_members=0), dict(max_lead=0)):
            assert fn(*forecast(**kw), C.byref(q16()), None) == -1, kw
        assert fn(*forecast(batch=65536), C.byref(q16()), None) == -2

    for args in ((None, 4, F, fake, fake, fake, fake, 1 << 30), (fake, 0, F, fake, fake, fake, fake, 1 << 30),
                 (fake, 4, F, None, fake, fake, fake, 1 << 30), (fake, 4, F, fake, fake, None, fake, 1 << 30),
                 (fake, 4, F, fake, fake, fake, None, 1 << 30), (fake, 4, F, fake, fake, fake, fake, 1)):
        assert lib.nlam_series_range(*args, None) == -1, args
    assert lib.nlam_series_range(fake, 4, L.MOMENTS_MAX_VARS + 1, fake, fake, fake, fake, 1 << 30, None) == -2
    assert lib.nlam_series_range_workspace_words(0, F) == -1 and lib.nlam_series_range_workspace_words(4, 0) == -1
    for args in ((None, 4, F, fake, fake, fake, 0), (fake, 4, F, None, fake, fake, 0), (fake, 4, F, fake, None, fake, 0),
                 (fake, 4, F, fake, fake, None, 0), (fake, 0, F, fake, fake, fake, 0), (fake, 4, F, fake, fake, fake, -1)):
        assert lib.nlam_series_pack_q16(*args, None) == -1, args
    assert lib.nlam_series_pack_q16(fake, 1 << 31, 1, fake, fake, fake, 0, None) == -2


def test_storage_argument_is_checked_before_the_device():
    from neural_lam_amd.data import DeviceWeatherDataset

    with pytest.raises(ValueError, match="storage"):
        DeviceWeatherDataset(np.zeros((8, 3, 2), np.float32), storage="bfloat16", device="cuda")


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _field(rng, shape):
    """A float32 series whose features differ in magnitude and offset (feature f: offset 100 f - 150, spread 3^(f % 5 - 2))."""
    F = shape[-1]
    f = np.arange(F)
    x = rng.normal(size=shape) * (3.0 ** (f % 5 - 2)) + (100.0 * f - 150.0)
    return x.astype(np.float32)


def _series(layout, shape, seed=0):
    """(state, forcing or None, times, elapsed or None, is_forecast) as numpy arrays for one of LAYOUTS."""
    N, ds, df = shape
    rng = np.random.default_rng(seed)
    lead = {"plain": (T_ANALYSIS,), "analysis_members": (T_ANALYSIS, MEMBERS), "forecast": (N_ANALYSES, N_LEADS),
            "forecast_members": (N_ANALYSES, N_LEADS, MEMBERS)}[layout]
    state = _field(rng, lead + (N, ds))
    forcing = _field(rng, lead + (N, df)) if df else None
    fc = layout.startswith("forecast")
    times = np.arange(lead[0], dtype=np.int64) * 3600 + 10 ** 9
    elapsed = np.arange(N_LEADS, dtype=np.int64) * 600 if fc else None
    return state, forcing, times, elapsed, fc


def _stats(shape, seed=3):
    rng = np.random.default_rng(seed)
    _, ds, df = shape
    out = {"state_mean": rng.normal(size=ds).astype(np.float32) * 50, "state_std": rng.uniform(0.5, 9.0, size=ds).astype(np.float32)}
    if df:
        out.update(forcing_mean=rng.normal(size=df).astype(np.float32) * 50, forcing_std=rng.uniform(0.5, 9.0, size=df).astype(np.float32))
    return out


def _pair(dev, layout, shape, ar, past, fut, seed=0, pack=("state", "forcing"), stats=True):
    """(packed dataset, fp32 dataset built from its decoded series)."""
    from neural_lam_amd.data import DeviceWeatherDataset, PackedSeries

    state, forcing, times, elapsed, fc = _series(layout, shape, seed)
    kw = dict(ar_steps=ar, num_past_forcing_steps=past, num_future_forcing_steps=fut, is_forecast=fc,
              standardization=_stats(shape) if stats else None, device=dev)
    if set(pack) == {"state", "forcing"}:
        packed = DeviceWeatherDataset(state, forcing, times, elapsed=elapsed, storage="int16", **kw)
    else:   # one series handed over packed (with the tables of the restatement), the other as floats, storage="float32"
        def maybe(name, x):
            if x is None or name not in pack:
                return x
            scale, offset = R.default_tables(x)
            return PackedSeries(R.encode(x, scale, offset), scale, offset)

        packed = DeviceWeatherDataset(maybe("state", state), maybe("forcing", forcing), times, elapsed=elapsed, **kw)
    dec_state, dec_forcing = packed.decoded("state"), packed.decoded("forcing")
    assert dec_state.dtype == torch.float32 and dec_state.shape == packed.state.shape
    el = None if elapsed is None else elapsed[: dec_state.shape[1]]
    plain = DeviceWeatherDataset(dec_state, dec_forcing, times, elapsed=el, **kw)
    assert plain.storage == "float32" and plain.kernel != "nlam_window_batch_q16" and len(plain) == len(packed)
    return packed, plain


def _assert_batches_equal(got, want, what):
    for name, g, w in zip(("init", "target", "forcing", "times"), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), (what, name)


@pytest.mark.gpu
def test_series_range_merges_chunks_and_counts_non_finite(dev):
    lib = L.load()
    rng = np.random.default_rng(4)
    F = 9
    a, b = _field(rng, (137, F)), _field(rng, (1500, F))   # two chunks of unequal length; the second needs several workgroups
    lo = torch.full((F,), float("inf"), device=dev)
    hi = torch.full((F,), float("-inf"), device=dev)
    bad = torch.zeros((F,), device=dev, dtype=torch.int64)

    def merge(x):
        t = torch.from_numpy(x).to(dev)
        words = int(lib.nlam_series_range_workspace_words(x.shape[0], F))
        assert words > 0
        ws = torch.empty((words,), device=dev, dtype=torch.int32)
        L.check(lib.nlam_series_range(_ptr(t), x.shape[0], F, _ptr(lo), _ptr(hi), _ptr(bad), _ptr(ws), words, _stream()), "range")
        torch.cuda.synchronize()

    merge(a)
    assert np.array_equal(lo.cpu().numpy(), a.min(axis=0)) and np.array_equal(hi.cpu().numpy(), a.max(axis=0))
    merge(b)
    both = np.concatenate([a, b])
    assert np.array_equal(lo.cpu().numpy(), both.min(axis=0)) and np.array_equal(hi.cpu().numpy(), both.max(axis=0))
    assert int(bad.sum()) == 0
    # planted NaN / inf are counted per feature and take no part in the extrema
    c = _field(rng, (301, F))
    c[5, 2], c[300, 2], c[17, 7], c[0, 0] = np.nan, np.inf, -np.inf, np.nan
    finite = np.where(np.isfinite(c), c, np.nan)
    want_lo, want_hi = np.fmin(both.min(axis=0), np.nanmin(finite, axis=0)), np.fmax(both.max(axis=0), np.nanmax(finite, axis=0))
    merge(c)
    assert bad.cpu().tolist() == [1, 0, 2, 0, 0, 0, 0, 1, 0]
    assert np.array_equal(lo.cpu().numpy(), want_lo) and np.array_equal(hi.cpu().numpy(), want_hi)


@pytest.mark.gpu
@pytest.mark.parametrize("dst_offset", [0, 1, 3, 4])
def test_series_pack_equals_the_numpy_encode(dev, dst_offset):
    """Random values, values exactly half-way between two levels (round half to even), values outside the tables' range (the
    clamp); written at an even and an odd element offset into the destination (the 8-byte store and the single-element path)."""
    lib = L.load()
    rng = np.random.default_rng(5)
    rows, F = 613, 9   # 5517 elements: odd, several workgroups
    scale = (2.0 ** rng.integers(-6, 3, size=F)).astype(np.float32)   # powers of two: half-way values are exact in fp32
    offset = rng.integers(-64, 64, size=F).astype(np.float32)
    levels = rng.integers(-32767, 32767, size=(rows, F))
    x = (levels * scale.astype(np.float64) + offset).astype(np.float32)
    x[::3] += (0.5 * scale)                      # exactly half-way to the next level
    assert np.array_equal((x[::3] - offset) / scale, levels[::3] + 0.5)
    assert (R.encode(x[::3], scale, offset) % 2 == 0).all()   # the half-way rows do pin round-half-even
    x[1::3] += (rng.uniform(-0.5, 0.5, size=x[1::3].shape) * scale).astype(np.float32)
    x[4, :], x[5, :] = 1e30, -1e30               # far outside
    x[7, :] = offset + 32767.5 * scale           # half a level outside
    x[8, :] = offset - 32768 * scale
    want = R.encode(x, scale, offset)
    assert want.max() == 32767 and want.min() == -32767
    xd, sd, od = (torch.from_numpy(t).to(dev) for t in (x, scale, offset))
    dst = torch.full((rows * F + 16,), 12345, device=dev, dtype=torch.int16)
    L.check(lib.nlam_series_pack_q16(_ptr(xd), rows, F, _ptr(sd), _ptr(od), _ptr(dst), dst_offset, _stream()), "pack")
    got = dst.cpu().numpy()
    assert np.array_equal(got[dst_offset:dst_offset + rows * F].reshape(rows, F), want)
    assert (got[:dst_offset] == 12345).all() and (got[dst_offset + rows * F:] == 12345).all()   # nothing else is written


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_packed_batch_equals_the_fp32_batch_on_the_decoded_series(dev, layout, shape):
    N, ds, df = shape
    for past, fut in WINDOWS:
        for ar in (1, 3):
            packed, plain = _pair(dev, layout, shape, ar, past, fut)
            assert packed.kernel == "nlam_window_batch_q16" and packed.storage == "int16"
            assert packed.state.dtype == torch.int16 and packed.state_scale.dtype == torch.float32
            assert packed.window == plain.window and packed.num_forcing_features == plain.num_forcing_features
            n = len(packed)
            for idx in ([n - 1], [0, n // 2, n - 1]):
                for standardize in (False, True):
                    what = (past, fut, ar, idx, standardize)
                    want = plain.batch(idx, standardize=standardize)
                    _assert_batches_equal(packed.batch(idx, standardize=standardize), want, what)
                    out = tuple(torch.full_like(t, 7) for t in want)
                    back = packed.batch(idx, standardize=standardize, out=out)
                    assert all(b is o for b, o in zip(back, out))
                    _assert_batches_equal(out, want, what + ("out",))
            # device indices outside the valid range: both paths clamp alike.  The packed cut is nlam_window_batch_ens's, which
            # clamps the flat sample index; nlam_window_batch (the default of a plain fp32 series) clamps every row's time index
            # instead and repeats boundary rows, so the plain layout is compared with the strided fp32 entry here
            if layout == "plain":
                plain.kernel = "nlam_window_batch_ens"
            wild = torch.tensor([-5, n + 3, n - 1], device=dev)
            _assert_batches_equal(packed.batch(wild, standardize=True), plain.batch(wild, standardize=True), (past, fut, ar, "wild"))
            item, ref_item = packed[n - 1], plain[n - 1]
            _assert_batches_equal(item, ref_item, "getitem")


@pytest.mark.gpu
@pytest.mark.parametrize("pack", ["state", "forcing"])
@pytest.mark.parametrize("layout", ["plain", "forecast_members"])
def test_one_series_packed_and_the_other_fp32(dev, layout, pack):
    packed, plain = _pair(dev, layout, SHAPES[0], 3, 1, 1, pack=(pack,))
    assert packed.storage == "mixed" and packed.kernel == "nlam_window_batch_q16"
    assert (packed.state.dtype == torch.int16) == (pack == "state") and (packed.forcing.dtype == torch.int16) == (pack == "forcing")
    assert (packed.state_scale is None) == (pack != "state") and (packed.forcing_offset is None) == (pack != "forcing")
    n = len(packed)
    for standardize in (False, True):
        _assert_batches_equal(packed.batch([0, n - 2, n - 1], standardize=standardize),
                              plain.batch([0, n - 2, n - 1], standardize=standardize), (pack, standardize))


@pytest.mark.gpu
def test_packed_series_with_hand_made_tables_against_the_numpy_oracle(dev):
    """An already packed archive: int16 codes (-32768 included: no special meaning) with tables that come from nowhere near the
    data's range, uploaded as they are; every sample against numpy decode + oracle.data.build_item."""
    from neural_lam_amd.data import DeviceWeatherDataset, PackedSeries
    from oracle import data as od

    N, ds, df = SHAPES[0]
    rng = np.random.default_rng(6)
    qs = rng.integers(-32768, 32768, size=(T_ANALYSIS, N, ds)).astype(np.int16)
    qf = rng.integers(-32768, 32768, size=(T_ANALYSIS, N, df)).astype(np.int16)
    qs[0, 0, 0] = -32768
    s_scale, s_offset = rng.uniform(1e-3, 2.0, size=ds).astype(np.float32), (rng.normal(size=ds) * 1e3).astype(np.float32)
    f_scale, f_offset = rng.uniform(1e-3, 2.0, size=df).astype(np.float32), (rng.normal(size=df) * 1e3).astype(np.float32)
    times = np.arange(T_ANALYSIS, dtype=np.int64) * 60 + 7
    ar, past, fut = 3, 3, 1
    data = DeviceWeatherDataset(PackedSeries(qs, s_scale, s_offset), PackedSeries(qf, f_scale, f_offset), times, ar_steps=ar,
                                num_past_forcing_steps=past, num_future_forcing_steps=fut, device=dev)
    assert data.storage == "int16" and torch.equal(data.state.cpu(), torch.from_numpy(qs))
    state, forcing = R.decode(qs, s_scale, s_offset), R.decode(qf, f_scale, f_offset)
    assert torch.equal(data.decoded("state").cpu(), torch.from_numpy(state))
    assert torch.equal(data.decoded("forcing").cpu(), torch.from_numpy(forcing))
    assert len(data) == od.dataset_len(T_ANALYSIS, T_ANALYSIS, ar, past, fut)
    got = [t.cpu() for t in data.batch(list(range(len(data))))]
    for i in range(len(data)):
        want = od.build_item(state, forcing, times, i, ar, past, fut)
        for g, w in zip(got, want):
            assert torch.equal(g[i], torch.from_numpy(np.ascontiguousarray(w))), i


@pytest.mark.gpu
def test_blocks_on_odd_two_byte_addresses(dev):
    """Two members of 137 x 9 = 1233 codes: every block of member 1 starts 2466 bytes after an aligned one, on an address that is
    2-byte but not 4-byte aligned, and takes the single-element path; member 0's blocks alternate between 8-byte aligned and not."""
    packed, plain = _pair(dev, "forecast_members", SHAPES[0], 3, 1, 1)
    st = packed.state
    assert st.dim() == 5 and st.shape[2] == MEMBERS and st.stride(2) == 1233
    assert st.data_ptr() % 8 == 0 and (st.data_ptr() + 2 * st.stride(2)) % 4 == 2
    assert (packed.forcing.data_ptr() + 2 * packed.forcing.stride(2)) % 4 == 2   # 137 x 3 = 411 codes
    odd = [i for i in range(len(packed)) if i % MEMBERS == 1]
    for standardize in (False, True):
        _assert_batches_equal(packed.batch(odd, standardize=standardize), plain.batch(odd, standardize=standardize), standardize)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["plain", "forecast_members"])
def test_round_trip_on_the_device_and_capacity(dev, layout):
    from neural_lam_amd.data import DeviceWeatherDataset

    shape = SHAPES[0]
    state, forcing, times, elapsed, fc = _series(layout, shape, seed=8)
    state[..., 4] = 273.15   # a constant feature
    kw = dict(ar_steps=3, is_forecast=fc, elapsed=elapsed, device=dev)
    packed = DeviceWeatherDataset(state, forcing, times, storage="int16", **kw)
    plain = DeviceWeatherDataset(state, forcing, times, **kw)
    for name, x in (("state", state), ("forcing", forcing)):
        res = getattr(plain, name).cpu().numpy()            # the resident part of x
        scale = getattr(packed, name + "_scale").cpu().numpy()
        offset = getattr(packed, name + "_offset").cpu().numpy()
        want = R.default_tables(x)
        if not fc:   # (of forecast data only the resident lead times are ranged and packed)
            assert np.array_equal(scale, want[0]) and np.array_equal(offset, want[1])
            assert np.array_equal(getattr(packed, name).cpu().numpy(), R.encode(res, scale, offset))
        back = packed.decoded(name).cpu().numpy()
        assert np.array_equal(back, R.decode(getattr(packed, name).cpu().numpy(), scale, offset))
        err = np.abs(back.astype(np.float64) - res.astype(np.float64))
        assert (err <= R.roundtrip_bound(res, scale, offset)).all(), name
    assert np.array_equal(packed.decoded("state").cpu().numpy()[..., 4], plain.state.cpu().numpy()[..., 4])   # exact
    # capacity: the same elements at half the bytes, the decode tables not counted
    elements = plain.state.numel() + plain.forcing.numel()
    assert packed.state.shape == plain.state.shape and packed.forcing.shape == plain.forcing.shape
    assert plain.resident_bytes == 4 * elements and packed.resident_bytes == 2 * elements
    if fc:   # only the lead times a sample can read are resident: max(2, past) + ar_steps, + future for the forcing
        assert elements == N_ANALYSES * MEMBERS * shape[0] * ((2 + 3) * shape[1] + (2 + 3 + 1) * shape[2])
    else:
        assert elements == T_ANALYSIS * shape[0] * (shape[1] + shape[2])


@pytest.mark.gpu
def test_upload_in_chunks_gives_the_same_codes(dev, monkeypatch):
    """Several chunks of unequal length (range merged chunk by chunk, pack at growing element offsets) against one chunk."""
    from neural_lam_amd import data as D

    state, forcing, times, _, _ = _series("analysis_members", SHAPES[0], seed=9)
    whole = D.DeviceWeatherDataset(state, forcing, times, storage="int16", device=dev)
    monkeypatch.setattr(D, "UPLOAD_CHUNK_BYTES", 4 * state[0].size * 4 + 8)   # 4 time steps of the state per chunk: 14 = 4 + 4 + 4 + 2
    parts = D.DeviceWeatherDataset(torch.from_numpy(state), forcing, times, storage="int16", device=dev)
    for name in ("state", "forcing", "state_scale", "state_offset", "forcing_scale", "forcing_offset"):
        assert torch.equal(getattr(whole, name), getattr(parts, name)), name


@pytest.mark.gpu
def test_non_finite_values_are_refused_before_anything_is_stored(dev):
    from neural_lam_amd.data import DeviceWeatherDataset

    state, forcing, times, _, _ = _series("plain", SHAPES[0], seed=10)
    state[3, 17, 6] = np.nan
    with pytest.raises(ValueError, match=r"state series.*feature 6"):
        DeviceWeatherDataset(state, forcing, times, storage="int16", device=dev)
    state[3, 17, 6] = 0.0
    forcing[0, 0, 1] = np.inf
    with pytest.raises(ValueError, match=r"forcing series.*feature 1"):
        DeviceWeatherDataset(state, forcing, times, storage="int16", device=dev)
    DeviceWeatherDataset(state, forcing, times, device=dev)   # fp32 storage keeps taking them, as before


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["plain", "forecast_members"])
@pytest.mark.parametrize("step_length", [1, 3])
def test_statistics_of_a_packed_dataset_are_bit_identical(dev, layout, step_length):
    from neural_lam_amd.stats import compute_standardization_stats

    packed, plain = _pair(dev, layout, SHAPES[0], 4, 0, 0, seed=11, stats=False)
    got = compute_standardization_stats(packed, step_length=step_length, flux_index=1, batch_size=3)
    want = compute_standardization_stats(plain, step_length=step_length, flux_index=1, batch_size=3)
    assert set(got) == set(want) and "flux_stats" in got
    for key in want:
        assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), key


@pytest.mark.gpu
def test_fp32_entries_refuse_packed_series_with_a_type_error(dev):
    from neural_lam_amd.stats import _moments

    packed, plain = _pair(dev, "plain", SHAPES[1], 3, 1, 1)
    packed.kernel = "nlam_window_batch"
    with pytest.raises(TypeError, match="storage"):
        packed.batch([0])
    packed.kernel = "nlam_window_batch_ens"
    with pytest.raises(TypeError, match="storage"):
        packed.batch([0])
    with pytest.raises(TypeError, match="storage"):
        _moments(plain, packed.state.clone(), 0, 1, 0, 5)   # an int16 tensor that is not the dataset's own packed series


# ---------------------------------------------------------------------------
# GPU: the forecast engines and the trainer
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """The 30 x 27 SyntheticDatastore of the forecast-engine tests with a 13-step series and a forecast-type series on it."""
    from neural_lam_amd.datastore import SyntheticDatastore
    from test_forecast import _graph_of

    root = tmp_path_factory.mktemp("packed_series")
    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=root, boundary="random", seed=1)
    w = types.SimpleNamespace(ds=ds, N=ds.num_grid_points, root=root, graph=_graph_of(ds))
    rng = np.random.default_rng(12)
    w.series = {"plain": (_field(rng, (13, w.N, 5)), _field(rng, (13, w.N, 2)), np.arange(13, dtype=np.int64) * 10 + 1000, None),
                "forecast": (_field(rng, (4, 12, 2, w.N, 5)), _field(rng, (4, 12, 2, w.N, 2)), np.arange(4, dtype=np.int64) * 20 + 1000,
                             np.arange(12, dtype=np.int64) * 10)}
    return w


def _engine_pair(world, dev, step, layout, ar_steps=3):
    from neural_lam_amd.data import DeviceWeatherDataset

    state, forcing, times, elapsed = world.series[layout]
    kw = dict(ar_steps=ar_steps, standardization=step.standardization_stats(), is_forecast=layout == "forecast", device=dev)
    packed = DeviceWeatherDataset(state, forcing, times, elapsed=elapsed, storage="int16", **kw)
    el = None if elapsed is None else elapsed[: packed.state.shape[1]]
    plain = DeviceWeatherDataset(packed.decoded("state"), packed.decoded("forcing"), times, elapsed=el, **kw)
    return packed, plain


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["plain", "forecast"])
def test_forecast_from_a_packed_dataset_equals_the_fp32_engine(dev, world, layout):
    from neural_lam_amd import models as hm
    from neural_lam_amd.forecast import Forecast

    torch.manual_seed(1)
    predictor = hm.MODELS["graph_lam"](world.ds, graph=world.graph, hidden_dim=16, processor_layers=2)
    step = hm.ForecasterStep(hm.ARForecaster(predictor, world.ds), world.ds).to(dev)
    packed, plain = _engine_pair(world, dev, step, layout)
    assert (plain.kernel == "nlam_window_batch") == (layout == "plain")   # the fp32 plain series takes the plain pair
    starts = [1, 4]
    results = {}
    for use_graph in (True, False):
        got_fc = Forecast(step, packed, max_lead=3, batch_size=2, verify=True, use_graph=use_graph)
        want_fc = Forecast(step, plain, max_lead=3, batch_size=2, verify=True, use_graph=use_graph)
        assert got_fc.n_starts == want_fc.n_starts
        got, want = got_fc.run(starts), want_fc.run(starts)
        for name in ("state", "valid_times", "sq", "ab"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (name, use_graph)
        results[use_graph] = got.state.clone()
        if use_graph:   # the recorded step keeps its launch count
            assert got_fc.launches_per_lead == want_fc.launches_per_lead
    assert torch.equal(results[True], results[False])


@pytest.mark.gpu
def test_ensemble_forecast_from_a_packed_dataset_equals_the_fp32_engine(dev, world):
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm
    from neural_lam_amd.forecast import EnsembleForecast

    G.save_graph(world.root / "graph" / "hierarchical",
                 G.create_regular_grid_graph(world.ds.get_xy("state"), n_max_levels=3, hierarchical=True))
    torch.manual_seed(5)
    model = graph_efm.GraphEFM(world.ds, hidden_dim=8)
    step = hm.ForecasterStep(hm.ARForecaster(model, world.ds), world.ds).to(dev)
    packed, plain = _engine_pair(world, dev, step, "forecast")
    mk = lambda ds: EnsembleForecast(step, ds, 3, members=2, n_starts=2, seed=11)   # noqa: E731
    got_fc, want_fc = mk(packed), mk(plain)
    got, want = got_fc.run([1, 6]), want_fc.run([1, 6])
    assert torch.equal(got.members, want.members)
    assert torch.equal(got.crps(step.state_std), want.crps(step.state_std))
    for name in ("ens_sq", "ens_var", "ens_abs", "ens_pair", "rank_hist", "mean", "spread"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert got_fc.launches_per_lead == want_fc.launches_per_lead


@pytest.mark.gpu
def test_training_from_a_packed_dataset_equals_training_from_the_decoded_series(dev, world):
    """Two captured Trainer.step_from steps: the losses and every parameter after the second step, bit for bit."""
    from neural_lam_amd import models as hm
    from neural_lam_amd.trainer import Trainer

    def make():
        torch.manual_seed(3)
        fc = hm.ARForecaster(hm.GraphLAM(world.ds, graph=world.graph, hidden_dim=16, processor_layers=2), world.ds)
        return Trainer(hm.ForecasterStep(fc, world.ds, standardize=False).to(dev), lr=1e-3, use_graph=True)

    t_packed, t_plain = make(), make()
    packed, plain = _engine_pair(world, dev, t_packed.module, "plain", ar_steps=2)
    perm = packed.epoch_permutation(seed=2)
    for k in range(2):
        idx = perm[2 * k: 2 * k + 2]
        l_packed, l_plain = float(t_packed.step_from(packed, idx)), float(t_plain.step_from(plain, idx))
        assert l_packed == l_plain, (k, l_packed, l_plain)
        assert torch.equal(t_packed.batch_times, t_plain.batch_times)
    assert t_packed._graph is not None and t_plain._graph is not None
    assert torch.equal(t_packed.fp.flat, t_plain.fp.flat)
