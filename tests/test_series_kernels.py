"""The row loops every data kernel shares (csrc/nlam_series.inc: series_state_row, series_forcing_row over fp32 and packed int16
series) at the instantiations and paths the per-feature suites do not reach:

* the float instantiations of the strided forecast pair launched through the packed entries (no packed series named): the bits of
  nlam_forecast_init_strided / _head_strided;
* the forecast pair on one packed and one fp32 series, and on two packed series whose blocks start on odd 2-byte addresses,
  against numpy (packed_ref.decode, oracle.data.build_item + standardize_item: IEEE fp32 sub, then div);
* every batch kernel on rows that are no multiple of four elements with standardisation off (no forecast kernel takes that path),
  against numpy.

Everything is torch.equal / np.array_equal: no tolerance.  Blocks are 137 x 9 = 1233, 137 x 3 = 411, 37 x 5 = 185 or 37 x 3 x 2 = 222
elements: odd or no multiple of 4, the first longer than the 1024 elements a workgroup covers per sweep."""
import ctypes as C

import numpy as np
import pytest
import torch

import packed_ref as R
import test_packed_series as PS
from neural_lam_amd import _lib as L
from oracle import data as od
from test_forecast_datasets import LEAD, MEMBERS, NVARS, _bits, _misaligned, _ptr, _stream, _strided_dataset


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


class _Pair:
    """The buffers and the nlam_forecast_t of an init / head pair over `data`, and its launches through any of the entries."""

    def __init__(self, dev, data, max_lead, batch, put=lambda t: t):
        nodes, ds = data.state.shape[-2:]
        self.d_forcing = 0 if data.forcing is None else data.forcing.shape[-1]
        self.max_lead = max_lead
        nan = lambda *shape: put(torch.full(shape, float("nan"), device=dev))   # noqa: E731
        self.prev, self.pprev, self.truth = nan(batch, nodes, ds), nan(batch, nodes, ds), nan(batch, nodes, ds)
        self.fw = nan(batch, nodes, self.d_forcing * data.window)
        self.idx = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.lead = torch.full((1,), 7, dtype=torch.int32, device=dev)
        p = L.Forecast()
        p.lead = _ptr(self.lead)
        p.state_mean, p.state_std = _ptr(data.stats["state_mean"]), _ptr(data.stats["state_std"])
        p.forcing_mean, p.forcing_std = _ptr(data.stats.get("forcing_mean")), _ptr(data.stats.get("forcing_std"))
        p.prev, p.prev_prev, p.truth = _ptr(self.prev), _ptr(self.pprev), _ptr(self.truth)
        p.forcing_windowed = _ptr(self.fw) if self.d_forcing else None
        p.nodes, p.d_state, p.d_forcing, p.batch = nodes, ds, self.d_forcing, batch
        p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps = max_lead, data.num_past_forcing_steps, data.num_future_forcing_steps
        self.p = p

    def run(self, lib, suffix, *sources):
        """(prev_prev, prev, [truth of lead k], [forcing window of lead k]) of nlam_forecast_init<suffix> / _head<suffix>."""
        init, head = getattr(lib, "nlam_forecast_init" + suffix), getattr(lib, "nlam_forecast_head" + suffix)
        extra = [C.byref(s) for s in sources]
        for t in (self.prev, self.pprev):
            t.fill_(float("nan"))
        self.lead.fill_(7)
        L.check(init(C.byref(self.p), *extra, _stream()), "nlam_forecast_init" + suffix)
        assert int(self.lead) == 0
        truths, windows = [], []
        for k in range(self.max_lead):
            self.lead.fill_(k)
            self.truth.fill_(float("nan"))
            self.fw.fill_(float("nan"))
            L.check(head(C.byref(self.p), *extra, _stream()), "nlam_forecast_head" + suffix)
            truths.append(self.truth.clone())
            windows.append(self.fw.clone())
        return self.pprev.clone(), self.prev.clone(), truths, windows


@pytest.mark.gpu
@pytest.mark.parametrize("nodes,misalign", [(37, False), (36, False), (36, True)])
@pytest.mark.parametrize("layout", ["forecast", "analysis"])
@pytest.mark.parametrize("past,fut", [(0, 0), (3, 1)])
def test_packed_entries_without_a_packed_series_give_the_bits_of_the_strided_entries(dev, past, fut, layout, nodes, misalign):
    """nlam_forecast_init_q16 / _head_q16 with both packed pointers NULL launch the float instantiations, as the strided entries do.
    nodes = 37: blocks of 185 floats, every other member's rows off a 16-byte boundary; nodes = 36: the 16-byte path; misalign: every
    base and every destination one float off.  The last index lies outside the dataset and is clamped."""
    from neural_lam_amd.forecast import dataset_source

    lib = L.load()
    data, _, d_forcing = _strided_dataset(dev, layout, "members", past, fut, nodes, misalign)
    assert d_forcing == 2 and data.state.shape[-2:] == (nodes, NVARS) and data.members == MEMBERS
    pair = _Pair(dev, data, LEAD, 3, put=_misaligned if misalign else (lambda t: t))
    assert (pair.truth.data_ptr() % 16 == 4) == misalign
    count = len(data)
    pair.idx.copy_(torch.tensor([1, count - 1, count + 7], dtype=torch.int64))
    src = dataset_source(data, pair.idx)
    want = pair.run(lib, "_strided", src)
    got = pair.run(lib, "_q16", src, L.Q16Src())
    assert not bool(torch.isnan(want[0]).any()) and not bool(torch.isnan(want[3][-1]).any())
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1]))
    for k in range(LEAD):
        assert torch.equal(_bits(got[2][k]), _bits(want[2][k])), k
        assert torch.equal(_bits(got[3][k]), _bits(want[3][k])), k


P_LEAD = 3
P_SHAPE = PS.SHAPES[0]   # 137 nodes, 9 state and 3 forcing features


def _packed_dataset(dev, layout, shape, pack, ar, past, fut, stats):
    """(dataset, state, forcing, times): the dataset keeps the series named in `pack` as int16 codes with the tables of the
    restatement; state and forcing are the float32 numpy series it stands for (decoded where packed)."""
    from neural_lam_amd.data import DeviceWeatherDataset, PackedSeries

    state, forcing, times, elapsed, fc = PS._series(layout, shape)
    given, stands_for = {}, {}
    for name, x in (("state", state), ("forcing", forcing)):
        if name in pack:
            scale, offset = R.default_tables(x)
            codes = R.encode(x, scale, offset)
            given[name], stands_for[name] = PackedSeries(codes, scale, offset), R.decode(codes, scale, offset)
        else:
            given[name] = stands_for[name] = x
    data = DeviceWeatherDataset(given["state"], given["forcing"], times, elapsed=elapsed, ar_steps=ar, num_past_forcing_steps=past,
                                num_future_forcing_steps=fut, is_forecast=fc, standardization=PS._stats(shape) if stats else None,
                                device=dev)
    assert (data.state.dtype == torch.int16) == ("state" in pack) and (data.forcing.dtype == torch.int16) == ("forcing" in pack)
    return data, stands_for["state"], stands_for["forcing"], times


def _member_series(layout, state, forcing, i, members):
    """The (time, nodes, features) series of flat sample i and its index on that time axis."""
    s, m = divmod(i, members)
    if layout == "plain":
        return state, forcing, i
    if layout == "analysis_members":
        return state[:, m], forcing[:, m], s
    assert layout == "forecast_members"
    return state[s, :, m], forcing[s, :, m], 0


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [("state",), ("forcing",), ("state", "forcing")], ids="+".join)
@pytest.mark.parametrize("layout", ["analysis_members", "forecast_members"])
def test_forecast_pair_on_packed_and_mixed_series_against_numpy(dev, layout, pack):
    """State packed and forcing fp32, the reverse, and both packed.  Two members of 1233 (state) and 411 (forcing) codes or floats:
    a packed block of member 1 starts on an address that is 2-byte but not 4-byte aligned and is read code by code, member 0's blocks
    alternate between 8-byte aligned and not; the fp32 blocks alternate around the 16-byte boundary in the same way."""
    from neural_lam_amd.forecast import dataset_source

    lib = L.load()
    past, fut = 3, 1
    data, state, forcing, _ = _packed_dataset(dev, layout, P_SHAPE, pack, P_LEAD, past, fut, stats=True)
    assert data.members == PS.MEMBERS == 2 and data.storage == ("int16" if len(pack) == 2 else "mixed")
    for name in pack:
        x = getattr(data, name)
        m_ax = x.dim() - 3
        assert x.stride(m_ax) % 2 == 1 and x.data_ptr() % 8 == 0 and (x.data_ptr() + 2 * x.stride(m_ax)) % 4 == 2
    count = len(data)
    picks = [1, count - 2, count - 1]   # members 1, 0 and 1
    assert [i % 2 for i in picks] == [1, 0, 1]
    pair = _Pair(dev, data, P_LEAD, len(picks))
    pair.idx.copy_(torch.tensor(picks, dtype=torch.int64))
    pprev, prev, truths, windows = pair.run(lib, "_q16", dataset_source(data, pair.idx), data.packed_source())
    st = PS._stats(P_SHAPE)
    for b, i in enumerate(picks):
        s, f, t = _member_series(layout, state, forcing, i, 2)
        item = od.build_item(s, f, None, t, P_LEAD, past, fut)
        init, target, forc = od.standardize_item(item[0], item[1], item[2], st["state_mean"], st["state_std"], st["forcing_mean"],
                                                 st["forcing_std"], past + fut + 1)
        assert init.dtype == np.float32 and forc.dtype == np.float32
        assert np.array_equal(pprev[b].cpu().numpy(), init[0]) and np.array_equal(prev[b].cpu().numpy(), init[1]), i
        for k in range(P_LEAD):
            assert np.array_equal(truths[k][b].cpu().numpy(), target[k]), (i, k)
            assert np.array_equal(windows[k][b].cpu().numpy(), forc[k]), (i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [(), ("state",), ("forcing",), ("state", "forcing")], ids=lambda p: "+".join(p) or "fp32")
@pytest.mark.parametrize("layout", ["plain", "analysis_members"])
def test_batch_kernels_on_rows_off_the_quad_path_without_standardisation(dev, layout, pack):
    """37 x 5 = 185 state and 37 x 3 x 2 = 222 windowed forcing elements per row: no multiple of 4, so every row is read and written
    element by element, and nothing is standardised.  fp32 plain series: nlam_window_batch; fp32 members: nlam_window_batch_ens; any
    packed series: the matching instantiation behind nlam_window_batch_q16.  Every sample against numpy."""
    shape, ar, past, fut = (37, 5, 3), 3, 1, 0
    data, state, forcing, times = _packed_dataset(dev, layout, shape, pack, ar, past, fut, stats=False)
    assert data.kernel == ("nlam_window_batch_q16" if pack else "nlam_window_batch" if layout == "plain" else "nlam_window_batch_ens")
    members = 1 if layout == "plain" else 2
    assert data.members == members and len(data) == members * od.dataset_len(PS.T_ANALYSIS, PS.T_ANALYSIS, ar, past, fut)
    got = [t.cpu().numpy() for t in data.batch(list(range(len(data))), standardize=False)]
    assert got[0].shape[1:] == (2, 37, 5) and got[2].shape[1:] == (ar, 37, 6)
    for i in range(len(data)):
        s, f, t = _member_series(layout, state, forcing, i, members)
        want = od.build_item(s, f, times, t, ar, past, fut)
        for name, g, w in zip(("init", "target", "forcing", "times"), got, want):
            assert np.array_equal(g[i], w), (i, name)
