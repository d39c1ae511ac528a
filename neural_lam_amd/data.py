"""The training data path on the GPU: samples cut out of time series that live in HBM.

Mirror of the reference's ``neural_lam/weather_dataset.py`` ``WeatherDataset`` -- ``__len__`` (:118-200),
``__getitem__`` (:467-533): same constructor arguments (``ar_steps``, ``num_past_forcing_steps``,
``num_future_forcing_steps``, ``load_single_member``), same 4-tuple ``(init_states, target_states, forcing, target_times)``,
same IndexError / negative-index behaviour -- but the xarray slicing, the host tensors and the DataLoader collation are
replaced by ONE launch that writes a whole batch from the resident series, reading its sample indices on the device,
optionally with ``ForecasterModule.on_after_batch_transfer`` (models/module.py:326-367) folded into the same pass.  A
MEPS-sized year of analyses (2 920 steps x 63 784 nodes x 17 + 6 variables, fp32) is 17 GB: it fits the 288 GB of one
MI355X many times over, so an epoch needs no host->device traffic at all (a resident permutation supplies the indices).

Both kinds of datastore are covered: analysis data (one time series, ``(time, [member], N, F)``) and forecast data
(``(analysis_time, elapsed_forecast_duration, [member], N, F)``, weather_dataset.py:135-178, :233-254, :300-329), each
with or without an ensemble-member axis.  Plain analysis series (no member axis left on the device) are cut by
``nlam_window_batch``; everything else by ``nlam_window_batch_ens``, which reads strided series.  Of a forecast only the
lead times a sample can read stay resident -- ``max(2, past) + ar_steps`` for the state, ``+ future`` for the forcing --
and host arrays (numpy memmaps included) are uploaded in chunks of analysis times, so the host never holds more than one
chunk and HBM never holds the unread tail of the forecasts.

``storage="int16"`` keeps the series as packed 16-bit codes with a per-feature ``scale`` / ``offset`` (the packing of GRIB
and packed netCDF), half the bytes of fp32: float series are packed on upload (exact range first, then the encoding, chunk
by chunk), ``PackedSeries`` hands over codes that are packed already.  ``nlam_window_batch_q16`` decodes them in the batch
launch, so the batches are fp32 as ever and carry the bits of an fp32 dataset holding the decoded series.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L

# host -> device uploads go in slices of the leading (time / analysis-time) axis of at most this many bytes
UPLOAD_CHUNK_BYTES = 256 << 20


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Layout(NamedTuple):
    """What ``plan_layout`` decides from the shapes alone (no device needed)."""
    n_times: int                    # leading axis: time steps (analysis) or analysis times (forecast), state and forcing in common
    state_members: Optional[int]    # size of the state's member axis, None without one
    forcing_members: Optional[int]  # the same for the forcing
    members: int                    # members the flat index runs over (1 under load_single_member or without a member axis)
    state_steps: Optional[int]      # forecast: lead times kept resident for the state (max(2, past) + ar_steps)
    forcing_steps: Optional[int]    # forecast: lead times kept resident for the forcing (+ future)
    keep_state_members: bool        # False: only member 0 of the state is ever read (and kept)
    keep_forcing_members: bool      # False: only member 0 of the forcing is ever read (and kept)
    base_len: int                   # samples per member
    length: int                     # len(dataset) = base_len * members


def plan_layout(state_shape, forcing_shape=None, *, is_forecast=False, ar_steps=3, num_past_forcing_steps=1,
                num_future_forcing_steps=1, load_single_member=False):
    """Shape checks, ``len()`` and the resident layout of ``DeviceWeatherDataset`` (weather_dataset.py:85-90, :118-200).

    ``state_shape``: ``(time, [member], N, F)`` for analysis data, ``(analysis_time, elapsed, [member], N, F)`` for forecast
    data -- the member axis is inferred from the rank; ``forcing_shape`` the same (or None).  Raises ValueError for
    malformed shapes and, for forecasts, too short a lead-time axis; warns (UserWarning) under ``load_single_member``."""
    state_shape = tuple(int(x) for x in state_shape)
    ranks = (4, 5) if is_forecast else (3, 4)
    dims = "(analysis_time, elapsed_forecast_duration, [ensemble_member], num_grid_nodes, %s)" if is_forecast else \
        "(n_times, [ensemble_member], num_grid_nodes, %s)"
    if len(state_shape) not in ranks:
        raise ValueError("state must be " + dims % "num_state_vars")
    ar, past, fut = int(ar_steps), int(num_past_forcing_steps), int(num_future_forcing_steps)
    off = max(2, past)
    state_members = state_shape[-3] if len(state_shape) == ranks[1] else None
    forcing_members = None
    if forcing_shape is not None:
        forcing_shape = tuple(int(x) for x in forcing_shape)
        if len(forcing_shape) not in ranks or forcing_shape[-2] != state_shape[-2]:
            raise ValueError("forcing must be " + dims % "num_forcing_vars" + " on the same nodes as state")
        if forcing_shape[-1] == 0:
            forcing_shape = None
    if forcing_shape is not None:
        forcing_members = forcing_shape[-3] if len(forcing_shape) == ranks[1] else None
        if is_forecast and forcing_shape[0] != state_shape[0]:
            raise ValueError(f"forcing has {forcing_shape[0]} analysis times, state {state_shape[0]}: they must be the same")
        if forcing_members is not None and state_members is not None and forcing_members != state_members:
            raise ValueError(f"forcing has {forcing_members} ensemble members, state {state_members}: they must be the same")
    if state_members is not None and state_members < 1:
        raise ValueError("the state's ensemble-member axis is empty")
    if state_members is not None and load_single_member:
        warnings.warn("only using first ensemble member, so dataset size is effectively reduced by the number of ensemble "
                      f"members ({state_members})", UserWarning, stacklevel=3)
    members = state_members if state_members is not None and not load_single_member else 1
    state_steps = forcing_steps = None
    if is_forecast:
        # weather_dataset.py:135-180, with its wording
        if state_shape[1] < off + ar:
            raise ValueError(f"The number of forecast steps available ({state_shape[1]}) is less than the required {off + ar} "
                             f"(max(2, num_past_forcing_steps={past}) + ar_steps={ar}) for creating a sample with initial and "
                             "target states.")
        state_steps = off + ar
        if forcing_shape is not None:
            if forcing_shape[1] < off + ar + fut:
                raise ValueError(f"The number of forcing forecast steps available ({forcing_shape[1]}) is less than the "
                                 f"required {off + ar + fut} (max(2, num_past_forcing_steps={past}) + ar_steps={ar} + "
                                 f"num_future_forcing_steps={fut}) for constructing forcing windows.")
            forcing_steps = off + ar + fut
        n_times = base_len = state_shape[0]
    else:
        n_times = state_shape[0] if forcing_shape is None else min(state_shape[0], forcing_shape[0])
        base_len = max(0, n_times - (off + ar + fut) + 1)   # nlam_window_len: the same arithmetic in the C-ABI
    return Layout(n_times=n_times, state_members=state_members, forcing_members=forcing_members, members=members,
                  state_steps=state_steps, forcing_steps=forcing_steps,
                  keep_state_members=state_members is not None and members > 1,
                  keep_forcing_members=forcing_members is not None and members > 1,
                  base_len=base_len, length=base_len * members)


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _resident(x, dev, steps, member_axis, keep_members):
    """The part of series ``x`` a sample can read, contiguous fp32 on ``dev``: lead times ``[0, steps)`` of axis 1 when
    ``steps`` is set, member 0 only (axis dropped) when the member axis exists and ``keep_members`` is False.  A device
    tensor is sliced on the device (no copy when nothing is cut); a host array -- numpy, memmap, torch CPU tensor -- is
    copied in chunks of the leading axis of at most UPLOAD_CHUNK_BYTES."""
    if not hasattr(x, "shape"):
        x = np.asarray(x, dtype=np.float32)
    sl = [slice(None)] * len(x.shape)
    if steps is not None:
        sl[1] = slice(0, steps)
    if member_axis is not None and not keep_members:
        sl[member_axis] = 0
    sl = tuple(sl)
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.to(dev, torch.float32)[sl].contiguous()
    rest = sl[1:]
    n0 = int(x.shape[0])
    shape = (n0,) + tuple(len(range(*r.indices(int(d)))) for d, r in zip(x.shape[1:], rest) if isinstance(r, slice))
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    row_bytes = 4 * max(1, int(np.prod(shape[1:], dtype=np.int64)))
    step = max(1, int(UPLOAD_CHUNK_BYTES) // row_bytes)
    for a0 in range(0, n0, step):
        a1 = min(n0, a0 + step)
        piece = x[(slice(a0, a1),) + rest]
        if isinstance(piece, torch.Tensor):
            piece = piece.to(torch.float32).contiguous()
        else:
            piece = np.ascontiguousarray(piece, dtype=np.float32)
            if not piece.flags.writeable:   # a read-only memmap chunk: torch.from_numpy wants writable memory
                piece = piece.copy()
            piece = torch.from_numpy(piece)
        out[a0:a1].copy_(piece)
    return out


class PackedSeries:
    """A series that is already packed, as GRIB and packed netCDF archives ship it: ``values`` int16 of the usual shape
    (``(time, [member], N, F)`` or ``(analysis_time, elapsed, [member], N, F)``; numpy, memmap, torch CPU or device tensor)
    with the per-feature fp32 tables of the archive, ``x = float32(q) * scale[f] + offset[f]`` (two fp32 roundings).  It is
    uploaded as it is, with no float pass.  TypeError unless ``values`` is int16; ValueError unless both tables hold ``F``
    finite entries and every ``scale > 0``.  The code -32768 has no special meaning (fill gaps before packing)."""

    def __init__(self, values, scale, offset):
        if not hasattr(values, "shape"):
            values = np.asarray(values)
        if str(values.dtype).replace("torch.", "") != "int16":
            raise TypeError(f"PackedSeries: values must be int16, got {values.dtype}")
        if len(values.shape) < 1:
            raise ValueError("PackedSeries: values must have a feature axis")
        F = int(values.shape[-1])
        tabs = []
        for name, t in (("scale", scale), ("offset", offset)):
            a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            if a.shape != (F,):
                raise ValueError(f"PackedSeries: {name} must have one entry per feature ({F}), got {a.size}")
            if not np.isfinite(a).all():
                raise ValueError(f"PackedSeries: {name} must be finite")
            tabs.append(a)
        if not (tabs[0] > 0).all():
            raise ValueError("PackedSeries: scale must be > 0 for every feature")
        self.values, self.scale, self.offset = values, tabs[0], tabs[1]

    @property
    def shape(self):
        return tuple(self.values.shape)


def default_tables(lo, hi):
    """The decode tables of features with the exact ranges ``[lo, hi]`` (float64 on the host): ``offset = fp32((hi + lo) / 2)``,
    ``scale = fp32((hi - lo) / 65534)``, so the extrema land on the codes -+32767.  A constant feature gets ``scale = 1`` and
    its value as the offset (it round-trips exactly); so does a range so small that its scale underflows fp32."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(over="ignore"):
        offset = ((hi + lo) / 2).astype(np.float32)
        scale = ((hi - lo) / 65534).astype(np.float32)
    flat = ~(scale > 0)
    scale[flat] = 1.0
    offset[flat & (hi == lo)] = lo[flat & (hi == lo)].astype(np.float32)
    return scale, offset


def _cut(x, steps, member_axis, keep_members):
    """(index of the axes behind the leading one, resident shape) of the part of ``x`` a sample can read: ``_resident``'s cut."""
    sl = [slice(None)] * len(x.shape)
    if steps is not None:
        sl[1] = slice(0, steps)
    if member_axis is not None and not keep_members:
        sl[member_axis] = 0
    rest = tuple(sl[1:])
    n0 = int(x.shape[0])
    shape = (n0,) + tuple(len(range(*r.indices(int(d)))) for d, r in zip(x.shape[1:], rest) if isinstance(r, slice))
    return rest, shape


def _pieces(x, dev, rest, shape, dtype):
    """``(a0, a1, chunk)``: the resident part of ``x`` in contiguous device chunks of its leading axis, each of at most
    UPLOAD_CHUNK_BYTES in ``dtype`` (``_resident``'s chunks); a host array is converted and copied chunk by chunk."""
    np_dtype = {torch.float32: np.float32, torch.int16: np.int16}[dtype]
    row_bytes = np.dtype(np_dtype).itemsize * max(1, int(np.prod(shape[1:], dtype=np.int64)))
    step = max(1, int(UPLOAD_CHUNK_BYTES) // row_bytes)
    for a0 in range(0, shape[0], step):
        a1 = min(shape[0], a0 + step)
        piece = x[(slice(a0, a1),) + rest]
        if isinstance(piece, torch.Tensor):
            piece = piece.to(dtype).contiguous().to(dev)
        else:
            piece = np.ascontiguousarray(piece, dtype=np_dtype)
            if not piece.flags.writeable:   # a read-only memmap chunk: torch.from_numpy wants writable memory
                piece = piece.copy()
            piece = torch.from_numpy(piece).to(dev)
        yield a0, a1, piece


def _resident_q16(name, x, dev, steps, member_axis, keep_members, lib):
    """``_resident`` for packed storage: ``(values int16, scale, offset)`` on ``dev``.  A ``PackedSeries`` is cut and uploaded
    as it is.  A float series takes two passes over the chunks of its leading axis -- ``nlam_series_range`` merges the exact
    per-feature range, then ``nlam_series_pack_q16`` encodes with the tables of that range -- so the host never holds more than
    one chunk and the device never an fp32 copy of more than one.  ValueError (before anything is stored) for a non-finite value."""
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    if isinstance(x, PackedSeries):
        rest, shape = _cut(x.values, steps, member_axis, keep_members)
        out = torch.empty(shape, dtype=torch.int16, device=dev)
        for a0, a1, piece in _pieces(x.values, dev, rest, shape, torch.int16):
            out[a0:a1].copy_(piece)
        return out, torch.from_numpy(x.scale.copy()).to(dev), torch.from_numpy(x.offset.copy()).to(dev)
    if not hasattr(x, "shape"):
        x = np.asarray(x, dtype=np.float32)
    rest, shape = _cut(x, steps, member_axis, keep_members)
    F = int(shape[-1])
    if F > L.MOMENTS_MAX_VARS:
        raise ValueError(f"{name}: {F} features; the range kernel of storage='int16' takes at most {L.MOMENTS_MAX_VARS}")
    with torch.cuda.device(dev):
        lo = torch.full((F,), float("inf"), device=dev, dtype=torch.float32)
        hi = torch.full((F,), float("-inf"), device=dev, dtype=torch.float32)
        bad = torch.zeros((F,), device=dev, dtype=torch.int64)
        ws = None
        for _, _, piece in _pieces(x, dev, rest, shape, torch.float32):
            rows = piece.numel() // F
            if rows == 0:
                continue
            words = int(lib.nlam_series_range_workspace_words(rows, F))
            if ws is None or ws.numel() < words:
                ws = torch.empty((words,), device=dev, dtype=torch.int32)
            L.check(lib.nlam_series_range(_ptr(piece), rows, F, _ptr(lo), _ptr(hi), _ptr(bad), _ptr(ws), ws.numel(), stream()),
                    "nlam_series_range")
        bad_host = bad.cpu().numpy()
        if bad_host.any():
            f = int(np.flatnonzero(bad_host)[0])
            raise ValueError(f"storage='int16': the {name} series holds non-finite values ({int(bad_host[f])} in feature {f}, the "
                             "first of them); fill gaps before packing -- the format has no missing-value code")
        if ws is None:   # no element at all
            scale, offset = np.ones(F, np.float32), np.zeros(F, np.float32)
        else:
            scale, offset = default_tables(lo.cpu().numpy(), hi.cpu().numpy())
        scale, offset = torch.from_numpy(scale).to(dev), torch.from_numpy(offset).to(dev)
        out = torch.empty(shape, dtype=torch.int16, device=dev)
        per = int(np.prod(shape[1:], dtype=np.int64))
        for a0, _, piece in _pieces(x, dev, rest, shape, torch.float32):
            rows = piece.numel() // F
            if rows:
                L.check(lib.nlam_series_pack_q16(_ptr(piece), rows, F, _ptr(scale), _ptr(offset), _ptr(out), a0 * per, stream()),
                        "nlam_series_pack_q16")
            del piece
    return out, scale, offset


def _ns(x, dev):
    """int64 nanoseconds on ``dev`` from int64 / numpy datetime64 / timedelta64 stamps."""
    if not isinstance(x, torch.Tensor):
        a = np.asarray(x)
        if a.dtype.kind == "M":
            a = a.astype("datetime64[ns]").astype(np.int64)
        elif a.dtype.kind == "m":
            a = a.astype("timedelta64[ns]").astype(np.int64)
        x = a
    return torch.as_tensor(x, dtype=torch.int64).to(dev).contiguous()


class DeviceWeatherDataset:
    """``WeatherDataset`` (weather_dataset.py:20-116) over device-resident series.

    is_forecast=False (analysis data):
        state    (n_times, [ensemble_member], num_grid_nodes, num_state_vars)   float32
        forcing  (n_times, [ensemble_member], num_grid_nodes, num_forcing_vars) float32 or None
        times    (n_times,) int64 nanoseconds (or datetime64) or None (then ``target_times`` are time indices)
    is_forecast=True (forecast data, e.g. a ``npyfilesmeps`` store):
        state    (analysis_time, elapsed_forecast_duration, [ensemble_member], num_grid_nodes, num_state_vars)
        forcing  (analysis_time, elapsed_forecast_duration, [ensemble_member], num_grid_nodes, num_forcing_vars) or None
        times    (analysis_time,) analysis times and ``elapsed`` (elapsed_forecast_duration,) lead times, both int64 ns (or
                 datetime64 / timedelta64) or both None (then ``target_times`` are lead-time indices)
    The member axis is inferred from the rank.  With one, ``len()`` is samples x members and index ``i`` is sample
    ``i // members``, member ``i % members`` (weather_dataset.py:399-409); forcing with a member axis follows the state's
    member, forcing without one is shared.  ``load_single_member=True`` uses member 0 only (and warns, :85-90).
    standardization: optional dict with ``state_mean, state_std, forcing_mean, forcing_std`` (the buffers
    ForecasterModule registers, module.py:159-215, std already clamped) for ``batch(..., standardize=True)``.
    ``kernel`` names the C entry that cuts the batches: ``"nlam_window_batch"`` for plain analysis series,
    ``"nlam_window_batch_ens"`` otherwise (the strided entry may be selected for any layout; it gives the same samples).
    storage: ``"float32"`` (default) keeps float series as fp32; ``"int16"`` packs them on upload with the tables of each
    feature's exact range (``default_tables``; ValueError for a non-finite value, before anything is stored).  A
    ``PackedSeries`` for ``state`` and / or ``forcing`` is kept packed under either setting, so one series may be packed and
    the other fp32.  With a packed series ``kernel`` is ``"nlam_window_batch_q16"`` (every layout), ``state`` / ``forcing`` are
    the int16 tensors, ``state_scale`` / ``state_offset`` / ``forcing_scale`` / ``forcing_offset`` the fp32 decode tables on the
    device (None for an fp32 series), ``resident_bytes`` the HBM the series take and ``decoded()`` the fp32 series they stand for.
    """

    def __init__(self, state, forcing=None, times=None, ar_steps=3, num_past_forcing_steps=1, num_future_forcing_steps=1,
                 standardization=None, device="cuda", is_forecast=False, elapsed=None, load_single_member=False,
                 storage="float32"):
        dev = torch.device(device)
        if storage not in ("float32", "int16"):
            raise ValueError(f"storage must be 'float32' or 'int16', got {storage!r}")
        if dev.type != "cuda":
            raise RuntimeError("DeviceWeatherDataset keeps its series in HBM and cuts samples with a HIP kernel: it needs a GPU "
                               "(there is no CPU fallback; the CPU restatement lives in oracle/data.py for the tests)")
        self.is_forecast = bool(is_forecast)
        self.ar_steps = int(ar_steps)
        self.num_past_forcing_steps = int(num_past_forcing_steps)
        self.num_future_forcing_steps = int(num_future_forcing_steps)
        self.load_single_member = bool(load_single_member)
        lay = plan_layout(_shape(state), None if forcing is None else _shape(forcing), is_forecast=self.is_forecast,
                          ar_steps=self.ar_steps, num_past_forcing_steps=self.num_past_forcing_steps,
                          num_future_forcing_steps=self.num_future_forcing_steps, load_single_member=self.load_single_member)
        self.layout = lay
        if self.is_forecast and (times is None) != (elapsed is None):
            raise ValueError("forecast data: give both the analysis times and the elapsed forecast durations, or neither")
        if not self.is_forecast and elapsed is not None:
            raise ValueError("elapsed is the lead-time axis of forecast data (is_forecast=True)")
        s_shape = _shape(state)
        m_ax = len(s_shape) - 3
        self._lib = L.load()
        self.state_scale = self.state_offset = self.forcing_scale = self.forcing_offset = None

        def resident(name, x, steps, member_axis, keep):   # (series, scale, offset): fp32 as ever, or packed int16 with its tables
            if storage == "int16" or isinstance(x, PackedSeries):
                return _resident_q16(name, x, dev, steps, member_axis, keep, self._lib)
            return _resident(x, dev, steps, member_axis, keep), None, None

        self.state, self.state_scale, self.state_offset = resident(
            "state", state, lay.state_steps, m_ax if lay.state_members is not None else None, lay.keep_state_members)
        self.forcing = None
        if forcing is not None and _shape(forcing)[-1] > 0:
            f_ax = len(_shape(forcing)) - 3
            self.forcing, self.forcing_scale, self.forcing_offset = resident(
                "forcing", forcing, lay.forcing_steps, f_ax if lay.forcing_members is not None else None, lay.keep_forcing_members)
        self.times = None if times is None else _ns(times, dev)
        if self.times is not None and self.times.shape != (s_shape[0],):
            raise ValueError("times must have one entry per state time step" if not self.is_forecast else
                             "times must have one entry per analysis time")
        self.elapsed = None
        if elapsed is not None:
            e = _ns(elapsed, dev)
            if e.shape != (s_shape[1],):
                raise ValueError("elapsed must have one entry per lead time of the state")
            self.elapsed = e[: lay.state_steps].contiguous()
        self.members = lay.members
        self._nodes, self._d_state = int(s_shape[-2]), int(s_shape[-1])
        self.device = dev
        plain = not self.is_forecast and self.state.dim() == 3 and (self.forcing is None or self.forcing.dim() == 3)
        self.kernel = "nlam_window_batch" if plain else "nlam_window_batch_ens"
        if self.state_scale is not None or self.forcing_scale is not None:
            self.kernel = "nlam_window_batch_q16"   # any layout: the strided entry with the decode in flight
        if plain:
            n_forc = -1 if self.forcing is None else self.forcing.shape[0]
            self._len = int(self._lib.nlam_window_len(self.state.shape[0], n_forc, self.ar_steps, self.num_past_forcing_steps,
                                                      self.num_future_forcing_steps))
        else:
            self._len = lay.length
        # one common time axis for the kernel: it indexes both series with the same time index
        self._n_times = lay.n_times
        self.stats = None
        if standardization is not None:
            g = lambda k: torch.as_tensor(standardization[k], dtype=torch.float32).to(dev).contiguous()  # noqa: E731
            self.stats = {"state_mean": g("state_mean"), "state_std": g("state_std")}
            if self.forcing is not None:
                self.stats.update(forcing_mean=g("forcing_mean"), forcing_std=g("forcing_std"))

    # ---- the reference's surface ----
    @property
    def window(self):
        return self.num_past_forcing_steps + self.num_future_forcing_steps + 1

    @property
    def num_forcing_features(self):
        return 0 if self.forcing is None else self.forcing.shape[-1] * self.window

    def __len__(self):
        return self._len

    # ---- packed storage ----
    @property
    def storage(self):
        """``"float32"``, ``"int16"`` (every resident series packed) or ``"mixed"`` (one of state and forcing packed)."""
        packed = [sc is not None for x, sc in ((self.state, self.state_scale), (self.forcing, self.forcing_scale)) if x is not None]
        return "int16" if all(packed) else "mixed" if any(packed) else "float32"

    @property
    def resident_bytes(self):
        """Bytes of HBM the resident series take (the decode tables, time stamps and statistics are not counted)."""
        return sum(x.numel() * x.element_size() for x in (self.state, self.forcing) if x is not None)

    def decoded(self, series="state"):
        """The fp32 series the resident ``series`` (``"state"`` or ``"forcing"``) stands for: ``float32(q) * scale + offset``
        with two fp32 roundings, the kernels' decode; an fp32 series is returned as it is, a missing forcing as None.  A
        FULL-SIZE fp32 allocation (plus a temporary of the same size): for tests and debugging on small datasets only."""
        if series not in ("state", "forcing"):
            raise ValueError(f"series must be 'state' or 'forcing', got {series!r}")
        x, scale, offset = ((self.state, self.state_scale, self.state_offset) if series == "state" else
                            (self.forcing, self.forcing_scale, self.forcing_offset))
        if x is None or scale is None:
            return x
        return torch.add(torch.mul(x.to(torch.float32), scale), offset)   # two launches: the product is rounded before the sum

    def __getitem__(self, idx):
        """One UNSTANDARDISED sample, as the reference's dataset returns it (:479-480)."""
        n = len(self)
        idx = int(idx)
        if idx < 0:
            idx += n
        if not 0 <= idx < n:
            raise IndexError(f"index {idx} out of range for WeatherDataset of length {n}")
        init, target, forcing, times = self.batch(torch.tensor([idx], dtype=torch.int64, device=self.device), standardize=False)
        return init[0], target[0], forcing[0], times[0]

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def check_indices(self, indices):
        """IndexError (as weather_dataset.py:497-503) if any entry of a DEVICE-resident index tensor lies outside
        ``[0, len(self))`` -- ``batch`` does not validate such tensors (the kernel clamps the time index instead of
        faulting, so a bad index would silently repeat boundary time steps).  One host synchronisation: call it once per
        epoch on the permutation, or pass ``validate=True`` to ``batch`` while debugging."""
        idx = torch.as_tensor(indices).reshape(-1)
        if idx.numel():
            lo, hi = int(idx.min()), int(idx.max())
            if lo < 0 or hi >= len(self):
                raise IndexError(f"sample index out of range for WeatherDataset of length {len(self)}: [{lo}, {hi}]")
        return indices

    # ---- the batched launch ----
    def batch(self, indices, standardize=False, out=None, validate=False):
        """(init_states (B, 2, N, d), target_states (B, T, N, d), forcing (B, T, N, F * window), target_times (B, T)).

        ``indices``: a device int64 tensor is used as it is (not validated unless ``validate=True``, which costs a host
        synchronisation: the kernel clamps; see ``check_indices``); anything else is validated on the host like
        ``__getitem__``.  ``out``: optional tuple of four preallocated tensors (e.g. the
        static input buffers of a captured training step)."""
        if not (isinstance(indices, torch.Tensor) and indices.is_cuda):
            host = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
            n = len(self)
            host = torch.where(host < 0, host + n, host)
            if host.numel() and (int(host.min()) < 0 or int(host.max()) >= n):
                raise IndexError(f"sample index out of range for WeatherDataset of length {n}")
            indices = host.to(self.device)
        elif validate:
            self.check_indices(indices)
        indices = indices.to(torch.int64).contiguous()
        B, T = indices.numel(), self.ar_steps
        N, ds = self._nodes, self._d_state
        fw = self.num_forcing_features
        if out is None:
            o = dict(device=self.device, dtype=torch.float32)
            out = (torch.empty((B, 2, N, ds), **o), torch.empty((B, T, N, ds), **o), torch.empty((B, T, N, fw), **o),
                   torch.empty((B, T), device=self.device, dtype=torch.int64))
        init, target, forcing, times = out
        for t_, shape in ((init, (B, 2, N, ds)), (target, (B, T, N, ds)), (forcing, (B, T, N, fw)), (times, (B, T))):
            if tuple(t_.shape) != shape or not t_.is_contiguous() or t_.device != self.state.device:
                raise ValueError(f"output buffer of shape {tuple(t_.shape)}: expected a contiguous {shape} tensor on {self.device}")
        if standardize and self.stats is None:
            raise ValueError("standardize=True needs the standardization statistics (constructor argument)")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.kernel in ("nlam_window_batch_ens", "nlam_window_batch_q16"):
            self._launch_ens(indices, init, target, forcing if fw else None, times, standardize, stream)
            return init, target, forcing, times
        if self.state_scale is not None or self.forcing_scale is not None:
            raise TypeError(f"kernel {self.kernel!r} reads fp32 series: this dataset has storage={self.storage!r} and is cut by "
                            "'nlam_window_batch_q16'")
        if self.kernel != "nlam_window_batch" or self.state.dim() != 3 or self.is_forecast:
            raise ValueError(f"kernel {self.kernel!r}: nlam_window_batch cuts plain analysis series only")
        p = L.Window()
        p.state, p.forcing, p.sample_idx = _ptr(self.state), _ptr(self.forcing), _ptr(indices)
        p.init_states, p.target_states = _ptr(init), _ptr(target)
        p.forcing_windowed = _ptr(forcing) if fw else None
        p.times, p.target_times = _ptr(self.times), _ptr(times)   # times == None: the kernel reports the time index of every target step
        if standardize:
            p.state_mean, p.state_std = _ptr(self.stats["state_mean"]), _ptr(self.stats["state_std"])
            if fw:
                p.forcing_mean, p.forcing_std = _ptr(self.stats["forcing_mean"]), _ptr(self.stats["forcing_std"])
        p.n_times, p.nodes, p.d_state, p.batch = self._n_times, N, ds, B
        p.d_forcing = 0 if self.forcing is None else self.forcing.shape[2]
        p.ar_steps, p.num_past_forcing_steps, p.num_future_forcing_steps = T, self.num_past_forcing_steps, self.num_future_forcing_steps
        L.check(self._lib.nlam_window_batch(C.byref(p), stream), "nlam_window_batch")
        return init, target, forcing, times

    def _launch_ens(self, indices, init, target, forcing, times, standardize, stream):
        """nlam_window_batch_ens over the resident series: strides in elements (floats, or int16 of a packed series) from the
        tensors' own layout.  With a packed series the launch is nlam_window_batch_q16 and that series rides in its own struct."""
        p = L.WindowEns()
        q = None
        if self.state_scale is not None or self.forcing_scale is not None:
            if self.kernel != "nlam_window_batch_q16":
                raise TypeError(f"kernel {self.kernel!r} reads fp32 series: this dataset has storage={self.storage!r} and is cut by "
                                "'nlam_window_batch_q16'")
            q = self.packed_source()
        p.state = None if self.state_scale is not None else _ptr(self.state)
        p.forcing = None if self.forcing_scale is not None else _ptr(self.forcing)
        p.sample_idx = _ptr(indices)
        p.init_states, p.target_states, p.forcing_windowed = _ptr(init), _ptr(target), _ptr(forcing)
        # no time stamps: the kernel reports the time index (analysis) or the lead-time index (forecast) of every target step
        p.times, p.elapsed, p.target_times = _ptr(self.times), _ptr(self.elapsed), _ptr(times)
        if standardize:
            p.state_mean, p.state_std = _ptr(self.stats["state_mean"]), _ptr(self.stats["state_std"])
            if forcing is not None:
                p.forcing_mean, p.forcing_std = _ptr(self.stats["forcing_mean"]), _ptr(self.stats["forcing_std"])

        def strides(x):   # (sample, step, member) strides of a resident series; member stride 0 without a member axis
            if x is None:
                return 0, 0, 0
            lead = 1 if self.is_forecast else 0
            member = x.stride(lead + 1) if x.dim() == 4 + lead else 0
            return x.stride(0), x.stride(lead), member

        p.state_stride_sample, p.state_stride_step, p.state_stride_member = strides(self.state)
        p.forcing_stride_sample, p.forcing_stride_step, p.forcing_stride_member = strides(self.forcing)
        p.n_times, p.is_forecast, p.members = self._n_times, int(self.is_forecast), self.members
        if self.is_forecast:
            p.state_steps = self.state.shape[1]
            p.forcing_steps = 0 if self.forcing is None else self.forcing.shape[1]
        p.nodes, p.d_state, p.batch = self._nodes, self._d_state, indices.numel()
        p.d_forcing = 0 if self.forcing is None else self.forcing.shape[-1]
        p.ar_steps, p.num_past_forcing_steps, p.num_future_forcing_steps = self.ar_steps, self.num_past_forcing_steps, self.num_future_forcing_steps
        if q is not None:
            L.check(self._lib.nlam_window_batch_q16(C.byref(p), C.byref(q), stream), "nlam_window_batch_q16")
            return
        L.check(self._lib.nlam_window_batch_ens(C.byref(p), stream), "nlam_window_batch_ens")

    def packed_source(self):
        """The ``nlam_q16_src_t`` of the resident series: the packed ones with their tables, NULL for an fp32 series."""
        q = L.Q16Src()
        if self.state_scale is not None:
            q.state, q.state_scale, q.state_offset = _ptr(self.state), _ptr(self.state_scale), _ptr(self.state_offset)
        if self.forcing is not None and self.forcing_scale is not None:
            q.forcing, q.forcing_scale, q.forcing_offset = _ptr(self.forcing), _ptr(self.forcing_scale), _ptr(self.forcing_offset)
        return q

    def epoch_permutation(self, seed=0):
        """A resident random permutation of the sample indices: ``perm[k * B : (k + 1) * B]`` feeds ``batch`` with no host copy."""
        g = torch.Generator(device="cpu").manual_seed(int(seed))
        return torch.randperm(len(self), generator=g).to(self.device)
