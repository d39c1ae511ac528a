"""Forecast to any lead time by replaying ONE recorded AR step.

``ARForecaster.forward`` under ``torch.no_grad()`` wants the forcing windows and boundary states of the whole horizon
materialised, records every AR step again when it is captured, and returns standardised, stacked predictions.  ``Forecast``
is the product form: the series stay where ``DeviceWeatherDataset`` keeps them (plain analysis series, or forecast-type and
ensemble layouts read through their strides), a lead counter in device memory ties the data
path to the inference step tail (``nlam_forecast_head`` / ``_tail`` / ``_finish``, include/nlam_hip.h), and one recorded step

    head -> predictor(prev, prev_prev, forcing, raw_delta=True) -> tail -> finish

is replayed ``max_lead`` times.  The graph, the memory besides the output and the host work per lead do not depend on the
horizon, and the horizon does not depend on the rollout length the model was trained with.

    fc = Forecast(step, dataset, max_lead=240, batch_size=2, verify=True)
    res = fc.run(starts)            # ForecastResult of device tensors, no host synchronisation
    res.state                       # (B, L, N, F) physical units
    res.rmse(step.state_std)        # (L, F) per-lead RMSE in physical units (verify=True)

``EnsembleForecast`` is the same engine over ``starts x members``: with a Graph-EFM predictor every lead draws each member's latent
sample on the device (``nlam_latent_sample``, a counter-based generator keyed by a seed and counted by lead, member and start
time), and one more launch per lead scores the ensemble (``nlam_ens_scores``: ensemble-mean error, spread, fair CRPS, rank
histogram, mean and spread fields).

    ens = EnsembleForecast(step, dataset, max_lead=40, members=16, seed=7)
    res = ens.run([0])              # EnsembleResult
    res.members                     # (S, M, L, N, F) physical units;  res.mean, res.spread (S, L, N, F)
    res.crps(step.state_std)        # (L, F) fair CRPS;  res.rmse(...), res.spread_skill(), res.rank_hist

``events`` / ``quantiles`` add one more launch per lead (``nlam_ens_products``): the probability that a variable crosses a
threshold and quantile fields, from the members sorted in registers, with their scores under ``verify``.

    ens = EnsembleForecast(step, dataset, 40, members=16, events=[("t2m", "<", 273.15)], quantiles=[0.1, 0.5, 0.9])
    pr = ens.run([0]).products      # EnsembleProducts: pr.prob (S, L, E, N), pr.quantile (S, L, Q, N, F)
    pr.brier_score(), pr.reliability(), pr.pinball_loss(step.state_std), pr.coverage()

``neighbourhoods`` (with ``events`` and the ``grid_shape`` of the lattice) adds ``nlam_ens_neighbourhood``: per event and window
radius the fraction of (member, cell) pairs in the event around every cell, and with ``verify`` the fractions skill score.

    ens = EnsembleForecast(step, dataset, 40, members=16, events=[("tp", ">", 1e-3)], neighbourhoods=[0, 1, 2, 5, 10],
                           grid_shape=(nx, ny))
    pr = ens.run([0]).products      # pr.nprob (S, L, E, W, N);  pr.fss() (L, E, W)

``spectra`` (with ``grid_shape``, on either engine) adds ``nlam_dct_spectra``: per lead the variance spectrum of the forecast (every
member), the analysis and the ensemble mean from a 2-D discrete cosine transform, binned by total wavenumber.

    fc = Forecast(step, dataset, 40, spectra=["t2m", "u10"], grid_shape=(nx, ny), spectra_window=(10, nx - 10, 10, ny - 10))
    sp = fc.run([0]).spectra        # Spectra: sp.forecast, sp.analysis (B, L, V, nb);  sp.wavenumber, sp.wavelength(2.5)
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib as L


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def plan_forecast(n_times, num_past_forcing_steps, num_future_forcing_steps, max_lead):
    """``(off, n_starts)``: sample ``i`` has its initial states at times ``i + off - 2`` and ``i + off - 1`` (``off = max(2, past)``,
    so ``t0 = i + off - 1``), and the ``n_starts`` valid samples are those whose last forcing window ends inside the series,
    ``t0 + max_lead + future <= n_times - 1`` -- the arithmetic of ``nlam_window_len`` with ``ar_steps = max_lead``.  No GPU."""
    n_times, past, fut, max_lead = int(n_times), int(num_past_forcing_steps), int(num_future_forcing_steps), int(max_lead)
    if n_times < 1 or past < 0 or fut < 0 or max_lead < 1:
        raise ValueError(f"plan_forecast: n_times {n_times} and max_lead {max_lead} must be >= 1, the forcing steps ({past}, {fut}) >= 0")
    off = max(2, past)
    return off, max(0, n_times - (off + max_lead + fut) + 1)


def plan_forecast_dataset(layout, num_past_forcing_steps, num_future_forcing_steps, max_lead, ar_steps):
    """``(off, n_starts, members)`` for a dataset of any layout (``layout``: the ``data.Layout`` of ``plan_layout``).  A start is a
    flat sample index, ``i -> (i // members, i % members)`` as ``DeviceWeatherDataset.batch`` decodes it.  Forecast data (the
    layout keeps lead times): every analysis time of every member is a start, and the horizon is what the dataset keeps resident,
    so ``max_lead > ar_steps`` is a ValueError.  Analysis data: ``plan_forecast`` over the common time axis per member; ``ar_steps``
    is not read.  No GPU."""
    past, fut, max_lead = int(num_past_forcing_steps), int(num_future_forcing_steps), int(max_lead)
    members = int(layout.members)
    if layout.state_steps is None:
        off, per_member = plan_forecast(layout.n_times, past, fut, max_lead)
        return off, per_member * members, members
    off = plan_forecast(layout.n_times, past, fut, max_lead)[0]
    if max_lead > int(ar_steps):
        raise ValueError(f"forecast data keeps the lead times of ar_steps = {int(ar_steps)} resident: max_lead {max_lead} needs a "
                         f"dataset built with ar_steps >= {max_lead}")
    return off, int(layout.n_times) * members, members


def dataset_source(dataset, sample_idx):
    """The ``nlam_forecast_src_t`` of a ``DeviceWeatherDataset``'s resident series: the strides in floats from the tensors' own
    layout, as its ``nlam_window_batch_ens`` launch takes them.  ``sample_idx``: the device int64 tensor of flat sample indices
    the launches read (kept alive by the caller).  A packed series (``storage="int16"``) leaves its float pointer NULL and its
    strides count int16 elements: it rides in ``dataset.packed_source()`` beside this struct, for the ``_q16`` pair."""
    s = L.ForecastSrc()
    s.state = None if getattr(dataset, "state_scale", None) is not None else _ptr(dataset.state)
    s.forcing = None if getattr(dataset, "forcing_scale", None) is not None else _ptr(dataset.forcing)
    s.sample_idx = _ptr(sample_idx)
    lead_ax = 1 if dataset.is_forecast else 0

    def strides(x):   # (sample, step, member); member stride 0 without a member axis
        if x is None:
            return 0, 0, 0
        return x.stride(0), x.stride(lead_ax), (x.stride(lead_ax + 1) if x.dim() == 4 + lead_ax else 0)

    s.state_stride_sample, s.state_stride_step, s.state_stride_member = strides(dataset.state)
    s.forcing_stride_sample, s.forcing_stride_step, s.forcing_stride_member = strides(dataset.forcing)
    s.n_times, s.is_forecast, s.members = int(dataset._n_times), int(dataset.is_forecast), int(dataset.members)
    if dataset.is_forecast:
        s.state_steps = dataset.state.shape[1]
        s.forcing_steps = 0 if dataset.forcing is None else dataset.forcing.shape[1]
    return s


def check_starts(starts, n_starts):
    """Host sample indices as an int64 tensor, negative ones counted from the end; IndexError outside ``[0, n_starts)``."""
    host = torch.as_tensor(starts, dtype=torch.int64).reshape(-1)
    host = torch.where(host < 0, host + n_starts, host)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= n_starts):
        raise IndexError(f"forecast start out of range: {n_starts} valid starts for this series and horizon")
    return host


def dct_basis(n):
    """The orthonormal DCT-II basis ``C[k][i] = beta_k cos(pi k (2 i + 1) / (2 n))``, ``beta_0 = sqrt(1 / n)``, ``beta_k = sqrt(2 / n)``
    (``scipy.fft.dct(norm="ortho")`` of the identity), a float64 ``(n, n)`` tensor.  ``nlam_dct_spectra`` takes it rounded once to
    fp32.  No GPU."""
    import math

    n = int(n)
    if n < 1:
        raise ValueError(f"dct_basis: n {n} must be >= 1")
    k = torch.arange(n, dtype=torch.int64)[:, None]
    i = torch.arange(n, dtype=torch.int64)[None, :]
    turn = (k * (2 * i + 1)) % (4 * n)   # the angle in units of pi / (2 n), reduced in integers: the cosine's argument stays below 2 pi
    basis = torch.cos(turn.to(torch.float64) * (math.pi / (2.0 * n))) * math.sqrt(2.0 / n)
    basis[0] = math.sqrt(1.0 / n)
    return basis


def dct_bins(cx, cy):
    """``(bin_of, bin_ptr, bin_idx, nb)``: the binning of Denis, Cote and Laprise (2002) of the ``cx x cy`` DCT coefficients by total
    normalised wavenumber, ``nb = Nmin = min(cx, cy)`` bins.  With ``k = floor(Nmin sqrt(m^2 / cx^2 + n^2 / cy^2))`` decided in
    integers (``k`` is the largest integer with ``k^2 cx^2 cy^2 <= (m^2 cy^2 + n^2 cx^2) Nmin^2``; no float tie decides a bin),
    coefficient ``(m, n)`` goes to bin ``max(k, 1) - 1`` when ``k <= Nmin - 1`` and to the last bin -- the corner beyond the
    inscribed quarter ellipse -- otherwise; ``(0, 0)``, the mean, goes to -1 (dropped), so the bins of a field add up to its
    variance.  ``bin_of`` (cx * cy) int32 at ``m * cy + n``; ``bin_ptr`` (nb + 1) / ``bin_idx`` int32 the same as a CSR list,
    ascending in ``m * cy + n`` inside a bin: the order ``nlam_dct_spectra`` adds in.  No GPU."""
    import math

    cx, cy = int(cx), int(cy)
    if cx < 2 or cy < 2:
        raise ValueError(f"dct_bins: a window of {cx} x {cy} cells; both sides must be >= 2")
    nmin = min(cx, cy)
    den = cx * cx * cy * cy
    bin_of = []
    for m in range(cx):
        for n in range(cy):
            if m == 0 and n == 0:
                bin_of.append(-1)
                continue
            k = math.isqrt((m * m * cy * cy + n * n * cx * cx) * nmin * nmin // den)
            bin_of.append(max(k, 1) - 1 if k <= nmin - 1 else nmin - 1)
    lists = [[] for _ in range(nmin)]
    for idx, b in enumerate(bin_of):
        if b >= 0:
            lists[b].append(idx)
    ptr = [0]
    for lst in lists:
        ptr.append(ptr[-1] + len(lst))
    i32 = torch.int32
    return (torch.tensor(bin_of, dtype=i32), torch.tensor(ptr, dtype=i32),
            torch.tensor([i for lst in lists for i in lst], dtype=i32), nmin)


def parse_spectra(spectra, grid_shape, window, var_names, n_vars, nodes=None):
    """The host checks of ``Forecast(spectra=..., grid_shape=..., spectra_window=...)``: ``(variables, (nx, ny), (i0, i1, j0, j1))``
    with every variable as its index, or ``([], None, None)`` without ``spectra``.  ``window`` None is the whole grid.  ValueError
    for an unknown variable name or an index out of range, a duplicate, an empty list, a missing grid shape or one that does not
    hold ``nodes`` nodes (when they are known), and a window that is not four integers with ``0 <= i0 < i1 <= nx``,
    ``i1 - i0 >= 2`` and the same in j.  No GPU."""
    if spectra is None:
        return [], None, None
    if isinstance(spectra, (str, bytes)):
        spectra = [spectra]
    variables = []
    for var in spectra:
        if isinstance(var, str):
            if var_names is None or var not in var_names:
                raise ValueError(f"Forecast: unknown state variable {var!r} in spectra (known: {var_names})")
            idx = list(var_names).index(var)
        else:
            try:
                idx = int(var)
            except (TypeError, ValueError):
                idx = -1
            if isinstance(var, bool) or idx != var or not 0 <= idx < n_vars:
                raise ValueError(f"Forecast: spectra variable index {var!r} outside [0, {n_vars})")
        if idx in variables:
            raise ValueError(f"Forecast: state variable {var!r} is listed twice in spectra")
        variables.append(idx)
    if not variables:
        raise ValueError("Forecast: spectra is empty")
    try:
        nx, ny = (int(v) for v in grid_shape)
    except (TypeError, ValueError):
        raise ValueError(f"Forecast: spectra need grid_shape=(nx, ny), got {grid_shape!r}") from None
    if nx < 1 or ny < 1 or (nodes is not None and nx * ny != nodes):
        raise ValueError(f"Forecast: grid_shape {(nx, ny)} does not hold the {nodes} grid nodes")
    if window is None:
        window = (0, nx, 0, ny)
    try:
        win = tuple(int(v) for v in window)
        exact = len(win) == 4 and all(not isinstance(v, bool) and w == v for v, w in zip(window, win))
    except (TypeError, ValueError):
        exact = False
    if not exact:
        raise ValueError(f"Forecast: spectra_window is four integers (i0, i1, j0, j1), got {window!r}")
    i0, i1, j0, j1 = win
    if not (0 <= i0 < i1 <= nx and 0 <= j0 < j1 <= ny) or i1 - i0 < 2 or j1 - j0 < 2:
        raise ValueError(f"Forecast: spectra_window {win} needs 0 <= i0 < i1 <= {nx}, 0 <= j0 < j1 <= {ny} and at least 2 cells "
                         "along each side")
    return variables, (nx, ny), win


class Spectra(NamedTuple):
    """Device tensors of ``nlam_dct_spectra`` for one run, cut to the ``leads`` that ran: the variance of every selected variable
    per wavenumber bin, in physical units squared; the bins of one field add up to its population variance over the window."""
    forecast: torch.Tensor             # (B, leads, V, nb): every batch item (every member, b = s * M + m, of an ensemble)
    analysis: torch.Tensor             # (B, leads, V, nb) (Forecast) or (S, leads, V, nb) (EnsembleForecast)
    mean: Optional[torch.Tensor]       # (S, leads, V, nb) of the ensemble mean, or None
    variables: tuple                   # the state variable index of every v
    wavenumber: torch.Tensor           # (nb) float64, host: k / Nmin of bin k - 1; NaN for the last bin, the corner
    window: tuple                      # (i0, i1, j0, j1)

    def wavelength(self, spacing):
        """(nb) wavelength of every bin in the units of the grid ``spacing``: ``2 * spacing / wavenumber`` (NaN for the corner bin)."""
        return 2.0 * float(spacing) / self.wavenumber


class ForecastResult(NamedTuple):
    """Device tensors of one ``Forecast.run``: ``state`` (B, L, N, F) in physical units, ``std`` (B, L, N, F) the predicted std
    in physical units or None, ``valid_times`` (B, L) int64 (time stamps, or time indices for a dataset without them), ``sq`` /
    ``ab`` (B, L, F) the masked grid means of the squared / absolute error against the analysis in standardised units (the
    ``sq`` / ``ab`` of ``nlam_eval_metrics``), or None without ``verify``."""
    state: torch.Tensor
    std: Optional[torch.Tensor]
    valid_times: torch.Tensor
    sq: Optional[torch.Tensor]
    ab: Optional[torch.Tensor]
    spectra: Optional[Spectra] = None   # Forecast(spectra=...): cut to the leads that ran

    def rmse(self, state_std):
        """(L, F) ``sqrt(mean_b sq) * state_std``: the rescaling of the reference's test epoch (models/module.py)."""
        if self.sq is None:
            raise ValueError("ForecastResult.rmse needs the verification sums: Forecast(..., verify=True)")
        return torch.sqrt(torch.mean(self.sq, dim=0)) * state_std


def _loaded_hip_runtime():
    """The HIP runtime this process already runs on (torch's), for the two graph queries below."""
    with open("/proc/self/maps") as maps:
        paths = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
    if not paths:
        raise RuntimeError("no HIP runtime is loaded in this process")
    return C.CDLL(paths[0])


def _kernel_nodes(graph: "torch.cuda.CUDAGraph") -> int:
    """Kernel nodes of a captured (``keep_graph=True``) graph: hipGraphGetNodes + hipGraphNodeGetType."""
    hip = _loaded_hip_runtime()
    raw = C.c_void_p(graph.raw_cuda_graph())
    n = C.c_size_t(0)
    if hip.hipGraphGetNodes(raw, None, C.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    nodes = (C.c_void_p * max(1, n.value))()
    if hip.hipGraphGetNodes(raw, nodes, C.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    kernels = 0
    for i in range(n.value):
        kind = C.c_int(-1)
        if hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(kind)) != 0:
            raise RuntimeError("hipGraphNodeGetType failed")
        kernels += kind.value == 0   # hipGraphNodeTypeKernel
    return kernels


class Forecast:
    """A forecast engine over a trained ``ForecasterStep`` and a ``DeviceWeatherDataset`` of any layout.

    ``step``: its predictor, boundary mask, interior weights and statistics are used; the predictor must satisfy
    ``can_return_raw_delta()`` or ``can_fuse_ext_tail()`` (GraphLAM, Hi-LAM, Hi-LAM-Parallel, with or without output clamps and a
    predicted std; ValueError otherwise, Graph-EFM included).  ``dataset``: a plain analysis series (``dataset.kernel ==
    "nlam_window_batch"``) is read by ``nlam_forecast_init`` / ``_head``, its ``ar_steps`` is ignored and the horizon is
    ``max_lead``.  A forecast-type or ensemble ``DeviceWeatherDataset`` is read by ``nlam_forecast_init_strided`` / ``_head_strided``
    through the dataset's own strides: a start is a flat sample index, ``i -> (i // members, i % members)`` as ``dataset.batch``
    decodes it; analysis data with members has ``plan_forecast(...)[1] * members`` starts; forecast data has ``len(dataset)`` starts
    and only the lead times of its ``ar_steps`` resident, so ``max_lead > dataset.ar_steps`` is a ValueError (build the dataset with
    ``ar_steps`` = the longest horizon wanted).  Every lead is verified against the dataset's own rows: the state of the start's
    member, the forcing shared or per member as the dataset has it.  Anything else that claims another kernel: ValueError.
    ``verify=True`` also scores every lead against the analysis (``ForecastResult.sq`` / ``ab``).  ``use_graph=False`` issues the
    same launches eagerly.
    ``autocast_dtype``: the predictor call alone runs under ``torch.autocast`` with it.  Weights changed in place between two
    ``run`` calls (a training step, ``load_state_dict``, ``with tr.ema_weights():``) are honoured by the second call: the recorded
    step reads the parameters where they live and the static embeddings are recomputed by every ``run``.
    ``spectra``: state variables (names of ``step.state_var_names`` or indices) whose variance spectrum is wanted per lead, on the
    ``grid_shape = (nx, ny)`` lattice, node ``n = i * ny + j`` as ``graph.py`` numbers it, over ``spectra_window = (i0, i1, j0, j1)``
    (default: the whole grid; pass the interior box so that the boundary rows, where forecast and analysis are the same by
    construction, do not dilute the comparison).  It adds ``nlam_dct_spectra`` between the tail and the finish of the recorded step:
    ``SPECTRA_LAUNCHES`` = 3 launches per lead for every size, ``ForecastResult.spectra`` with the spectra of the forecast and of the
    analysis (``8 B L V nb`` bytes, ``nb = min(cx, cy)``) and ``8 B cx cy V`` bytes of workspace per source.  ``set_spectra_window``
    moves the window without a new recording.  With ``spectra=None`` nothing is allocated or launched."""

    _serves_latent = False
    _defers_spectra = False   # a subclass whose sources do not exist yet when this constructor ends sets the call up itself
    SPECTRA_LAUNCHES = 3   # pass along j, pass along i, bins: for every size, window, variable list and source count

    def __init__(self, step, dataset, max_lead, batch_size=1, verify=False, use_graph=True, autocast_dtype=None, spectra=None,
                 grid_shape=None, spectra_window=None):
        weight = getattr(step, "interior_weight", None)
        self._spec_vars, self._spec_grid, self._spec_window = parse_spectra(
            spectra, grid_shape, spectra_window, getattr(step, "state_var_names", None),
            int(getattr(step, "state_mean", torch.empty(0)).numel()), None if weight is None else int(weight.numel()))
        from .models import ARForecaster

        forecaster = getattr(step, "forecaster", None)
        if not isinstance(forecaster, ARForecaster):
            raise ValueError("Forecast needs a ForecasterStep over an ARForecaster")
        predictor = forecaster.predictor
        raw = getattr(predictor, "can_return_raw_delta", lambda: False)()
        ext = getattr(predictor, "can_fuse_ext_tail", lambda: False)()
        if getattr(predictor, "draws_latent", False) and not self._serves_latent:
            raw = ext = False   # a predictor that samples: EnsembleForecast
        if not (raw or ext):
            raise ValueError(f"Forecast: {type(predictor).__name__} cannot hand its raw network output to the forecast tail (it needs "
                             "can_return_raw_delta() or can_fuse_ext_tail(): a graph model with a per-variable diff_std, and "
                             "NLAM_FUSED_CLAMPED_TAIL on for output clamps or a predicted std; Graph-EFM is not served)")
        from .data import DeviceWeatherDataset

        packed = isinstance(dataset, DeviceWeatherDataset) and dataset.storage != "float32"
        strided = isinstance(dataset, DeviceWeatherDataset) and (packed or dataset.kernel == "nlam_window_batch_ens")
        if packed and dataset.kernel != "nlam_window_batch_q16":
            raise TypeError(f"Forecast: dataset.kernel {dataset.kernel!r} reads fp32 series, but the dataset has storage="
                            f"{dataset.storage!r} (its kernel is 'nlam_window_batch_q16')")
        if not strided and getattr(dataset, "kernel", None) != "nlam_window_batch":
            raise ValueError("Forecast reads a DeviceWeatherDataset (any layout) or plain analysis series (dataset.kernel == "
                             "'nlam_window_batch'): other forecast-type and ensemble datasets are not served")
        self.max_lead, self.batch_size = int(max_lead), int(batch_size)
        if self.max_lead < 1 or self.batch_size < 1:
            raise ValueError(f"Forecast: max_lead {max_lead} and batch_size {batch_size} must be >= 1")
        dev = getattr(getattr(dataset, "state", None), "device", dataset.device)   # with its index: "cuda" names the current device
        if dev.type != "cuda" or any(p.device != dev for p in predictor.parameters()) or step.state_mean.device != dev:
            raise RuntimeError(f"Forecast runs on the GPU that holds the dataset ({dev}): move the step there (there is no CPU fallback)")
        if not packed and any(x is not None and x.dtype != torch.float32 for x in (getattr(dataset, "state", None),
                                                                                   getattr(dataset, "forcing", None))):
            raise TypeError("Forecast: the plain and strided entries read fp32 series; packed int16 series come from a "
                            "DeviceWeatherDataset built with storage='int16' or from data.PackedSeries")
        self.step, self.dataset, self.predictor = step, dataset, predictor
        self.verify, self.use_graph, self.autocast_dtype = bool(verify), bool(use_graph), autocast_dtype
        self.past, self.future = dataset.num_past_forcing_steps, dataset.num_future_forcing_steps
        self.n_times = int(dataset._n_times)
        self.strided = strided
        if strided:
            self.off, self.n_starts, self.data_members = plan_forecast_dataset(dataset.layout, self.past, self.future, self.max_lead,
                                                                               dataset.ar_steps)
        else:
            self.off, self.n_starts = plan_forecast(self.n_times, self.past, self.future, self.max_lead)
            self.data_members = 1
        B, Lm = self.batch_size, self.max_lead
        N, F = int(dataset.state.shape[-2]), int(dataset.state.shape[-1])
        dfo = 0 if dataset.forcing is None else int(dataset.forcing.shape[-1])
        if N != predictor.num_grid_nodes or F != step.state_mean.numel() or (dfo > 0 and step.forcing_mean is None):
            raise ValueError(f"Forecast: the dataset's series ({N} nodes, {F} state and {dfo} forcing variables) do not fit the step")
        self.has_std = bool(predictor.output_std)
        if self.verify and F > L.EVAL_MAX_VARS:
            raise ValueError(f"Forecast(verify=True): at most {L.EVAL_MAX_VARS} state variables, got {F}")
        self._lib = L.load()
        f32 = dict(device=dev, dtype=torch.float32)
        self.start = torch.zeros((B,), device=dev, dtype=torch.int64)
        self.lead = torch.zeros((1,), device=dev, dtype=torch.int32)
        self.prev, self.prev_prev = torch.zeros((B, N, F), **f32), torch.zeros((B, N, F), **f32)
        self.truth = torch.zeros((B, N, F), **f32)
        self.forcing = torch.zeros((B, N, dfo * (self.past + self.future + 1)), **f32)
        self.out_state = torch.empty((B, Lm, N, F), **f32)
        self.out_std = torch.empty((B, Lm, N, F), **f32) if self.has_std else None
        self.valid_times = torch.zeros((B, Lm), device=dev, dtype=torch.int64)
        self.sq = self.ab = self.workspace = None
        if self.verify:
            self.sq, self.ab = torch.zeros((B, Lm, F), **f32), torch.zeros((B, Lm, F), **f32)
            self.workspace = torch.empty((int(self._lib.nlam_forecast_workspace_floats(B, N, F)),), **f32)
        self._bmask = forecaster.boundary_mask.reshape(-1).contiguous()
        self._clamp = predictor.clamp_tables()
        p = L.Forecast()
        p.state, p.forcing, p.times = _ptr(dataset.state), _ptr(dataset.forcing), _ptr(dataset.times)
        p.start, p.lead = _ptr(self.start), _ptr(self.lead)
        p.state_mean, p.state_std = _ptr(step.state_mean), _ptr(step.state_std)
        if dfo > 0:
            p.forcing_mean, p.forcing_std = _ptr(step.forcing_mean), _ptr(step.forcing_std)
            p.forcing_windowed = _ptr(self.forcing)
        p.prev, p.prev_prev, p.truth = _ptr(self.prev), _ptr(self.prev_prev), _ptr(self.truth)
        p.dstd, p.dmean = _ptr(predictor.diff_std), _ptr(predictor.diff_mean)
        p.bmask, p.row_weight = _ptr(self._bmask), _ptr(step.interior_weight)
        if self._clamp is not None:
            p.clamp_mode_host, p.clamp_lo, p.clamp_hi = C.addressof(self._clamp.mode), _ptr(self._clamp.lo), _ptr(self._clamp.hi)
        p.out_state, p.out_std, p.valid_times = _ptr(self.out_state), _ptr(self.out_std), _ptr(self.valid_times)
        p.sq, p.ab, p.workspace = _ptr(self.sq), _ptr(self.ab), _ptr(self.workspace)
        p.workspace_floats = 0 if self.workspace is None else self.workspace.numel()
        p.n_times, p.nodes, p.d_state, p.d_forcing, p.batch = self.n_times, N, F, dfo, B
        p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps = Lm, self.past, self.future
        p.delta_ld = 2 * F if self.has_std else F
        self._p = p
        self._src = self._packed = None
        if packed:
            # every layout of a packed dataset, the plain one included, goes through the strided pair with the decode in flight;
            # p.state / p.forcing only satisfy the tail's argument check (no launch reads a series through them)
            self._packed = dataset.packed_source()
        if strided:
            # the head and init read the series through the dataset's own strides (they ignore p.state / p.forcing / p.start, which
            # the tail's argument check still wants); the tail's valid-time arithmetic is a plain series': computed per run (_replay)
            p.times = p.valid_times = None
            self._src = dataset_source(dataset, self.start)
        self._static = None     # persistent copies of the predictor's static embeddings: the recorded step reads these
        self._graph = None
        self._delta = None      # the recorded step's network output (kept alive with the graph)
        self._launches = None
        self._sp = None
        if self._spec_vars and not self._defers_spectra:
            parse_spectra(self._spec_vars, self._spec_grid, self._spec_window, None, F, N)
            self._init_spectra(self._spectra_sources())

    # ---- variance spectra ----
    def _spectra_sources(self):
        """``(name, tensor, batch, batch stride, lead stride, physical)`` of every source of the ``nlam_dct_spectra`` call."""
        B, per = self.batch_size, self._p.nodes * self._p.d_state
        return [("forecast", self.prev, B, per, 0, 0), ("analysis", self.truth, B, per, 0, 0)]

    def _init_spectra(self, sources):
        """The tables, outputs and argument struct of ``nlam_dct_spectra`` (only with ``spectra``)."""
        (nx, ny), (i0, i1, j0, j1) = self._spec_grid, self._spec_window
        cx, cy, V, Lm = i1 - i0, j1 - j0, len(self._spec_vars), self.max_lead
        dev = self.start.device
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        _, bin_ptr, bin_idx, nb = dct_bins(cx, cy)
        self.spec_basis_x, self.spec_basis_y = dct_basis(cx).to(**f32), dct_basis(cy).to(**f32)   # float64, rounded once
        self.spec_bin_ptr, self.spec_bin_idx = bin_ptr.to(dev), bin_idx.to(dev)
        self.spec_var = torch.tensor(self._spec_vars, **i32)
        self.spec_origin = torch.tensor([i0, j0], **i32)
        items = sum(src[2] for src in sources)
        nws = int(self._lib.nlam_dct_spectra_workspace_floats(items, cx, cy, V))
        if nws < 0 or len(sources) > L.SPEC_MAX_SOURCES:
            raise ValueError(f"Forecast: nlam_dct_spectra does not serve these sizes ({nws})")
        self.spectra_workspace = torch.empty((nws,), **f32)
        self.spec_out = {}
        sp = L.DctSpectra()
        for k, (name, t, batch, batch_stride, lead_stride, physical) in enumerate(sources):
            self.spec_out[name] = torch.zeros((batch, Lm, V, nb), **f32)
            q = sp.src[k]
            q.x, q.spec = t.data_ptr(), self.spec_out[name].data_ptr()
            q.batch_stride, q.lead_stride, q.batch, q.physical = batch_stride, lead_stride, batch, physical
        sp.origin, sp.basis_x, sp.basis_y = _ptr(self.spec_origin), _ptr(self.spec_basis_x), _ptr(self.spec_basis_y)
        sp.var, sp.bin_ptr, sp.bin_idx = _ptr(self.spec_var), _ptr(self.spec_bin_ptr), _ptr(self.spec_bin_idx)
        sp.state_std, sp.lead = _ptr(self.step.state_std), _ptr(self.lead)
        sp.workspace, sp.workspace_floats = _ptr(self.spectra_workspace), nws
        sp.sources, sp.nx, sp.ny, sp.d_state = len(sources), nx, ny, self._p.d_state
        sp.vars, sp.bins, sp.bin_entries, sp.max_lead = V, nb, int(bin_idx.numel()), Lm
        sp.cx, sp.cy = cx, cy
        wn = torch.arange(1, nb + 1, dtype=torch.float64) / nb
        wn[-1] = float("nan")
        self._spec_wavenumber = wn
        self._sp = sp

    def set_spectra_window(self, window):
        """A new window ``(i0, i1, j0, j1)`` of the same ``cx x cy`` cells for the following runs: the origin the launches read is
        rewritten in device memory (the bases and the bins depend on ``cx`` and ``cy`` alone).  No new recording, like
        ``set_thresholds``; a window that changes ``cx`` or ``cy`` is a ValueError (it would change the launches)."""
        if self._sp is None:
            raise ValueError("Forecast.set_spectra_window: the engine was built without spectra")
        _, _, win = parse_spectra(self._spec_vars, self._spec_grid, window, None, self._p.d_state)
        if (win[1] - win[0], win[3] - win[2]) != (self._sp.cx, self._sp.cy):
            raise ValueError(f"Forecast.set_spectra_window: {win} is {win[1] - win[0]} x {win[3] - win[2]} cells, the recorded "
                             f"step takes {self._sp.cx} x {self._sp.cy}")
        self.spec_origin.copy_(torch.tensor([win[0], win[2]], dtype=torch.int32))
        self._spec_window = win

    def _launch_spectra(self):
        from .ops import _stream

        if self._sp is not None:
            L.check(self._lib.nlam_dct_spectra(C.byref(self._sp), _stream()), "nlam_dct_spectra")

    def _spectra_result(self, leads):
        if self._sp is None:
            return None
        out = {name: t.narrow(1, 0, leads) for name, t in self.spec_out.items()}
        return Spectra(out["forecast"], out["analysis"], out.get("mean"), tuple(self._spec_vars), self._spec_wavenumber,
                       tuple(self._spec_window))

    # ---- one lead time ----
    def _entry(self, name):
        from .ops import _stream

        if self._src is not None and name in ("nlam_forecast_init", "nlam_forecast_head"):
            if self._packed is not None:
                name += "_q16"
                L.check(getattr(self._lib, name)(C.byref(self._p), C.byref(self._src), C.byref(self._packed), _stream()), name)
                return
            name += "_strided"
            L.check(getattr(self._lib, name)(C.byref(self._p), C.byref(self._src), _stream()), name)
            return
        L.check(getattr(self._lib, name)(C.byref(self._p), _stream()), name)

    def _autocast(self):
        return (torch.autocast(device_type="cuda", dtype=self.autocast_dtype) if self.autocast_dtype is not None
                else contextlib.nullcontext())

    def _network(self):
        """The predictor's raw output for the current lead."""
        with self._autocast():
            delta, _ = self.predictor(self.prev, self.prev_prev, self.forcing, raw_delta=True)
        return delta

    def _after_tail(self):
        """Launches between the tail and the finish of a lead: ``nlam_dct_spectra`` with ``spectra``, else none."""
        self._launch_spectra()

    def _one_lead(self):
        """head -> predictor -> tail -> finish on the current stream; every launch reads the lead counter on the device."""
        self._entry("nlam_forecast_head")
        delta = self._network().float().contiguous()
        if tuple(delta.shape) != (self.batch_size, self._p.nodes, self._p.delta_ld):
            raise RuntimeError(f"Forecast: the predictor returned {tuple(delta.shape)}")
        self._p.delta = _ptr(delta)
        self._entry("nlam_forecast_tail")
        self._after_tail()
        self._entry("nlam_forecast_finish")
        return delta

    @contextlib.contextmanager
    def _static_installed(self):
        """The predictor reads the persistent static embeddings (``BaseGraphModel._static``, as inside ``static_cache``)."""
        old = self.predictor._static
        self.predictor._static = self._static
        try:
            yield
        finally:
            self.predictor._static = old

    def _refresh_static(self):
        """The static embeddings from the CURRENT weights into the buffers the recorded step reads."""
        new = self.predictor.compute_static_embeddings()
        if self._static is None:
            self._static = {k: [t.clone() for t in v] if isinstance(v, (list, tuple)) else v.clone() for k, v in new.items()}
            return
        for k, v in new.items():
            if isinstance(v, (list, tuple)):
                for dst, src in zip(self._static[k], v):
                    dst.copy_(src)
            else:
                self._static[k].copy_(v)

    def _record(self):
        """Warm the step up (two eager leads on a side stream), then record it once."""
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(2):
                self._one_lead()
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(graph):
            self._delta = self._one_lead()
        self._launches = _kernel_nodes(graph)
        graph.instantiate()
        self._graph = graph

    @property
    def launches_per_lead(self):
        """Kernel nodes of the recorded step (it is recorded on first use); None with ``use_graph=False``.  ``spectra`` adds
        ``SPECTRA_LAUNCHES`` = 3 to it, for every size."""
        if not self.use_graph:
            return None
        if self._graph is None:
            with torch.no_grad():
                self._refresh_static()
                with self._static_installed():
                    self._record()
        return self._launches

    # ---- the forecast ----
    def run(self, starts, leads=None):
        """Forecast ``leads`` (default and at most ``max_lead``) steps ahead from the dataset samples ``starts`` (``batch_size``
        of them, the indices ``dataset.batch`` takes; host indices are validated: IndexError; a device int64 tensor is used
        as it is).  No host synchronisation.  The result's tensors are the engine's buffers: the next ``run`` overwrites them,
        and with ``leads < max_lead`` the slots from ``leads`` on are unspecified."""
        leads = self.max_lead if leads is None else int(leads)
        if not 1 <= leads <= self.max_lead:
            raise ValueError(f"Forecast.run: leads {leads} outside [1, {self.max_lead}]")
        if not (isinstance(starts, torch.Tensor) and starts.is_cuda):
            starts = check_starts(starts, self.n_starts).to(self.dataset.device)
        starts = starts.to(torch.int64).reshape(-1)
        if starts.numel() != self.batch_size:
            raise ValueError(f"Forecast.run: {starts.numel()} starts for batch_size {self.batch_size}")
        self._replay(starts, leads)
        return ForecastResult(self.out_state, self.out_std, self.valid_times, self.sq, self.ab, self._spectra_result(leads))

    def _dataset_times(self, starts):
        """``valid_times`` of a strided dataset, the ``target_times`` of ``dataset.batch``: ``times[s + off + k]`` (analysis data),
        ``times[s] + elapsed[off + k]`` (forecast data), the time / lead-time index without stamps.  On the device, once per run,
        with the kernels' clamp of the flat index."""
        ds, M = self.dataset, self.data_members
        s = torch.clamp(starts, 0, max(self.n_starts, M) - 1) // M
        rows = torch.arange(self.off, self.off + self.max_lead, device=starts.device)
        if ds.is_forecast:
            vt = rows.expand(s.numel(), -1) if ds.times is None else ds.times[s][:, None] + ds.elapsed[rows][None]
        else:
            vt = torch.clamp(s[:, None] + rows, max=self.n_times - 1)
            if ds.times is not None:
                vt = ds.times[vt]
        self.valid_times.copy_(vt)

    def _replay(self, starts, leads):
        """``leads`` leads from the device sample indices ``starts`` (one per batch item) into the engine's buffers."""
        with torch.no_grad():
            self._refresh_static()
            with self._static_installed():
                if self.use_graph and self._graph is None:
                    self._record()
                if self.strided:
                    self.start.copy_(starts)   # the flat sample index: the kernels split it into (sample, member)
                    self._dataset_times(starts)
                else:
                    torch.add(starts, self.off - 1, out=self.start)   # t0 of every forecast
                self._entry("nlam_forecast_init")
                for _ in range(leads):
                    if self.use_graph:
                        self._graph.replay()
                    else:
                        self._one_lead()


class EnsembleProducts(NamedTuple):
    """Device tensors of ``nlam_ens_products`` for one ``EnsembleForecast.run``, cut to the ``leads`` that ran.  ``prob`` /
    the event scores are None without ``events``, ``quantile`` / the quantile scores without ``quantiles``, all scores without
    ``verify``.  Sums are in standardised units, the quantile fields in physical units."""
    prob: Optional[torch.Tensor]        # (S, leads, E, N) fraction of the members in the event
    quantile: Optional[torch.Tensor]    # (S, leads, Q, N, F) linear-interpolation quantiles of the members
    brier: Optional[torch.Tensor]       # (S, leads, E) sum_n w_n (prob - o)^2
    rel_count: Optional[torch.Tensor]   # (S, leads, E, M + 1) int32: live nodes with c members in the event
    rel_obs: Optional[torch.Tensor]     # (S, leads, E, M + 1) int32: those of them where the truth is in it
    pinball: Optional[torch.Tensor]     # (S, leads, Q, F) sum_n w_n rho_q(y - Q_q)
    below: Optional[torch.Tensor]       # (S, leads, Q, F) int32: live nodes with the truth below the quantile
    events: tuple                       # ((variable index, ">" or "<", threshold in physical units), ...)
    levels: tuple                       # the quantile levels
    n_members: int
    n_live: int                         # nodes with a non-zero weight
    nprob: Optional[torch.Tensor] = None     # (S, leads, E, W, N) fraction of the (member, live cell) pairs of the window in the event
    fbs: Optional[torch.Tensor] = None       # (S, leads, E, W) sum_n w_n (nprob - observed fraction)^2
    fbs_ref: Optional[torch.Tensor] = None   # (S, leads, E, W) sum_n w_n (nprob^2 + observed fraction^2)
    radii: tuple = ()                        # the window radii in cells (``neighbourhoods``)

    def _scores(self, t, what):
        if t is None:
            raise ValueError(f"EnsembleProducts: {what} needs EnsembleForecast(..., verify=True) and the products it scores")
        return t

    def brier_score(self):
        """(leads, E) Brier score of every event: the mean over the starts of ``brier``."""
        return torch.mean(self._scores(self.brier, "brier_score"), dim=0)

    def reliability(self):
        """``(forecast probability (M + 1), observed frequency (leads, E, M + 1), counts (leads, E, M + 1))`` summed over the
        starts: of the live nodes forecast ``c / M``, the fraction where the event happened (NaN for an empty bin)."""
        count = self._scores(self.rel_count, "reliability").sum(0)
        obs = self.rel_obs.sum(0)
        fc = torch.arange(self.n_members + 1, device=count.device, dtype=torch.float32) / self.n_members
        return fc, obs.to(torch.float32) / count.to(torch.float32), count

    def pinball_loss(self, state_std):
        """(leads, Q, F) pinball (quantile) loss in physical units: ``mean_s pinball * state_std``."""
        return torch.mean(self._scores(self.pinball, "pinball_loss"), dim=0) * state_std

    def coverage(self):
        """(leads, Q, F) fraction of the live nodes, over all starts, whose truth lies below the quantile: ``q`` when calibrated."""
        below = self._scores(self.below, "coverage")
        return below.sum(0).to(torch.float32) / float(below.shape[0] * self.n_live)

    def fss(self):
        """(leads, E, W) fractions skill score of every event and window radius over all starts: ``1 - sum_s fbs / sum_s fbs_ref``,
        in [0, 1], NaN where no live window holds a member or a truth in the event."""
        ref = self._scores(self.fbs_ref, "fss").sum(0)
        return 1.0 - self.fbs.sum(0) / ref


def quantile_tables(levels, members):
    """``(index, frac)`` of ``nlam_ens_products_t.q_index`` / ``q_frac``: ``i = floor(q (M - 1))``, ``g = q (M - 1) - i`` in float64."""
    import math

    pos = [float(q) * (int(members) - 1) for q in levels]
    idx = [min(int(math.floor(v)), int(members) - 1) for v in pos]
    return idx, [v - i for v, i in zip(pos, idx)]


def parse_products(events, quantiles, var_names, n_vars):
    """The host checks of ``EnsembleForecast(events=..., quantiles=...)``: ``(events, levels)`` with every event as ``(variable
    index, 0 for ">" or 1 for "<", threshold)``.  ValueError for an unknown variable, a bad sense, a level outside [0, 1] and
    more than ``NLAM_ENS_MAX_EVENTS`` / ``NLAM_ENS_MAX_QUANTILES`` of them.  No GPU."""
    ev, levels = [], []
    for item in (events or ()):
        try:
            var, sense, thr = item
        except (TypeError, ValueError):
            raise ValueError(f"EnsembleForecast: an event is (variable, '>' or '<', threshold), got {item!r}") from None
        if isinstance(var, str):
            if var_names is None or var not in var_names:
                raise ValueError(f"EnsembleForecast: unknown state variable {var!r} in an event (known: {var_names})")
            idx = list(var_names).index(var)
        else:
            try:
                idx = int(var)
            except (TypeError, ValueError):
                idx = -1
            if isinstance(var, bool) or idx != var or not 0 <= idx < n_vars:
                raise ValueError(f"EnsembleForecast: event variable index {var!r} outside [0, {n_vars})")
        if sense not in (">", "<"):
            raise ValueError(f"EnsembleForecast: an event's sense is '>' or '<', got {sense!r}")
        thr = float(thr)
        if thr != thr:
            raise ValueError("EnsembleForecast: an event's threshold is NaN")
        ev.append((idx, 0 if sense == ">" else 1, thr))
    for q in (quantiles or ()):
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"EnsembleForecast: quantile level {q} outside [0, 1]")
        levels.append(q)
    if len(ev) > L.ENS_MAX_EVENTS:
        raise ValueError(f"EnsembleForecast: at most {L.ENS_MAX_EVENTS} events, got {len(ev)}")
    if len(levels) > L.ENS_MAX_QUANTILES:
        raise ValueError(f"EnsembleForecast: at most {L.ENS_MAX_QUANTILES} quantile levels, got {len(levels)}")
    return ev, levels


def parse_neighbourhoods(neighbourhoods, grid_shape, n_events, members, nodes=None):
    """The host checks of ``EnsembleForecast(neighbourhoods=..., grid_shape=...)``: ``(radii, (nx, ny))``, or ``([], None)`` without
    ``neighbourhoods``.  ValueError for radii without events, a missing grid shape or one that does not hold ``nodes`` nodes (when
    they are known), a radius that is negative or no integer, more than ``NLAM_NBR_MAX_SCALES`` radii, and ``members * nodes`` above
    2^24 (the window sums must stay integers a float holds).  No GPU."""
    if neighbourhoods is None:
        return [], None
    radii = []
    for r in neighbourhoods:
        try:
            ri = int(r)
        except (TypeError, ValueError):
            ri = -1
        if isinstance(r, bool) or ri != r or ri < 0:
            raise ValueError(f"EnsembleForecast: a neighbourhood radius is a non-negative integer number of cells, got {r!r}")
        radii.append(min(ri, 2 ** 31 - 1))
    if not radii:
        raise ValueError("EnsembleForecast: neighbourhoods is empty")
    if not n_events:
        raise ValueError("EnsembleForecast: neighbourhoods are those of the events: give events=[...] too")
    if len(radii) > L.NBR_MAX_SCALES:
        raise ValueError(f"EnsembleForecast: at most {L.NBR_MAX_SCALES} neighbourhood radii, got {len(radii)}")
    try:
        nx, ny = (int(v) for v in grid_shape)
    except (TypeError, ValueError):
        raise ValueError(f"EnsembleForecast: neighbourhoods need grid_shape=(nx, ny), got {grid_shape!r}") from None
    if nx < 1 or ny < 1 or (nodes is not None and nx * ny != nodes):
        raise ValueError(f"EnsembleForecast: grid_shape {(nx, ny)} does not hold the {nodes} grid nodes")
    if members * nx * ny > 2 ** 24:
        raise ValueError(f"EnsembleForecast: neighbourhoods need members * nodes <= 2^24, got {members} * {nx * ny}")
    return radii, (nx, ny)


class EnsembleResult(NamedTuple):
    """Device tensors of one ``EnsembleForecast.run`` (the engine's buffers, cut to the ``leads`` that ran; batch item
    ``b = s * M + m``).  The raw fields are those of ``ForecastResult`` over the ``S * M`` batch plus the ensemble launch's; the
    accessors below give them their ensemble shapes.  Sums are in standardised units, fields in physical units."""
    state: torch.Tensor
    out_std: Optional[torch.Tensor]
    times: torch.Tensor
    sq: Optional[torch.Tensor]
    ab: Optional[torch.Tensor]
    mean: torch.Tensor                 # (S, leads, N, F) ensemble mean
    spread: torch.Tensor               # (S, leads, N, F) sqrt of the unbiased member variance
    ens_sq: Optional[torch.Tensor]     # (S, leads, F) sum_n w_n (xbar - y)^2
    ens_var: Optional[torch.Tensor]    # (S, leads, F) sum_n w_n * unbiased member variance
    ens_abs: Optional[torch.Tensor]    # (S, leads, F) sum_n w_n / M sum_m |x_m - y|
    ens_pair: Optional[torch.Tensor]   # (S, leads, F) sum_n w_n / (M (M - 1)) sum_{i<j} |x_i - x_j|
    rank_hist: Optional[torch.Tensor]  # (S, leads, F, M + 1) int32
    noise: Optional[torch.Tensor]      # (leads, S * M, R, latent_dim) the standard-normal draws (record_noise / latent_noise)
    n_members: int
    products: Optional[EnsembleProducts] = None   # EnsembleForecast(events=..., quantiles=...)
    spectra: Optional[Spectra] = None             # EnsembleForecast(spectra=...)

    def _per_member(self, t):
        return None if t is None else t.view(t.shape[0] // self.n_members, self.n_members, *t.shape[1:])

    @property
    def members(self):
        """(S, M, leads, N, F) member fields."""
        return self._per_member(self.state)

    @property
    def std(self):
        """(S, M, leads, N, F) predicted std of a std head, or None."""
        return self._per_member(self.out_std)

    @property
    def valid_times(self):
        """(S, leads)."""
        return self._per_member(self.times)[:, 0]

    @property
    def member_sq(self):
        """(S, M, leads, F): ``ForecastResult.sq`` of every member."""
        return self._per_member(self.sq)

    @property
    def member_ab(self):
        return self._per_member(self.ab)

    def _scores(self):
        if self.ens_sq is None:
            raise ValueError("EnsembleResult: the scores need EnsembleForecast(..., verify=True)")

    def rmse(self, state_std):
        """(leads, F) RMSE of the ensemble mean in physical units: ``sqrt(mean_s ens_sq) * state_std``."""
        self._scores()
        return torch.sqrt(torch.mean(self.ens_sq, dim=0)) * state_std

    def crps(self, state_std):
        """(leads, F) fair CRPS in physical units: ``mean_s (ens_abs - ens_pair) * state_std``."""
        self._scores()
        return torch.mean(self.ens_abs - self.ens_pair, dim=0) * state_std

    def spread_skill(self):
        """(leads, F) ``sqrt((M + 1) / M * mean_s ens_var) / sqrt(mean_s ens_sq)``: 1 for a calibrated ensemble."""
        self._scores()
        M = self.n_members
        return torch.sqrt((M + 1) / M * torch.mean(self.ens_var, dim=0)) / torch.sqrt(torch.mean(self.ens_sq, dim=0))


class EnsembleForecast(Forecast):
    """``members`` forecasts from each of ``n_starts`` initial times, as ONE recorded step over the batch ``n_starts * members``:

        head -> embed + prior parameters -> nlam_latent_sample -> decoder -> tail -> nlam_ens_scores [-> nlam_ens_products
             [-> nlam_ens_neighbourhood]] -> finish

    replayed per lead.  The predictor is a Graph-EFM (``GraphEFM``, ``GraphEFMMultiScale``; ``can_return_raw_delta()``): every
    lead draws a new latent sample per member from Philox4x32-10 keyed by ``seed`` and counted by (lead, member, start time),
    so the forecast of ``(seed, start, member)`` has the same bits with and without the graph, from run to run and whatever
    other starts share the batch.  A deterministic predictor (whatever ``Forecast`` takes) is accepted too, without the sampling
    launch: its members are identical by construction (the baseline of the ensemble launch's cost).
    On a forecast-type or ensemble dataset (``Forecast``'s rules) all ``members`` model members of a start begin from the same
    dataset sample ``(s, m_data)``, and the "start" word of the Philox counter is the flat sample index, not the time index ``t0``
    of a plain series: the guarantee above holds per dataset, but the same weather read from a plain series draws other noise.
    ``verify``: the per-member sums of ``Forecast`` and the ensemble scores; the mean and spread fields are always written.
    ``record_noise``: keep every lead's draws (``EnsembleResult.noise``).  Members are always kept: the member fields take
    ``4 S M L N F`` bytes (twice that with a std head), mean and spread ``8 S L N F``.
    ``events``: ``(variable, sense, threshold)`` triples -- a state variable name of the datastore (``step.state_var_names``) or its
    index, ``">"`` or ``"<"`` (equality never counts), a threshold in physical units -- and ``quantiles``: levels in [0, 1].  Either
    adds ``nlam_ens_products`` after ``nlam_ens_scores`` in the recorded step (``EnsembleResult.products``: ``4 S L N (E + Q F)``
    bytes of fields; their scores with ``verify``).  Thresholds live in a device table in standardised units, ``(thr - mean) / std``
    computed in float64: ``set_thresholds`` rewrites it without a new recording.  With neither, nothing is allocated or launched.
    ``neighbourhoods``: window radii in cells (at most 8) on the ``grid_shape = (nx, ny)`` lattice, node ``n = i * ny + j`` as
    ``graph.py`` numbers it; it needs ``events`` and ``members * nodes <= 2^24``.  It adds ``nlam_ens_neighbourhood`` behind
    ``nlam_ens_products`` (5 launches per lead with ``verify``, 4 without, for every size): ``products.nprob`` takes ``4 S L E W N``
    bytes, ``fbs`` / ``fbs_ref`` / ``fss()`` come with ``verify``.  The radii live in a device table (``set_radii``), and the event
    tables are shared, so ``set_thresholds`` moves both launches.  With ``neighbourhoods=None`` nothing is allocated or launched.
    ``spectra`` / ``spectra_window``: as in ``Forecast`` (``grid_shape`` is the one ``neighbourhoods`` use).  ``nlam_dct_spectra`` goes
    last before the finish, 3 launches per lead for every size, over three sources: every member, the analysis of every start and
    the ensemble mean that ``nlam_ens_scores`` has just written (``EnsembleResult.spectra.forecast`` (S M, L, V, nb), ``.analysis``
    and ``.mean`` (S, L, V, nb))."""

    _serves_latent = True
    _defers_spectra = True    # the mean slots come after Forecast.__init__

    def __init__(self, step, dataset, max_lead, members, n_starts=1, seed=0, verify=True, use_graph=True, autocast_dtype=None,
                 record_noise=False, events=None, quantiles=None, neighbourhoods=None, grid_shape=None, spectra=None,
                 spectra_window=None):
        members, n_starts = int(members), int(n_starts)
        if not 1 <= members <= L.ENS_MAX_MEMBERS:
            raise ValueError(f"EnsembleForecast: members {members} outside [1, {L.ENS_MAX_MEMBERS}]")
        if n_starts < 1:
            raise ValueError(f"EnsembleForecast: n_starts {n_starts} must be >= 1")
        self._events, self._levels = parse_products(events, quantiles, getattr(step, "state_var_names", None),
                                                    int(getattr(step, "state_mean", torch.empty(0)).numel()))
        weight = getattr(step, "interior_weight", None)
        self._radii, self._grid = parse_neighbourhoods(neighbourhoods, grid_shape, len(self._events), members,
                                                       None if weight is None else int(weight.numel()))
        super().__init__(step, dataset, max_lead, batch_size=n_starts * members, verify=verify, use_graph=use_graph,
                         autocast_dtype=autocast_dtype, spectra=spectra, grid_shape=grid_shape, spectra_window=spectra_window)
        S, M, B, Lm = n_starts, members, n_starts * members, self.max_lead
        N, F = self._p.nodes, self._p.d_state
        if F > L.EVAL_MAX_VARS:
            raise ValueError(f"EnsembleForecast: at most {L.EVAL_MAX_VARS} state variables, got {F}")
        self.members, self.starts_per_run, self.record_noise = M, S, bool(record_noise)
        dev = self.start.device
        f32 = dict(device=dev, dtype=torch.float32)
        self.mean, self.spread = torch.empty((S, Lm, N, F), **f32), torch.empty((S, Lm, N, F), **f32)
        self.ens_sq, self.ens_var, self.ens_abs, self.ens_pair = (torch.zeros((S, Lm, F), **f32) for _ in range(4))
        self.rank_hist = torch.zeros((S, Lm, F, M + 1), device=dev, dtype=torch.int32)
        self.ens_workspace = torch.empty((int(self._lib.nlam_ens_scores_workspace_floats(S, M, N, F)),), **f32)
        e = L.EnsScores()
        e.prev, e.truth, e.row_weight = _ptr(self.prev), _ptr(self.truth), _ptr(step.interior_weight)
        e.state_mean, e.state_std, e.lead = _ptr(step.state_mean), _ptr(step.state_std), _ptr(self.lead)
        e.ens_sq, e.ens_var, e.ens_abs, e.ens_pair = (_ptr(t) for t in (self.ens_sq, self.ens_var, self.ens_abs, self.ens_pair))
        e.rank_hist, e.out_mean, e.out_spread = _ptr(self.rank_hist), _ptr(self.mean), _ptr(self.spread)
        e.workspace, e.workspace_floats = _ptr(self.ens_workspace), self.ens_workspace.numel()
        e.starts, e.members, e.nodes, e.d_state, e.max_lead = S, M, N, F, Lm
        self._e = e
        self.samples = bool(getattr(self.predictor, "draws_latent", False))
        self.noise = self.latent = self.seed = None
        self._given = False      # which of the two recordings is installed: noise drawn on the device / read from self.noise
        self._recorded = {}
        if self.samples:
            R, D = int(self.predictor.latent_spatial_dim), int(self.predictor.latent_dim)
            self.latent = torch.zeros((B, R, D), **f32)
            self.seed = torch.zeros((1,), device=dev, dtype=torch.int64)
            self._set_seed(seed)
            if self.record_noise:
                self.noise = torch.zeros((Lm, B, R, D), **f32)
            s = L.LatentSample()
            s.latent, s.start, s.lead, s.seed = _ptr(self.latent), _ptr(self.start), _ptr(self.lead), _ptr(self.seed)
            s.noise_out = _ptr(self.noise)
            s.batch, s.members, s.rows, s.latent_dim, s.max_lead = B, M, R, D, Lm
            s.diagonal = int(self.predictor.prior_model.output_dist == "diagonal")
            self._s = s
        self._kept = None   # the recorded step's prior parameters (kept alive with the graph, like its network output)
        self._pr = None
        if self._events or self._levels:
            self._init_products()
        self._nb = None
        if self._radii:
            parse_neighbourhoods(self._radii, self._grid, len(self._events), M, N)
            self._init_neighbourhoods()
        if self._spec_vars:
            parse_spectra(self._spec_vars, self._spec_grid, self._spec_window, None, F, N)
            self._init_spectra(self._spectra_sources())

    def _spectra_sources(self):
        """Every member, member 0's analysis row of every start, and this lead's slot of the ensemble mean (physical units)."""
        S, M, Lm, per = self.starts_per_run, self.members, self.max_lead, self._p.nodes * self._p.d_state
        return [("forecast", self.prev, S * M, per, 0, 0), ("analysis", self.truth, S, M * per, 0, 0),
                ("mean", self.mean, S, Lm * per, per, 1)]

    def _init_products(self):
        """The tables, outputs and argument struct of ``nlam_ens_products`` (only with ``events`` or ``quantiles``)."""
        e, step = self._e, self.step
        S, M, N, F, Lm = e.starts, e.members, e.nodes, e.d_state, e.max_lead
        E, Q = len(self._events), len(self._levels)
        dev = self.start.device
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        self._mean64, self._std64 = step.state_mean.detach().cpu().double(), step.state_std.detach().cpu().double()
        self.n_live = int((step.interior_weight != 0).sum())
        p = L.EnsProducts()
        p.prev, p.row_weight, p.state_mean, p.state_std, p.lead = e.prev, e.row_weight, e.state_mean, e.state_std, e.lead
        p.truth = e.truth if self.verify else None
        self.prob = self.quantile = self.brier = self.rel_count = self.rel_obs = self.pinball = self.below = None
        if E:
            self.event_var = torch.tensor([v for v, _, _ in self._events], **i32)
            self.event_sense = torch.tensor([sn for _, sn, _ in self._events], **i32)
            self.event_thr = torch.zeros((E,), **f32)
            self.set_thresholds([t for _, _, t in self._events])
            self.prob = torch.empty((S, Lm, E, N), **f32)
            p.event_var, p.event_sense, p.event_thr, p.prob = (_ptr(t) for t in (self.event_var, self.event_sense, self.event_thr, self.prob))
            if self.verify:
                self.brier = torch.zeros((S, Lm, E), **f32)
                self.rel_count, self.rel_obs = torch.zeros((S, Lm, E, M + 1), **i32), torch.zeros((S, Lm, E, M + 1), **i32)
                p.brier, p.rel_count, p.rel_obs = _ptr(self.brier), _ptr(self.rel_count), _ptr(self.rel_obs)
        if Q:
            idx, frac = quantile_tables(self._levels, M)
            self.q_index = torch.tensor(idx, **i32)
            self.q_frac = torch.tensor(frac, dtype=torch.float64).to(**f32)
            self.q_level = torch.tensor(self._levels, dtype=torch.float64).to(**f32)
            self.quantile = torch.empty((S, Lm, Q, N, F), **f32)
            p.q_index, p.q_frac, p.q_level, p.quant = (_ptr(t) for t in (self.q_index, self.q_frac, self.q_level, self.quantile))
            if self.verify:
                self.pinball = torch.zeros((S, Lm, Q, F), **f32)
                self.below = torch.zeros((S, Lm, Q, F), **i32)
                p.pinball, p.below = _ptr(self.pinball), _ptr(self.below)
        self.products_workspace = torch.empty((int(self._lib.nlam_ens_products_workspace_floats(S, M, N, F, E, Q)),), **f32)
        p.workspace, p.workspace_floats = _ptr(self.products_workspace), self.products_workspace.numel()
        p.starts, p.members, p.nodes, p.d_state, p.max_lead, p.events, p.quantiles = S, M, N, F, Lm, E, Q
        self._pr = p

    def _init_neighbourhoods(self):
        """The radius table, outputs and argument struct of ``nlam_ens_neighbourhood`` (only with ``neighbourhoods``)."""
        pr = self._pr
        S, M, F, Lm, E, W = pr.starts, pr.members, pr.d_state, pr.max_lead, pr.events, len(self._radii)
        (nx, ny), N = self._grid, pr.nodes
        dev = self.start.device
        f32 = dict(device=dev, dtype=torch.float32)
        self.radius = torch.zeros((W,), device=dev, dtype=torch.int32)
        self.set_radii(self._radii)
        self.nprob = torch.empty((S, Lm, E, W, N), **f32)
        self.fbs = self.fbs_ref = None
        nb = L.EnsNeighbourhood()
        nb.prev, nb.truth, nb.row_weight, nb.lead = pr.prev, pr.truth, pr.row_weight, pr.lead
        nb.event_var, nb.event_sense, nb.event_thr = pr.event_var, pr.event_sense, pr.event_thr
        nb.radius, nb.nprob = _ptr(self.radius), _ptr(self.nprob)
        if self.verify:
            self.fbs, self.fbs_ref = torch.zeros((S, Lm, E, W), **f32), torch.zeros((S, Lm, E, W), **f32)
            nb.fbs, nb.fbs_ref = _ptr(self.fbs), _ptr(self.fbs_ref)
        nws = int(self._lib.nlam_ens_neighbourhood_workspace_floats(S, M, nx, ny, F, E, W))
        if nws < 0:
            raise ValueError(f"EnsembleForecast: nlam_ens_neighbourhood does not serve these sizes ({nws})")
        self.neighbourhood_workspace = torch.empty((nws,), **f32)
        nb.workspace, nb.workspace_floats = _ptr(self.neighbourhood_workspace), nws
        nb.starts, nb.members, nb.nx, nb.ny, nb.d_state, nb.max_lead, nb.events, nb.scales = S, M, nx, ny, F, Lm, E, W
        self._nb = nb

    def set_radii(self, values):
        """New window radii (cells, one per entry of ``neighbourhoods``) for the following runs: the device table is rewritten in
        place.  No new recording, like ``set_thresholds``."""
        values = list(values)
        if len(values) != len(self._radii) or not values:
            raise ValueError(f"EnsembleForecast.set_radii: {len(values)} radii for {len(self._radii)} neighbourhoods")
        radii, _ = parse_neighbourhoods(values, self._grid, len(self._events), self.members)
        self.radius.copy_(torch.tensor(radii, dtype=torch.int32))
        self._radii = radii

    def set_thresholds(self, values):
        """New thresholds (physical units, one per event, in the order of ``events``) for the following runs: the device table
        is rewritten in place, ``(thr - state_mean) / state_std`` in float64 rounded to fp32.  No new recording, like ``run(seed=...)``."""
        values = [float(v) for v in values]
        if len(values) != len(self._events) or not values:
            raise ValueError(f"EnsembleForecast.set_thresholds: {len(values)} thresholds for {len(self._events)} events")
        if any(v != v for v in values):
            raise ValueError("EnsembleForecast.set_thresholds: a threshold is NaN")
        var = torch.tensor([v for v, _, _ in self._events], dtype=torch.int64)
        std = (torch.tensor(values, dtype=torch.float64) - self._mean64[var]) / self._std64[var]
        self.event_thr.copy_(std.to(torch.float32))
        self._events = [(v, sn, t) for (v, sn, _), t in zip(self._events, values)]

    def _set_seed(self, seed):
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.seed.fill_(seed - (1 << 64) if seed >= (1 << 63) else seed)   # the 64 bits, in the int64 the device word is kept as

    def _network(self):
        if not self.samples:
            return super()._network()
        from .ops import _stream

        pred, s = self.predictor, self._s
        with self._autocast():
            grid_emb, graph_emb = pred.embedd_grid_and_graph(self.prev, self.prev_prev, self.forcing)
            params = pred.prior_params(grid_emb, graph_emb)
        params = params.float().contiguous()
        if tuple(params.shape) != (s.batch, s.rows, s.latent_dim * (2 if s.diagonal else 1)):
            raise RuntimeError(f"EnsembleForecast: the prior returned parameters of shape {tuple(params.shape)}")
        s.params = _ptr(params)
        L.check(self._lib.nlam_latent_sample(C.byref(s), _stream()), "nlam_latent_sample")
        self._kept = params
        with self._autocast():
            return pred.decoder(grid_emb, self.latent, graph_emb, raw=True)

    def _after_tail(self):
        from .ops import _stream

        L.check(self._lib.nlam_ens_scores(C.byref(self._e), _stream()), "nlam_ens_scores")
        if self._pr is not None:
            L.check(self._lib.nlam_ens_products(C.byref(self._pr), _stream()), "nlam_ens_products")
        if self._nb is not None:
            L.check(self._lib.nlam_ens_neighbourhood(C.byref(self._nb), _stream()), "nlam_ens_neighbourhood")
        self._launch_spectra()

    def _install(self, given):
        """Install the recording that draws the noise (``given`` False) or reads it from ``self.noise`` (True)."""
        if given and self.noise is None:
            self.noise = torch.zeros((self.max_lead, *self.latent.shape), device=self.latent.device, dtype=torch.float32)
        if given != self._given:
            self._recorded[self._given] = (self._graph, self._delta, self._launches, self._kept)
            self._graph, self._delta, self._launches, self._kept = self._recorded.pop(given, (None, None, None, None))
            self._given = given
        self._s.noise_in = _ptr(self.noise) if given else None
        self._s.noise_out = None if given or not self.record_noise else _ptr(self.noise)

    def run(self, starts, leads=None, seed=None, latent_noise=None):
        """``leads`` leads (default and at most ``max_lead``) from the dataset samples ``starts`` (``n_starts`` of them, as
        ``Forecast.run`` takes them), every one as ``members`` forecasts.  ``seed``: a new 64-bit seed (kept for later runs; no new
        recording).  ``latent_noise`` (leads, n_starts * members, R, latent_dim): the standard-normal noise to use in place of
        the generator's.  No host synchronisation; the result's tensors are the engine's buffers."""
        leads = self.max_lead if leads is None else int(leads)
        if not 1 <= leads <= self.max_lead:
            raise ValueError(f"EnsembleForecast.run: leads {leads} outside [1, {self.max_lead}]")
        if not (isinstance(starts, torch.Tensor) and starts.is_cuda):
            starts = check_starts(starts, self.n_starts).to(self.dataset.device)
        starts = starts.to(torch.int64).reshape(-1)
        if starts.numel() != self.starts_per_run:
            raise ValueError(f"EnsembleForecast.run: {starts.numel()} starts for n_starts {self.starts_per_run}")
        if latent_noise is not None:
            if not self.samples:
                raise ValueError("EnsembleForecast.run: latent_noise for a predictor that draws none")
            if tuple(latent_noise.shape) != (leads, *self.latent.shape):
                raise ValueError(f"EnsembleForecast.run: latent_noise of shape {tuple(latent_noise.shape)}, expected "
                                 f"{(leads, *self.latent.shape)}")
            if not latent_noise.is_cuda:
                raise RuntimeError("EnsembleForecast.run: latent_noise must be on the GPU (there is no CPU fallback)")
        if self.samples:
            self._install(latent_noise is not None)
            if latent_noise is not None:
                self.noise[:leads].copy_(latent_noise)
            if seed is not None:
                self._set_seed(seed)
        self._replay(starts.repeat_interleave(self.members), leads)
        cut = lambda t, dim=1: None if t is None else t.narrow(dim, 0, leads)   # noqa: E731
        scores = (self.ens_sq, self.ens_var, self.ens_abs, self.ens_pair, self.rank_hist) if self.verify else (None,) * 5
        noise = self.noise if self.samples and (self.record_noise or latent_noise is not None) else None
        products = None
        if self._pr is not None:
            fields = (self.prob, self.quantile, self.brier, self.rel_count, self.rel_obs, self.pinball, self.below)
            products = EnsembleProducts(*(cut(t) for t in fields), tuple((v, "<" if sn else ">", t) for v, sn, t in self._events),
                                        tuple(self._levels), self.members, self.n_live)
            if self._nb is not None:
                products = products._replace(nprob=cut(self.nprob), fbs=cut(self.fbs), fbs_ref=cut(self.fbs_ref), radii=tuple(self._radii))
        return EnsembleResult(cut(self.out_state), cut(self.out_std), cut(self.valid_times), cut(self.sq), cut(self.ab),
                              cut(self.mean), cut(self.spread), *(cut(t) for t in scores), cut(noise, 0), self.members, products,
                              self._spectra_result(leads))
