"""Standardization statistics of a dataset on the device data path.

Counterpart of the reference's ``neural_lam/datastore/npyfilesmeps/compute_standardization_stats.py``: that script runs a
CPU DataLoader over ``WeatherDataset(split="train", ar_steps=63, num_past_forcing_steps=0, num_future_forcing_steps=0)``
twice (values, then standardized one-step differences) and writes ``parameter_mean.pt``, ``parameter_std.pt``,
``diff_mean.pt``, ``diff_std.pt`` and ``flux_stats.pt`` into the store's ``static`` directory.  Here both passes read the
series that ``DeviceWeatherDataset`` keeps in HBM in place (``nlam_window_moments``: per-sample means and second moments,
fp64 sums in a fixed order), the per-sample rows are combined on the device in float64, and one copy brings the result to
the host.  ``save_standardization_stats`` / ``load_standardization_stats`` write and read the reference's files, and
``SyntheticDatastore(state_stats=..., forcing_stats=...)`` hands them to the models.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import NamedTuple

import torch

from . import _lib as L
from .data import plan_layout

# the reference store's file names (npyfilesmeps/store.py get_standardization_dataarray)
STATE_FILES = {
    "state_mean": "parameter_mean.pt",
    "state_std": "parameter_std.pt",
    "state_diff_mean_standardized": "diff_mean.pt",
    "state_diff_std_standardized": "diff_std.pt",
}
FLUX_FILE = "flux_stats.pt"


class StatsLayout(NamedTuple):
    """What ``plan_statistics`` reads of a dataset: its length and window arguments and its feature counts."""
    length: int                     # len(dataset): samples x members
    ar_steps: int
    num_past_forcing_steps: int
    num_future_forcing_steps: int
    d_state: int
    d_forcing: int                  # 0 without forcing


class StatsPlan(NamedTuple):
    n_samples: int                  # per-sample rows of the values pass
    diff_rows_per_sample: int       # rows of the difference pass per sample: one per sub-offset (= step_length)
    pairs: int                      # consecutive pairs differenced in one of those rows
    flux_batches: tuple             # (begin, end) sample ranges of the reference's flux batches


def stats_layout(state_shape, forcing_shape=None, *, is_forecast=False, ar_steps=63, num_past_forcing_steps=0,
                 num_future_forcing_steps=0, load_single_member=False) -> StatsLayout:
    """``StatsLayout`` of the ``DeviceWeatherDataset`` these shapes and arguments would make (host only, no device)."""
    lay = plan_layout(state_shape, forcing_shape, is_forecast=is_forecast, ar_steps=ar_steps,
                      num_past_forcing_steps=num_past_forcing_steps, num_future_forcing_steps=num_future_forcing_steps,
                      load_single_member=load_single_member)
    d_forcing = 0 if forcing_shape is None else int(tuple(forcing_shape)[-1])
    return StatsLayout(length=lay.length, ar_steps=int(ar_steps), num_past_forcing_steps=int(num_past_forcing_steps),
                       num_future_forcing_steps=int(num_future_forcing_steps), d_state=int(tuple(state_shape)[-1]),
                       d_forcing=d_forcing)


def _layout_of(dataset) -> StatsLayout:
    return StatsLayout(length=len(dataset), ar_steps=dataset.ar_steps, num_past_forcing_steps=dataset.num_past_forcing_steps,
                       num_future_forcing_steps=dataset.num_future_forcing_steps, d_state=int(dataset.state.shape[-1]),
                       d_forcing=0 if dataset.forcing is None else int(dataset.forcing.shape[-1]))


def plan_statistics(layout: StatsLayout, *, step_length=3, flux_index=0, batch_size=32) -> StatsPlan:
    """Host-side checks of a statistics run (no GPU); ValueError for what the reference's script would not compute or
    the kernel cannot: forcing windows other than 0 / 0, ``step_length < 1`` or no consecutive pair of
    ``step_length``-spaced rows among the ``ar_steps + 2`` of a sample, ``flux_index`` outside the forcing features,
    ``batch_size < 1``, more than ``MOMENTS_MAX_VARS`` features, an empty dataset."""
    if layout.num_past_forcing_steps != 0 or layout.num_future_forcing_steps != 0:
        raise ValueError("standardization statistics read the dataset with num_past_forcing_steps = "
                         "num_future_forcing_steps = 0 (as compute_standardization_stats.py does); got "
                         f"{layout.num_past_forcing_steps} / {layout.num_future_forcing_steps}")
    step, rows = int(step_length), layout.ar_steps + 2
    if step < 1:
        raise ValueError(f"step_length must be >= 1, got {step}")
    if rows // step < 2:
        raise ValueError(f"step_length {step} leaves no consecutive pair to difference among the {rows} rows "
                         f"(ar_steps + 2) of a sample")
    if layout.d_forcing > 0 and not 0 <= int(flux_index) < layout.d_forcing:
        raise ValueError(f"flux_index {flux_index} outside the {layout.d_forcing} forcing features")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    for what, d in (("state", layout.d_state), ("forcing", layout.d_forcing)):
        if d > L.MOMENTS_MAX_VARS:
            raise ValueError(f"{d} {what} features: the statistics kernel takes at most {L.MOMENTS_MAX_VARS}")
    n = int(layout.length)
    if n < 1:
        raise ValueError("the dataset has no samples")
    bs = int(batch_size)
    return StatsPlan(n_samples=n, diff_rows_per_sample=step, pairs=rows // step - 1,
                     flux_batches=tuple((b, min(n, b + bs)) for b in range(0, n, bs)))


def _decode_tables(ds, x):
    """(scale, offset) of resident series ``x`` of ``ds`` when it is packed int16, None for an fp32 series; TypeError for
    anything else (the moments kernels read fp32, or int16 with the dataset's own tables)."""
    if x.dtype == torch.float32:
        return None
    for series, scale, offset in ((getattr(ds, "state", None), getattr(ds, "state_scale", None), getattr(ds, "state_offset", None)),
                                  (getattr(ds, "forcing", None), getattr(ds, "forcing_scale", None),
                                   getattr(ds, "forcing_offset", None))):
        if x is series and x.dtype == torch.int16 and scale is not None:
            return scale, offset
    raise TypeError(f"the moments kernels read an fp32 series, or a packed int16 series of the dataset itself (storage="
                    f"{getattr(ds, 'storage', 'float32')!r}); got a {x.dtype} tensor")


def _moments(ds, x, first, count, row_begin, nrows, step=0, mean=None, std=None):
    """nlam_window_moments over samples [first, first + count) of resident series ``x`` of dataset ``ds``: two fresh
    float64 device tensors (count * max(step, 1), F), per-row means and second moments.  A packed series (``ds.state`` /
    ``ds.forcing`` of a ``storage="int16"`` dataset) goes through nlam_window_moments_q16 with the dataset's decode tables."""
    tables = _decode_tables(ds, x)
    S, F = max(step, 1), int(x.shape[-1])
    o = dict(device=ds.device, dtype=torch.float64)
    out_mean, out_sq = torch.empty((count * S, F), **o), torch.empty((count * S, F), **o)
    if count == 0:
        return out_mean, out_sq
    lib = L.load()
    nodes = int(x.shape[-2])
    n_ws = int(lib.nlam_moments_workspace_doubles(nodes, F, count, step))
    if n_ws < 0:
        raise ValueError(f"nlam_moments_workspace_doubles rejected nodes={nodes}, nvars={F}, count={count}, step={step}")
    ws = torch.empty(n_ws, **o)
    lead = 1 if ds.is_forecast else 0
    p = L.Moments()
    p.series = C.c_void_p(x.data_ptr()) if tables is None else None
    p.workspace = C.c_void_p(ws.data_ptr())
    p.out_mean, p.out_sq = C.c_void_p(out_mean.data_ptr()), C.c_void_p(out_sq.data_ptr())
    if step:
        p.mean, p.std = C.c_void_p(mean.data_ptr()), C.c_void_p(std.data_ptr())
    p.workspace_doubles = n_ws
    # (sample, step, member) strides in elements, as DeviceWeatherDataset._launch_ens; member stride 0 without a member axis
    p.stride_sample, p.stride_step = x.stride(0), x.stride(lead)
    p.stride_member = x.stride(lead + 1) if x.dim() == 4 + lead else 0
    p.n_times, p.first, p.count = ds.layout.n_times, first, count
    p.is_forecast, p.members = int(ds.is_forecast), ds.members
    p.steps = x.shape[1] if ds.is_forecast else 0
    p.nodes, p.nvars, p.row_begin, p.nrows, p.step = nodes, F, row_begin, nrows, step
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    if tables is not None:
        L.check(lib.nlam_window_moments_q16(C.byref(p), C.c_void_p(x.data_ptr()), C.c_void_p(tables[0].data_ptr()),
                                            C.c_void_p(tables[1].data_ptr()), stream), "nlam_window_moments_q16")
        return out_mean, out_sq
    L.check(lib.nlam_window_moments(C.byref(p), stream), "nlam_window_moments")
    return out_mean, out_sq


def _rank_world(group):
    import torch.distributed as dist

    if group is None and not (dist.is_available() and dist.is_initialized()):
        return 0, 1
    return dist.get_rank(group), dist.get_world_size(group)


def _gather(rows, world, group, dev):
    """All ranks' per-sample rows in sample order (each rank holds a contiguous slice, in rank order): CPU tensors through
    all_gather_object, which gloo and RCCL both carry, then fresh device tensors."""
    if world == 1:
        return rows
    import torch.distributed as dist

    got = [None] * world
    dist.all_gather_object(got, tuple(r.cpu() for r in rows), group=group)
    return tuple(torch.cat([g[k] for g in got]).to(dev) for k in range(len(rows)))


def _mean_std(m, q):
    """The estimator of save_stats: mean of the per-row means, sqrt(mean of the second moments - mean^2), in float64;
    a negative difference (round-off on a constant field, where the reference's fp32 formula gives NaN) is clamped to 0."""
    mean = m.sum(0) / m.shape[0]
    second = q.sum(0) / q.shape[0]
    return mean, (second - mean * mean).clamp_min(0.0).sqrt()


def compute_standardization_stats(dataset, *, step_length=3, flux_index=0, batch_size=32, group=None):
    """The statistics ``compute_standardization_stats.py`` writes, computed from a ``DeviceWeatherDataset``.

    The dataset must be built with ``num_past_forcing_steps = num_future_forcing_steps = 0``.  The reference uses
    ``ar_steps=63`` (the 65 lead times of a MEPS forecast); any ``ar_steps`` is accepted here (short series in tests).
    ``step_length`` counts dataset steps: on MEPS's hourly lead times it is the reference's ``--step_length`` in hours.
    Returns fp32 CPU tensors:
      ``state_mean``, ``state_std``                 (d_state,)  values of the ``ar_steps + 2`` state rows of every sample
      ``state_diff_mean_standardized``, ``state_diff_std_standardized``  (d_state,)  differences of consecutive
          ``step_length``-spaced rows (every sub-offset), standardized with the fp32 ``state_mean`` / ``state_std``
      ``flux_stats``                                (2,) with forcing: forcing feature ``flux_index``, mean and std
      ``forcing_mean``, ``forcing_std``             (d_forcing,) with forcing: every forcing feature with the same
          estimator -- beyond the reference's files, whose store fixes all but the flux to 0 / 1.
    Estimator (single-process reference): the mean is the mean of the per-sample means, the std is
    sqrt(mean of the per-sample second moments - mean^2), clamped at 0 where round-off makes the difference negative
    (the reference's fp32 formula gives NaN for a constant field).  Members count as samples, as ``WeatherDataset``
    counts them (``load_single_member`` through the dataset).  The flux keeps the reference's quirk: the mean over
    batches of ``batch_size`` consecutive samples of each batch's mean, so a short last batch weighs like a full one.
    Per-sample sums are fp64 in a fixed order; the combination is float64 on the device; no host synchronisation inside
    a pass and one copy to the host at the end.

    ``group`` (or an initialised default group) with world > 1: every rank reads a contiguous slice of the samples, the
    per-sample rows are all-gathered and every rank combines them in sample order -- the result is bit-identical to one
    rank.  The reference's padding of the last rank (``PaddedWeatherDataset``) and its ``[:n_original_windows]`` slice
    are deliberately not reproduced: no sample is counted twice."""
    lay = _layout_of(dataset)
    plan = plan_statistics(lay, step_length=step_length, flux_index=flux_index, batch_size=batch_size)
    rank, world = _rank_world(group)
    n, dev, ar = plan.n_samples, dataset.device, lay.ar_steps
    first = n * rank // world
    count = n * (rank + 1) // world - first
    has_forcing = lay.d_forcing > 0

    # values: the ar_steps + 2 state rows; the forcing rows of the ar_steps target steps (window 1: j = 2 ... ar_steps + 1)
    rows = _moments(dataset, dataset.state, first, count, 0, ar + 2)
    if has_forcing:
        rows = rows + _moments(dataset, dataset.forcing, first, count, 2, ar)
    rows = _gather(rows, world, group, dev)
    mean64, std64 = _mean_std(rows[0], rows[1])
    state_mean, state_std = mean64.float(), std64.float()   # what the reference saves and reloads for the second pass
    out = [state_mean, state_std]

    diff = _moments(dataset, dataset.state, first, count, 0, ar + 2, step=plan.diff_rows_per_sample, mean=state_mean,
                    std=state_std)
    diff = _gather(diff, world, group, dev)
    out += [t.float() for t in _mean_std(*diff)]

    if has_forcing:
        out += [t.float() for t in _mean_std(rows[2], rows[3])]
        nb, bs = len(plan.flux_batches), int(batch_size)
        counts = torch.full((nb,), float(bs), device=dev, dtype=torch.float64)
        counts[-1] = float(n - (nb - 1) * bs)
        flux = []
        for col in (rows[2][:, flux_index], rows[3][:, flux_index]):   # per-sample flux mean / second moment
            padded = torch.zeros(nb * bs, device=dev, dtype=torch.float64)
            padded[:n] = col
            flux.append((padded.view(nb, bs).sum(1) / counts).sum() / nb)   # mean over batches of the batch means
        fm, fsq = flux
        out += [torch.stack((fm, (fsq - fm * fm).clamp_min(0.0).sqrt())).float()]

    host = torch.cat(out).cpu()
    ds_, df = lay.d_state, lay.d_forcing
    keys = ["state_mean", "state_std", "state_diff_mean_standardized", "state_diff_std_standardized"]
    sizes = [ds_] * 4
    if has_forcing:
        keys += ["forcing_mean", "forcing_std", "flux_stats"]
        sizes += [df, df, 2]
    return dict(zip(keys, (t.clone() for t in torch.split(host, sizes))))


def save_standardization_stats(static_dir, stats):
    """Write the reference store's files into ``static_dir`` (created if missing): ``parameter_mean.pt``,
    ``parameter_std.pt``, ``diff_mean.pt``, ``diff_std.pt`` as fp32 (d_state,) and, when ``stats`` has it,
    ``flux_stats.pt`` as fp32 (2,) -- CPU tensors through ``torch.save``, as compute_standardization_stats.py saves them."""
    d = Path(static_dir)
    d.mkdir(parents=True, exist_ok=True)
    for key, name in STATE_FILES.items():
        torch.save(torch.as_tensor(stats[key], dtype=torch.float32).detach().cpu().reshape(-1).clone(), d / name)
    if stats.get("flux_stats") is not None:
        flux = torch.as_tensor(stats["flux_stats"], dtype=torch.float32).detach().cpu().reshape(-1).clone()
        if flux.numel() != 2:
            raise ValueError(f"flux_stats must hold (mean, std), got {flux.numel()} values")
        torch.save(flux, d / FLUX_FILE)


def load_standardization_stats(static_dir, num_forcing):
    """Read the files back as the reference's ``npyfilesmeps`` store does (store.py get_standardization_dataarray):
    the four state statistics, and for ``num_forcing > 0`` the forcing statistics ``[flux_mean, 0, ...]`` /
    ``[flux_std, 1, ...]`` from ``flux_stats.pt``.  fp32 CPU tensors keyed as ``SyntheticDatastore(state_stats=...,
    forcing_stats=...)`` and ``compute_standardization_stats`` key them (``flux_stats`` included with forcing)."""
    d = Path(static_dir)

    def load(name):
        return torch.load(d / name, weights_only=True).to(torch.float32).reshape(-1)

    out = {key: load(name) for key, name in STATE_FILES.items()}
    nf = int(num_forcing)
    if nf > 0:
        flux = load(FLUX_FILE)
        mean, std = torch.zeros(nf), torch.ones(nf)
        mean[0], std[0] = flux[0], flux[1]
        out.update(forcing_mean=mean, forcing_std=std, flux_stats=flux)
    return out
