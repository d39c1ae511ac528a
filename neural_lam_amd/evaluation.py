"""The epoch-end half of evaluation: what ``ForecasterModule.aggregate_and_plot_metrics`` (models/module.py:923-993) and
``on_test_epoch_end`` (:994-1071) log, plus the epoch means of ``_log_step_loss`` (:512-544), computed from the
``EvalResult`` objects of ``ForecasterStep.evaluate`` / ``trainer.graphed_eval_step`` -- without plots, files or loggers.

    agg = MetricAggregator(datastore, prefix="test", steps_to_log=(1, 3))
    for batch in loader:
        agg.update(step.evaluate(*batch, phase="test", steps_to_log=(1, 3)))
    logs = agg.compute()     # {"test_mean_loss": ..., "test_loss_unroll1": ..., "test_rmse": (T, F), "test_mae": (T, F), ...}
"""
from __future__ import annotations

import torch

# per-sample tensors of an EvalResult and the metric name they are logged under (module.py:228-236, :576, :630, :651)
_PER_SAMPLE = (("entry_mse", "mse"), ("entry_mae", "mae"), ("output_std", "output_std"))


def _all_gather_cat(t):
    """module.py:419-440: the per-sample tensors of every rank, concatenated along dim 0 (equal shapes on every rank, as
    Lightning's all_gather needs); the tensor itself outside ``torch.distributed``."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return t
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t.contiguous())
    return torch.cat(parts, dim=0)


def _all_reduce_sum(t):
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = t.clone()
        dist.all_reduce(t)
    return t


class MetricAggregator:
    """Epoch aggregation of one evaluation phase.

    ``source``: the datastore (its state ``state_std`` and state variable names are read) or a (F,) ``state_std``;
    ``var_names``: the state variable names (needed with a ``state_std`` and ``metrics_watch``); ``prefix``: "val" or "test";
    ``steps_to_log``: ``val_steps_to_log``; ``metrics_watch`` / ``var_leads_metrics_watch``: as in train_model.py:380-390
    (``{var_index: [lead steps]}``).

    ``update(result)`` keeps the loss sums weighted by the batch size and clones the per-sample tensors (a graphed step's
    outputs are overwritten by its next call).  ``compute()`` returns, on every rank:
      ``{prefix}_mean_loss``, ``{prefix}_loss_unroll{k}``   batch-size-weighted epoch means (Lightning's on_epoch=True,
                                                             sync_dist=True, batch_size=B)
      ``{prefix}_rmse`` (T, F)                              sqrt of the per-sample mean of entry_mse, times state_std
      ``test_mae``, ``test_output_std`` (T, F)              per-sample means times state_std (when the results had them)
      ``test_mean_spatial_loss`` (S, N)                     nanmean over samples of the loss maps
      ``{prefix}_{metric}_{var_name}_step_{step}``          scalars of the metrics named in metrics_watch (module.py:905-921)
    Under an initialised ``torch.distributed`` the per-sample tensors are all-gathered and the loss sums all-reduced first."""

    def __init__(self, source, var_names=None, prefix="val", steps_to_log=(1,), metrics_watch=(), var_leads_metrics_watch=None):
        if isinstance(source, torch.Tensor) or not hasattr(source, "get_standardization_dataarray"):
            state_std = torch.as_tensor(source, dtype=torch.float32).reshape(-1)
        else:
            state_std = torch.tensor(source.get_standardization_dataarray("state").state_std.values, dtype=torch.float32)
            if var_names is None:
                var_names = list(source.get_vars_names(category="state"))
        self.state_std = state_std
        self.var_names = None if var_names is None else list(var_names)
        self.prefix = prefix
        self.steps_to_log = tuple(int(k) for k in steps_to_log)
        self.metrics_watch = tuple(metrics_watch)
        self.var_leads_metrics_watch = {int(k): list(v) for k, v in (var_leads_metrics_watch or {}).items()}
        self.reset()

    def reset(self):
        self._loss_sum = None     # (T,) sum over batches of batch_size * time_step_loss
        self._mean_sum = None     # () sum over batches of batch_size * mean_loss
        self._count = 0
        self._per_sample = {name: [] for _, name in _PER_SAMPLE}
        self._maps = []

    def update(self, result):
        B = result.batch_size
        tsl, ml = result.time_step_loss.detach().float() * B, result.mean_loss.detach().float() * B
        self._loss_sum = tsl if self._loss_sum is None else self._loss_sum + tsl
        self._mean_sum = ml if self._mean_sum is None else self._mean_sum + ml
        self._count += B
        for attr, name in _PER_SAMPLE:
            t = getattr(result, attr)
            if t is not None:
                self._per_sample[name].append(t.detach().float().clone())
        if result.spatial_loss is not None:
            self._maps.append(result.spatial_loss.detach().float().clone())

    def compute(self):
        if self._count == 0:
            raise RuntimeError("MetricAggregator.compute: no results were added")
        p = self.prefix
        out = {}
        count = _all_reduce_sum(torch.tensor([float(self._count)], device=self._loss_sum.device))
        loss_sum = _all_reduce_sum(self._loss_sum)
        out[f"{p}_mean_loss"] = _all_reduce_sum(self._mean_sum) / count[0]
        for k in self.steps_to_log:
            if k <= loss_sum.shape[0]:
                out[f"{p}_loss_unroll{k}"] = loss_sum[k - 1] / count[0]
        for _, name in _PER_SAMPLE:
            vals = self._per_sample[name]
            if not vals:
                continue
            avg = torch.mean(_all_gather_cat(torch.cat(vals, dim=0)), dim=0)   # (T, F)
            if "mse" in name:
                avg = torch.sqrt(avg)
                name = name.replace("mse", "rmse")
            rescaled = avg * self.state_std.to(avg.device)
            full = f"{p}_{name}"
            out[full] = rescaled
            if full in self.metrics_watch:
                if self.var_names is None:
                    raise ValueError("MetricAggregator: metrics_watch needs the state variable names")
                for var_i, leads in self.var_leads_metrics_watch.items():
                    for step in leads:
                        out[f"{full}_{self.var_names[var_i]}_step_{step}"] = rescaled[step - 1, var_i]
        if self._maps:
            out[f"{p}_mean_spatial_loss"] = torch.nanmean(_all_gather_cat(torch.cat(self._maps, dim=0)), dim=0)
        return out
