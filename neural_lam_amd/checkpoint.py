"""Checkpoints in the reference's layout, for every optimizer home of this project.

The reference saves Lightning checkpoints (train_model.py:544-560) and resumes from them with ``--load ckpt --restore_opt``
(train_model.py:170-176, 514, 589-592).  Its optimizer is ``torch.optim.AdamW(self.parameters(), betas=(0.9, 0.95))``
(models/module.py:293-304), so a checkpoint holds one state entry per parameter.  This project keeps the same AdamW state
in three places:

* ``trainer.Trainer``: ``ops.AdamWFlat``, two flat fp32 buffers over the ``FlatParams`` layout (reverse registration
  order, every view on a 4-element boundary) and one device-resident step counter;
* ``graphed_training_step(..., flat=True)``: ``torch.optim.AdamW([step.flat_parameter])``, one padded tensor in the
  staging layout of ``_GraphedStep`` (forward order, 4-aligned);
* the stock modules under ``torch.optim.AdamW(module.parameters())``.

``save_checkpoint`` writes, and ``load_checkpoint`` reads, a plain dict shaped like a Lightning checkpoint:
``state_dict``, ``optimizer_states = [sd]`` with ``sd`` exactly what ``torch.optim.AdamW(reference_module.parameters())``
holds, ``lr_schedulers = []``, ``epoch``, ``global_step``, optional ``hyper_parameters`` and a ``"neural_lam_amd"`` entry
(format version and the caller's ``extra``, e.g. the data cursor).  Files written here load with
``torch.load(path, weights_only=True)`` as long as ``hyper_parameters`` and ``extra`` hold plain values.

Optimizer index ``i`` is the ``i``-th PARAMETER name in the order the names appear in the checkpoint's own ``state_dict``
(``state_dict()`` and ``parameters()`` walk the modules in the same order); persistent buffers are skipped.  Moments are
mapped by name, never by position.  A parameter without an entry in ``state`` (torch creates state lazily) loads with
zero moments.

The functions below the public API are pure layout helpers: they need torch only, not the HIP library.
"""
from __future__ import annotations

import os

import torch
from torch import nn

FORMAT_VERSION = 1
NAMESPACE = "neural_lam_amd"
# data buffers the reference's pre-refactor ARModel kept at top level (models/module.py:1098-1103): not remapped there;
# here they are derived from the datastore (non-persistent), so a checkpoint that still carries them drops them
LEGACY_DATA_KEYS = ("interior_mask_bool", "per_var_std")
_GRID_MLP_OLD = "forecaster.predictor.g2m_gnn.grid_mlp"
_GRID_MLP_NEW = "forecaster.predictor.encoding_grid_mlp"


# ---------------------------------------------------------------------------
# Public API
# ---------------------------------------------------------------------------
def save_checkpoint(path, trainer_or_step, optimizer=None, *, epoch, global_step, hyper_parameters=None, extra=None) -> dict:
    """Build a reference-layout checkpoint of ``trainer_or_step`` and write it to ``path`` (``None``: do not write).

    ``trainer_or_step``: a ``trainer.Trainer`` (its ``AdamWFlat``; ``optimizer`` must be None), a ``_GraphedStep`` from
    ``graphed_training_step(..., flat=True)`` with ``optimizer = AdamW([step.flat_parameter])``, or a module with
    ``optimizer = AdamW(module.parameters())``.  Under ``torch.distributed`` only rank 0 writes; every rank gets the dict.
    The file is written next to ``path`` and renamed over it, so a job killed while saving leaves the previous file."""
    from .trainer import Trainer, _GraphedStep

    if isinstance(trainer_or_step, Trainer):
        if optimizer is not None:
            raise ValueError("save_checkpoint: a Trainer owns its optimizer; pass optimizer=None")
        body = trainer_or_step.state_dict()
        group = trainer_or_step.buckets.group
    elif isinstance(trainer_or_step, _GraphedStep):
        if optimizer is None:
            raise ValueError("save_checkpoint: a graphed step needs the optimizer built over step.flat_parameter")
        body = {"state_dict": module_state_to_cpu(trainer_or_step.module),
                "optimizer_states": [trainer_or_step.optimizer_state_to_reference(optimizer)]}
        group = None
    elif isinstance(trainer_or_step, nn.Module):
        if optimizer is None:
            raise ValueError("save_checkpoint: a module needs its optimizer (torch.optim.AdamW(module.parameters()))")
        body = {"state_dict": module_state_to_cpu(trainer_or_step),
                "optimizer_states": [_stock_optimizer_state(trainer_or_step, optimizer)]}
        group = None
    else:
        raise TypeError(f"save_checkpoint: expected a Trainer, a graphed step or a module, got {type(trainer_or_step).__name__}")
    ckpt = {
        "epoch": int(epoch),
        "global_step": int(global_step),
        "state_dict": body["state_dict"],
        "optimizer_states": body["optimizer_states"],
        "lr_schedulers": [],
        NAMESPACE: {"format_version": FORMAT_VERSION, "extra": {} if extra is None else extra},
    }
    ckpt[NAMESPACE].update(body.get(NAMESPACE, {}))   # a Trainer's optimizer controls (schedule, skipped steps), when it has any
    if hyper_parameters is not None:
        ckpt["hyper_parameters"] = hyper_parameters
    if path is not None and _rank(group) == 0:
        path = os.fspath(path)
        tmp = f"{path}.tmp"
        torch.save(ckpt, tmp)
        os.replace(tmp, path)
    return ckpt


def load_checkpoint(path_or_dict, trainer_or_step, optimizer=None, *, restore_opt=True, strict=True, weights_only=True) -> dict:
    """Load a reference-layout checkpoint (a path or the dict itself) into ``trainer_or_step`` (see ``save_checkpoint``).

    The reference's ``on_load_checkpoint`` remaps are applied (models/module.py:1086-1136): legacy un-prefixed keys get
    ``forecaster.predictor.``, ``g2m_gnn.grid_mlp`` becomes ``encoding_grid_mlp``.  Weights are copied in place.
    ``restore_opt=False`` loads the weights only and resets the optimizer (step 0, zero moments, the hyper-parameters it
    was built with), as the reference does without ``--restore_opt``.  Inconsistent state raises a ValueError that names
    the key.  Returns the loaded dict (remapped ``state_dict``) for ``epoch``, ``global_step`` and
    ``ckpt["neural_lam_amd"]["extra"]``.  ``weights_only=False`` is needed for a reference checkpoint whose
    ``hyper_parameters`` hold an ``argparse.Namespace``; only use it on files you trust."""
    from .trainer import Trainer, _GraphedStep

    if isinstance(path_or_dict, dict):
        ckpt = dict(path_or_dict)
    else:
        ckpt = torch.load(os.fspath(path_or_dict), map_location="cpu", weights_only=weights_only)
    if "state_dict" not in ckpt:
        raise ValueError("checkpoint has no 'state_dict'")
    if isinstance(trainer_or_step, (Trainer, _GraphedStep)):
        module = trainer_or_step.module
    elif isinstance(trainer_or_step, nn.Module):
        module = trainer_or_step
    else:
        raise TypeError(f"load_checkpoint: expected a Trainer, a graphed step or a module, got {type(trainer_or_step).__name__}")
    ckpt["state_dict"] = remap_legacy_keys(ckpt["state_dict"], module.state_dict().keys())
    if isinstance(trainer_or_step, Trainer):
        if optimizer is not None:
            raise ValueError("load_checkpoint: a Trainer owns its optimizer; pass optimizer=None")
        trainer_or_step.load_state_dict(ckpt, restore_opt=restore_opt, strict=strict)
        return ckpt
    names = load_module_weights(module, ckpt["state_dict"], strict=strict, copy=False)   # validate before anything changes
    if optimizer is not None and restore_opt:
        sd = _single_optimizer_state(ckpt)
        if isinstance(trainer_or_step, _GraphedStep):
            trainer_or_step.load_reference_optimizer_state(optimizer, sd, names=names, strict=strict)
        else:
            _load_stock_optimizer_state(module, optimizer, sd, names, strict)
    elif optimizer is not None:
        optimizer.state.clear()   # torch creates zero moments and step 0 on the next step; the groups keep what they were built with
    load_module_weights(module, ckpt["state_dict"], strict=strict)
    return ckpt


# ---------------------------------------------------------------------------
# Pure layout helpers (no HIP library)
# ---------------------------------------------------------------------------
def remap_legacy_keys(state_dict: dict, own_keys=()) -> dict:
    """models/module.py:1086-1136 as a new dict that keeps the checkpoint's key order (the optimizer's index order).
    Keys in ``own_keys`` (the target module's ``state_dict`` keys) are left alone: a module that is not laid out like
    ``ForecasterModule`` (any module a ``Trainer`` drives) loads its own keys unchanged."""
    own = set(own_keys)
    keys = [k if (k in own or k.startswith("forecaster.") or k in LEGACY_DATA_KEYS) else f"forecaster.predictor.{k}"
            for k in state_dict]
    if f"{_GRID_MLP_OLD}.0.weight" in keys:
        keys = [_GRID_MLP_NEW + k[len(_GRID_MLP_OLD):] if (k.startswith(_GRID_MLP_OLD) and k not in own) else k for k in keys]
    return dict(zip(keys, state_dict.values()))


def trainable_names(module: nn.Module):
    """Names of the trainable parameters, in ``module.parameters()`` order (= ``FlatParams.params`` / ``_GraphedStep.params``)."""
    return [n for n, p in module.named_parameters() if p.requires_grad]


def flat_params_offsets(shapes):
    """``trainer.FlatParams`` layout: reverse registration order, every view on a 4-element boundary."""
    offs, off = [0] * len(shapes), 0
    for i in reversed(range(len(shapes))):
        offs[i] = off
        off += (_numel(shapes[i]) + 3) // 4 * 4
    return offs, off


def staging_offsets(shapes):
    """``_GraphedStep`` staging / flat-leaf layout: forward order, every view on a 4-element boundary."""
    offs, off = [], 0
    for s in shapes:
        offs.append(off)
        off += (_numel(s) + 3) // 4 * 4
    return offs, off


def optimizer_param_names(state_dict_keys, param_names, buffer_names=()):
    """The parameter name of every reference optimizer index: the checkpoint's keys in their order, persistent buffers and
    legacy data keys skipped.  A key that is neither a known parameter nor a known buffer counts as a parameter (strict
    loading rejects it by name)."""
    params, skip = set(param_names), set(buffer_names) | set(LEGACY_DATA_KEYS)
    return [k for k in state_dict_keys if k in params or k not in skip]


def reorder_optimizer_state(sd, ckpt_names, target_names, shapes, strict=True):
    """A checkpoint's AdamW state dict re-indexed to ``target_names`` (index ``j`` = ``target_names[j]``), matched by name.

    Validates the single parameter group, the parameter set (under ``strict``) and every moment's shape; parameters the
    checkpoint has no state for (or, non-strict, does not know) are left without an entry."""
    groups = sd.get("param_groups")
    if not isinstance(groups, (list, tuple)) or len(groups) != 1:
        raise ValueError(f"optimizer state 'param_groups' has {len(groups) if groups is not None else 0} groups; "
                         "the reference's AdamW (and this project's) has exactly one")
    group = groups[0]
    ids = list(group["params"])
    if len(ids) != len(ckpt_names):
        extra = [n for n in ckpt_names if n not in set(target_names)]
        if not strict and extra and len(ids) == len(ckpt_names) - len(extra):
            ckpt_names = [n for n in ckpt_names if n in set(target_names)]   # the unknown keys were buffers of the saving module
        else:
            raise ValueError(f"optimizer state 'param_groups[0][\"params\"]' has {len(ids)} entries but the checkpoint's "
                             f"state_dict has {len(ckpt_names)} parameters")
    where = {n: j for j, n in enumerate(target_names)}
    if strict:
        for n in ckpt_names:
            if n not in where:
                raise ValueError(f"unexpected parameter {n!r} in the checkpoint")
        have = set(ckpt_names)
        for n in target_names:
            if n not in have:
                raise ValueError(f"missing parameter {n!r} in the checkpoint")
    state = sd.get("state", {})
    out_state = {}
    for pid, name in zip(ids, ckpt_names):
        j = where.get(name)
        if j is None or pid not in state:
            continue
        st = state[pid]
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st and tuple(st[key].shape) != tuple(shapes[j]):
                raise ValueError(f"optimizer state {key!r} of {name!r} has shape {tuple(st[key].shape)}, "
                                 f"the parameter has {tuple(shapes[j])}")
        out_state[j] = st
    out_group = {k: v for k, v in group.items() if k != "params"}
    out_group["params"] = list(range(len(target_names)))
    return {"state": out_state, "param_groups": [out_group]}


def check_flat_group(group):
    """A parameter group the flat AdamW update reproduces: amsgrad and maximize off."""
    if group.get("amsgrad", False):
        raise ValueError("optimizer state 'amsgrad' is True: the flat AdamW kernel implements amsgrad=False only")
    if group.get("maximize", False):
        raise ValueError("optimizer state 'maximize' is True: the flat AdamW kernel implements maximize=False only")


def import_flat_state(sd, shapes, offsets, m, v):
    """A reference-layout AdamW state dict, already indexed like ``shapes`` (``reorder_optimizer_state``), written into
    the flat moment buffers ``m`` / ``v`` at ``offsets`` (padding stays 0).  Returns ``(t, hyper)``:
    one step count for all parameters, ``hyper`` = lr, betas, eps, weight_decay of the group."""
    group = sd["param_groups"][0]
    check_flat_group(group)
    steps = {}
    for j, st in sd["state"].items():
        for key in ("step", "exp_avg", "exp_avg_sq"):
            if key not in st:
                raise ValueError(f"optimizer state of parameter index {j} has no {key!r}")
        steps[j] = float(st["step"])
    t = 0
    if steps:
        t_f = next(iter(steps.values()))
        for j, s in steps.items():
            if s != t_f:
                raise ValueError(f"optimizer state 'step' of parameter index {j} is {s:g}, another parameter's is {t_f:g}: "
                                 "the flat AdamW keeps one step counter")
        if t_f < 0 or t_f != int(t_f):
            raise ValueError(f"optimizer state 'step' is {t_f:g}, not a step count")
        t = int(t_f)
    with torch.no_grad():
        m.zero_()
        v.zero_()
        for j, st in sd["state"].items():
            o, n = offsets[j], _numel(shapes[j])
            m[o : o + n].copy_(st["exp_avg"].reshape(-1))
            v[o : o + n].copy_(st["exp_avg_sq"].reshape(-1))
    hyper = dict(lr=float(group["lr"]), betas=tuple(float(b) for b in group["betas"]), eps=float(group["eps"]),
                 weight_decay=float(group["weight_decay"]))
    return t, hyper


def export_flat_state(shapes, offsets, m, v, t, hyper, group_template=None):
    """The reference-layout AdamW state dict of flat moment buffers: index ``j`` = ``shapes[j]`` at ``offsets[j]``.
    ``t == 0`` gives empty state, as a torch optimizer that has not stepped.  ``group_template``: the other keys of the
    parameter group (default: those the installed torch writes for AdamW)."""
    m_h, v_h = m.detach().to("cpu"), v.detach().to("cpu")   # one device-to-host copy per buffer
    state = {}
    if t > 0:
        for j, (s, o) in enumerate(zip(shapes, offsets)):
            n = _numel(s)
            state[j] = {"step": torch.tensor(float(t), dtype=torch.float32),
                        "exp_avg": m_h[o : o + n].view(s).clone(), "exp_avg_sq": v_h[o : o + n].view(s).clone()}
    group = dict(_adamw_group_template() if group_template is None else group_template)
    group.pop("params", None)
    group.update(lr=hyper["lr"], betas=tuple(hyper["betas"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"])
    group["params"] = list(range(len(shapes)))
    return {"state": state, "param_groups": [group]}


def export_flat_params(names, shapes, offsets, flat) -> dict:
    """A flat buffer in the ``FlatParams`` layout (the weight average of ``ops.AdamWFlat``) cut into ``{name: CPU tensor}``."""
    host = flat.detach().to("cpu")   # one device-to-host copy
    return {n: host[o : o + _numel(s)].view(s).clone() for n, s, o in zip(names, shapes, offsets)}


def import_flat_params(state_dict, names, shapes, offsets, flat, own_keys=()):
    """The inverse: ``{name: tensor}`` (legacy keys remapped as the weights' are) written into ``flat`` at ``offsets``, in
    place.  Every name must be there with its shape; ``flat=None`` only validates."""
    sd = remap_legacy_keys(state_dict, own_keys)
    for n, s in zip(names, shapes):
        if n not in sd:
            raise ValueError(f"missing parameter {n!r} in the checkpoint's weight average")
        if tuple(sd[n].shape) != tuple(s):
            raise ValueError(f"shape mismatch for {n!r} in the checkpoint's weight average: {tuple(sd[n].shape)}, the parameter "
                             f"has {tuple(s)}")
    if flat is not None:
        with torch.no_grad():
            for n, s, o in zip(names, shapes, offsets):
                flat[o : o + _numel(s)].copy_(sd[n].reshape(-1))


def module_state_to_cpu(module: nn.Module) -> dict:
    """``module.state_dict()`` as fresh CPU tensors."""
    return {k: v.detach().to("cpu", copy=True) for k, v in module.state_dict().items()}


def load_module_weights(module: nn.Module, state_dict: dict, strict=True, copy=True):
    """Copy a (remapped) ``state_dict`` into ``module`` IN PLACE: parameters stay where they are (views of a flat buffer,
    addresses that captured graphs and packed weight images hold).  Returns the checkpoint's optimizer index names.
    ``copy=False`` only validates."""
    own = module.state_dict(keep_vars=True)
    param_names = [n for n, _ in module.named_parameters()]
    buffer_names = [k for k in own if k not in set(param_names)]
    for k, src in state_dict.items():
        if k not in own:
            if k in LEGACY_DATA_KEYS:
                continue
            if strict:
                kind = "key" if k in buffer_names else "parameter"
                raise ValueError(f"unexpected {kind} {k!r} in the checkpoint's state_dict")
            continue
        if tuple(src.shape) != tuple(own[k].shape):
            raise ValueError(f"shape mismatch for {k!r}: checkpoint {tuple(src.shape)}, module {tuple(own[k].shape)}")
    if strict:
        for k in own:
            if k not in state_dict:
                kind = "parameter" if k in param_names else "key"
                raise ValueError(f"missing {kind} {k!r} in the checkpoint's state_dict")
    if copy:
        with torch.no_grad():
            for k, dst in own.items():
                if k in state_dict:
                    dst.copy_(state_dict[k])
    return optimizer_param_names(state_dict.keys(), param_names, buffer_names)


# ---------------------------------------------------------------------------
# internals
# ---------------------------------------------------------------------------
def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _adamw_group_template():
    return torch.optim.AdamW([torch.zeros(1)]).state_dict()["param_groups"][0]


def _rank(group=None):
    import torch.distributed as dist

    return dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0


def _single_optimizer_state(ckpt):
    states = ckpt.get("optimizer_states")
    if not isinstance(states, (list, tuple)) or len(states) != 1:
        raise ValueError(f"checkpoint 'optimizer_states' must hold one optimizer state, got "
                         f"{len(states) if isinstance(states, (list, tuple)) else type(states).__name__}")
    return states[0]


def _check_stock_optimizer(module, optimizer):
    params = list(module.parameters())
    groups = optimizer.param_groups
    if len(groups) != 1 or len(groups[0]["params"]) != len(params) or any(a is not b for a, b in zip(groups[0]["params"], params)):
        raise ValueError("the optimizer must hold module.parameters(), in order, in one parameter group")


def _stock_optimizer_state(module, optimizer):
    """``optimizer.state_dict()`` of ``AdamW(module.parameters())`` with CPU tensors (already the reference layout)."""
    _check_stock_optimizer(module, optimizer)
    sd = optimizer.state_dict()
    state = {j: {k: (v.detach().to("cpu", copy=True) if torch.is_tensor(v) else v) for k, v in st.items()}
             for j, st in sd["state"].items()}
    return {"state": state, "param_groups": sd["param_groups"]}


def _load_stock_optimizer_state(module, optimizer, sd, names, strict):
    _check_stock_optimizer(module, optimizer)
    target = [n for n, _ in module.named_parameters()]
    shapes = [tuple(p.shape) for p in module.parameters()]
    optimizer.load_state_dict(reorder_optimizer_state(sd, names, target, shapes, strict=strict))
