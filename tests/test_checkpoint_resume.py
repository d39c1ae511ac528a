"""Checkpoints in the reference's layout (neural_lam_amd/checkpoint.py): the optimizer state of Trainer's AdamWFlat, of
AdamW([flat_parameter]) on the drop-in path and of the stock AdamW(module.parameters()) converts to and from what
torch.optim.AdamW(reference_module.parameters()) holds (models/module.py:293-304), and a resumed run continues bit for bit.

CPU tests: layouts, key remaps, errors, the file format.  GPU tests: resume on every executor, loading into a live
trainer, the data cursor, import parity with torch's AdamW, flat leaf <-> stock, restore_opt=False, two ranks."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

from conftest import ROOT

from neural_lam_amd import checkpoint as ck


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _datastore(tmp_path):
    from neural_lam_amd.datastore import SyntheticDatastore

    return SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)


def _graph(ds):
    from neural_lam_amd import graph as G

    ext = ds.get_xy_extent("state")
    return G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))


def _clamping(ds):
    """Output clamping of three kinds: the predictor then holds persistent clamping buffers between its parameters."""
    names = ds.get_vars_names("state")
    return dict(output_clamping_lower={names[0]: -1.0, names[1]: 0.0}, output_clamping_upper={names[0]: 2.0, names[2]: 3.0})


class _Ref(nn.Module):
    """The reference's key layout: ForecasterModule holds the ARForecaster as ``.forecaster``."""

    def __init__(self, fc):
        super().__init__()
        self.forecaster = fc


def _oracle(ds, graph, seed=1):
    from oracle import models as om

    torch.manual_seed(seed)
    return _Ref(om.ARForecaster(om.GraphLAM(ds, graph, hidden_dim=16, processor_layers=2, **_clamping(ds)), ds))


def _hip_step(ds, graph, seed=1, clamp=True, **kw):
    from neural_lam_amd import models as hm

    torch.manual_seed(seed)
    pred = hm.GraphLAM(ds, graph=graph, hidden_dim=16, processor_layers=2, **(_clamping(ds) if clamp else {}))
    return hm.ForecasterStep(hm.ARForecaster(pred, ds), ds, **kw)


def _stepped_adamw(module, steps=2, seed=0):
    """torch AdamW(betas=(0.9, 0.95)) after ``steps`` updates with a different random gradient per parameter."""
    opt = torch.optim.AdamW(module.parameters(), lr=1e-3, betas=(0.9, 0.95))
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in module.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def _same(a, b, path="root"):
    """Recursive bit-for-bit equality of nested dicts / lists / tensors / plain values."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        assert torch.is_tensor(a) and torch.is_tensor(b), path
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), (path, set(a) ^ set(b))
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b and type(a) is type(b), (path, a, b)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_layout_round_trip_through_flat_and_staging_layouts(tmp_path):
    """Reference AdamW state -> FlatParams buffers -> reference layout, and the same through the _GraphedStep staging layout:
    the same dict bit for bit, every moment on its own name, padding 0.  The HIP module's parameter order equals the
    reference's, and the persistent clamping buffers are skipped in the index mapping."""
    from neural_lam_amd.trainer import FlatParams

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    ref = _oracle(ds, graph)
    opt = _stepped_adamw(ref)
    ref_sd, opt_sd = ref.state_dict(), opt.state_dict()
    ref_names = [n for n, _ in ref.named_parameters()]
    buffers = [k for k in ref_sd if k not in set(ref_names)]
    assert "forecaster.predictor.clamp_lower_upper_idx" in buffers and "forecaster.predictor.sigmoid_lower_lims" in buffers
    assert ck.optimizer_param_names(ref_sd.keys(), ref_names, buffers) == ref_names
    by_name = dict(zip(ref_names, (opt.state[p] for p in ref.parameters())))
    ms = [by_name[n]["exp_avg"] for n in ref_names]
    assert len({float(m.reshape(-1)[0]) for m in ms}) == len(ms)   # no two moments alike: a misplaced one would show

    step = _hip_step(ds, graph, seed=5)
    names = ck.trainable_names(step)
    assert names == ref_names   # the HIP module registers its parameters in the reference's order
    fp = FlatParams(step)
    shapes = [tuple(p.shape) for p in fp.params]
    offs = [fp.offsets[i] for i in range(len(fp.params))]
    assert (offs, fp.numel) == ck.flat_params_offsets(shapes)
    ckpt_names = ck.load_module_weights(step, ck.remap_legacy_keys(ref_sd))
    assert ckpt_names == ref_names
    _same(ck.module_state_to_cpu(step), ref_sd)

    for layout in ("flat", "staging"):
        if layout == "flat":
            m, v = torch.zeros_like(fp.flat), torch.zeros_like(fp.flat)
            o = offs
        else:
            o, total = ck.staging_offsets(shapes)
            m, v = torch.zeros(total), torch.zeros(total)
        t, hyper = ck.import_flat_state(ck.reorder_optimizer_state(opt_sd, ckpt_names, names, shapes), shapes, o, m, v)
        assert t == 2 and hyper == dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-2)
        for n, s, off in zip(names, shapes, o):
            k = int(np.prod(s))
            assert torch.equal(m[off : off + k].view(s), by_name[n]["exp_avg"]), (layout, n)
            assert torch.equal(v[off : off + k].view(s), by_name[n]["exp_avg_sq"]), (layout, n)
        used = torch.zeros(m.numel(), dtype=torch.bool)
        for s, off in zip(shapes, o):
            used[off : off + int(np.prod(s))] = True
        assert not m[~used].any() and not v[~used].any()   # padding stays 0
        _same(ck.export_flat_state(shapes, o, m, v, t, hyper), opt_sd)


def test_optimizer_state_is_mapped_by_name_not_by_position(tmp_path):
    """A checkpoint whose state_dict lists the parameters in another order: index i is the i-th parameter name of THAT
    state_dict, so the moments still land on their own names."""
    ds = _datastore(tmp_path)
    graph = _graph(ds)
    ref = _oracle(ds, graph)
    opt = _stepped_adamw(ref)
    sd, osd = ref.state_dict(), opt.state_dict()
    names = [n for n, _ in ref.named_parameters()]
    perm = list(reversed(range(len(names))))
    buffers = [k for k in sd if k not in set(names)]
    shuffled_sd = {**{names[i]: sd[names[i]] for i in perm}, **{k: sd[k] for k in buffers}}
    shuffled_opt = {"state": {j: osd["state"][i] for j, i in enumerate(perm)}, "param_groups": osd["param_groups"]}
    got = ck.reorder_optimizer_state(shuffled_opt, ck.optimizer_param_names(shuffled_sd.keys(), names, buffers), names,
                                     [tuple(p.shape) for p in ref.parameters()])
    _same(got, osd)


def test_legacy_key_remaps_and_stock_module_load(tmp_path):
    """models/module.py:1086-1136: un-prefixed keys get forecaster.predictor., g2m_gnn.grid_mlp becomes encoding_grid_mlp,
    the key order (= the optimizer's index order) is kept; a legacy checkpoint loads into a stock module + AdamW."""
    sd = {"g2m_gnn.grid_mlp.0.weight": 1, "g2m_gnn.grid_mlp.0.bias": 2, "mesh_embedder.0.weight": 3,
          "interior_mask_bool": 4, "per_var_std": 5, "forecaster.predictor.x": 6}
    out = ck.remap_legacy_keys(sd)
    assert list(out) == ["forecaster.predictor.encoding_grid_mlp.0.weight", "forecaster.predictor.encoding_grid_mlp.0.bias",
                         "forecaster.predictor.mesh_embedder.0.weight", "interior_mask_bool", "per_var_std",
                         "forecaster.predictor.x"]
    assert list(out.values()) == [1, 2, 3, 4, 5, 6]
    assert list(ck.remap_legacy_keys({"forecaster.predictor.g2m_gnn.grid_mlp.0.weight": 0})) == \
        ["forecaster.predictor.encoding_grid_mlp.0.weight"]   # already prefixed, renamed only
    assert list(ck.remap_legacy_keys({"net.w": 0, "old.w": 1}, own_keys=["net.w"])) == ["net.w", "forecaster.predictor.old.w"]

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    ref = _oracle(ds, graph)
    opt = _stepped_adamw(ref)
    legacy = {}
    for k, v in ref.state_dict().items():
        k = k[len("forecaster.predictor."):]
        legacy[k.replace("encoding_grid_mlp", "g2m_gnn.grid_mlp")] = v
    legacy["interior_mask_bool"] = torch.ones(3, dtype=torch.bool)   # a pre-refactor data buffer: dropped
    assert any(k.startswith("g2m_gnn.grid_mlp") for k in legacy)
    dst = _oracle(ds, graph, seed=9)
    dst_opt = torch.optim.AdamW(dst.parameters(), lr=5e-3)
    got = ck.load_checkpoint({"state_dict": legacy, "optimizer_states": [opt.state_dict()]}, dst, dst_opt)
    assert "forecaster.predictor.encoding_grid_mlp.0.weight" in got["state_dict"]
    _same(dst.state_dict(), ref.state_dict())
    _same(dst_opt.state_dict(), opt.state_dict())


def test_errors_name_the_offending_key(tmp_path):
    from neural_lam_amd.trainer import Trainer

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    ref = _oracle(ds, graph)
    opt = _stepped_adamw(ref)
    sd, osd = ref.state_dict(), opt.state_dict()
    names = [n for n, _ in ref.named_parameters()]
    shapes = [tuple(p.shape) for p in ref.parameters()]
    victim = names[3]

    dst = _oracle(ds, graph, seed=2)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    missing = {k: v for k, v in sd.items() if k != victim}
    with pytest.raises(ValueError, match=f"missing parameter '{victim}'"):
        ck.load_checkpoint({"state_dict": missing}, dst)
    with pytest.raises(ValueError, match="unexpected parameter 'forecaster.predictor.bogus.weight'"):
        ck.load_checkpoint({"state_dict": {**sd, "forecaster.predictor.bogus.weight": torch.zeros(2)}}, dst)
    with pytest.raises(ValueError, match=f"shape mismatch for '{victim}'"):
        ck.load_checkpoint({"state_dict": {**sd, victim: torch.zeros(7, 7)}}, dst)
    _same(dst.state_dict(), before)   # a rejected checkpoint changes nothing
    ck.load_checkpoint({"state_dict": missing}, dst, strict=False)   # non-strict: the rest loads
    assert torch.equal(dst.state_dict()[names[4]], sd[names[4]]) and torch.equal(dst.state_dict()[victim], before[victim])

    def flat_import(o):
        re = ck.reorder_optimizer_state(o, names, names, shapes)
        return ck.import_flat_state(re, shapes, ck.staging_offsets(shapes)[0], torch.zeros(100000), torch.zeros(100000))

    bad = {"state": dict(osd["state"]), "param_groups": osd["param_groups"]}
    bad["state"][3] = {**osd["state"][3], "exp_avg": torch.zeros(5)}
    with pytest.raises(ValueError, match=f"'exp_avg' of '{victim}'"):
        flat_import(bad)
    two = {"state": osd["state"], "param_groups": [dict(osd["param_groups"][0], params=[0]),
                                                   dict(osd["param_groups"][0], params=list(range(1, len(names))))]}
    with pytest.raises(ValueError, match="param_groups"):
        flat_import(two)
    with pytest.raises(ValueError, match="amsgrad"):
        flat_import({"state": osd["state"], "param_groups": [dict(osd["param_groups"][0], amsgrad=True)]})
    skew = {"state": dict(osd["state"]), "param_groups": osd["param_groups"]}
    skew["state"][5] = {**osd["state"][5], "step": torch.tensor(7.0)}
    with pytest.raises(ValueError, match="'step' of parameter index 5"):
        flat_import(skew)
    with pytest.raises(ValueError, match="unexpected parameter 'forecaster.predictor.extra'"):
        ck.reorder_optimizer_state({"state": {}, "param_groups": [dict(osd["param_groups"][0], params=list(range(len(names) + 1)))]},
                                   names + ["forecaster.predictor.extra"], names, shapes)
    with pytest.raises(ValueError, match=f"missing parameter '{names[-1]}'"):
        ck.reorder_optimizer_state({"state": {}, "param_groups": [dict(osd["param_groups"][0], params=list(range(len(names) - 1)))]},
                                   names[:-1], names, shapes)

    # lazily created state: a parameter without an entry loads with zero moments
    lazy = {"state": {i: s for i, s in osd["state"].items() if i != 3}, "param_groups": osd["param_groups"]}
    o, total = ck.staging_offsets(shapes)
    m, v = torch.full((total,), 9.0), torch.full((total,), 9.0)
    t, _ = ck.import_flat_state(ck.reorder_optimizer_state(lazy, names, names, shapes), shapes, o, m, v)
    assert t == 2 and not m[o[3] : o[3] + int(np.prod(shapes[3]))].any() and m[o[4]] != 0

    # a Trainer with any other optimizer than AdamWFlat has no reference-layout state
    class Plain:
        def step(self, grad_scale=1.0):
            pass

    tr = Trainer(_oracle(ds, graph), optimizer_factory=lambda p, g: Plain())
    with pytest.raises(TypeError, match="AdamWFlat"):
        tr.state_dict()
    with pytest.raises(TypeError, match="AdamWFlat"):
        tr.load_state_dict({"state_dict": sd, "optimizer_states": [osd]})
    with pytest.raises(TypeError, match="AdamWFlat"):
        ck.save_checkpoint(None, tr, epoch=0, global_step=0)


def test_written_file_loads_with_weights_only(tmp_path):
    ds = _datastore(tmp_path)
    graph = _graph(ds)
    ref = _oracle(ds, graph)
    opt = _stepped_adamw(ref, steps=3)
    path = tmp_path / "last.ckpt"
    hp = {"args": {"model": "graph_lam", "lr": 1e-3}}
    made = ck.save_checkpoint(path, ref, opt, epoch=4, global_step=123, hyper_parameters=hp, extra={"epoch": 4, "batch": 7})
    got = torch.load(path, weights_only=True)
    _same(got, made)
    assert got["epoch"] == 4 and got["global_step"] == 123 and got["lr_schedulers"] == [] and got["hyper_parameters"] == hp
    assert got["neural_lam_amd"] == {"format_version": ck.FORMAT_VERSION, "extra": {"epoch": 4, "batch": 7}}
    _same(got["optimizer_states"][0], opt.state_dict())
    assert not os.path.exists(f"{path}.tmp")
    dst = _oracle(ds, graph, seed=3)
    dst_opt = torch.optim.AdamW(dst.parameters(), lr=1e-3, betas=(0.9, 0.95))
    back = ck.load_checkpoint(path, dst, dst_opt)
    assert back["neural_lam_amd"]["extra"] == {"epoch": 4, "batch": 7}
    _same(dst_opt.state_dict(), opt.state_dict())
    dst_opt2 = torch.optim.AdamW(dst.parameters(), lr=1e-3, betas=(0.9, 0.95))
    _stepped_adamw(dst, steps=1)
    ck.load_checkpoint(path, dst, dst_opt2, restore_opt=False)
    assert dst_opt2.state_dict()["state"] == {}


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from neural_lam_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _batches(ds, dev, n, seed=0, T=2):
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(1, 2, N, 5, generator=g).to(dev), torch.randn(1, T, N, 5, generator=g).to(dev),
             torch.randn(1, T, N, 6, generator=g).to(dev)] for _ in range(n)]


_MODES = {"eager": dict(use_graph=False), "forks": dict(use_graph=True, executor="forks"),
          "segments": dict(use_graph=True, executor="segments")}


def _trainer(ds, graph, dev, mode, seed=1, lr=1e-3):
    from neural_lam_amd.trainer import Trainer

    return Trainer(_hip_step(ds, graph, seed=seed).to(dev), lr=lr, **_MODES[mode])


def _assert_same_state(a, b):
    assert torch.equal(a.fp.flat, b.fp.flat)
    assert torch.equal(a.opt.m, b.opt.m) and torch.equal(a.opt.v, b.opt.v)
    assert a.opt.t == b.opt.t and torch.equal(a.opt.t_dev, b.opt.t_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "forks", "segments"])
def test_resume_is_bit_identical(dev, tmp_path, mode):
    """A: 5 steps.  B: 3 steps, saved.  C: a fresh module and trainer loading B's file, 2 steps.  C's losses, weights, m, v
    and t equal A's bit for bit (same trainer mode: the weight-gradient summation order depends on it)."""
    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = _batches(ds, dev, 5)
    a = _trainer(ds, graph, dev, mode)
    la = [float(a.step(*b)) for b in batches]
    b_ = _trainer(ds, graph, dev, mode)
    lb = [float(b_.step(*b)) for b in batches[:3]]
    assert lb == la[:3]
    path = tmp_path / "b.ckpt"
    ck.save_checkpoint(path, b_, epoch=0, global_step=3)
    c = _trainer(ds, graph, dev, mode, seed=7)
    assert not torch.equal(c.fp.flat, b_.fp.flat)
    got = ck.load_checkpoint(path, c)
    assert got["global_step"] == 3 and c.opt.t == 3 and int(c.opt.t_dev.item()) == 3
    lc = [float(c.step(*b)) for b in batches[3:]]
    assert lc == la[3:]
    _assert_same_state(c, a)
    assert int(a.opt.t_dev.item()) == 5
    if mode != "eager":
        assert c._graph is not None


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["forks", "segments"])
def test_load_into_a_live_trainer(dev, tmp_path, mode):
    """A trainer that has captured and stepped loads B's checkpoint in place: its next 2 steps equal a fresh trainer's
    (the packed weight images are rewritten from the loaded weights at the start of every step).  A checkpoint with
    another lr re-records the captured AdamW launch once, without switching the trainer to schedule mode, even after
    an earlier lr change of its own."""
    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = _batches(ds, dev, 5)
    own = _batches(ds, dev, 2, seed=11)
    b_ = _trainer(ds, graph, dev, mode)
    for b in batches[:3]:
        b_.step(*b)
    ckpt = ck.save_checkpoint(None, b_, epoch=0, global_step=3)
    fresh = _trainer(ds, graph, dev, mode, seed=7)
    ck.load_checkpoint(ckpt, fresh)
    lf = [float(fresh.step(*b)) for b in batches[3:]]

    live = _trainer(ds, graph, dev, mode, seed=9)
    for b in own:
        live.step(*b)
    assert live._graph is not None
    packer_before = live._packer
    ptr = live.fp.flat.data_ptr()
    ck.load_checkpoint(ckpt, live)
    assert live.fp.flat.data_ptr() == ptr and live._packer is packer_before
    assert [float(live.step(*b)) for b in batches[3:]] == lf
    _assert_same_state(live, fresh)

    # another lr in the checkpoint
    other = dict(ckpt)
    osd = ckpt["optimizer_states"][0]
    other["optimizer_states"] = [{"state": osd["state"], "param_groups": [dict(osd["param_groups"][0], lr=5e-4)]}]
    fresh2 = _trainer(ds, graph, dev, mode, seed=7)
    ck.load_checkpoint(other, fresh2)
    assert fresh2.opt.lr == 5e-4
    lf2 = [float(fresh2.step(*b)) for b in batches[3:]]
    assert lf2[0] == lf[0] and not torch.equal(fresh2.fp.flat, fresh.fp.flat)   # same first loss, another update
    live2 = _trainer(ds, graph, dev, mode, seed=9)
    live2.step(*own[0])
    live2.opt.lr = 2e-3   # one schedule change of its own: re-records once
    live2.step(*own[1])
    assert live2._opt_changes == 1 and not live2._opt_eager
    ck.load_checkpoint(other, live2)
    assert live2.opt.lr == 5e-4 and not live2._opt_eager and live2._opt_changes == 1
    assert [float(live2.step(*b)) for b in batches[3:]] == lf2
    _assert_same_state(live2, fresh2)
    assert live2._opt_in_graph or live2._tail_graph is not None   # the optimizer is still captured


@pytest.mark.gpu
def test_mid_epoch_resume_feeds_the_same_batches(dev, tmp_path):
    """A step_from loop over a DeviceWeatherDataset stopped after k batches and resumed from the checkpoint's cursor
    (epoch, batch index; epoch_permutation(seed=epoch) is deterministic) equals the uninterrupted run bit for bit."""
    from neural_lam_amd.data import DeviceWeatherDataset
    from neural_lam_amd.trainer import Trainer

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    N = ds.num_grid_points
    rng = np.random.default_rng(4)
    state = rng.normal(size=(14, N, 5)).astype(np.float32)
    forcing = rng.normal(size=(14, N, 2)).astype(np.float32)
    times = np.arange(14, dtype=np.int64) * 3 * 3600 * 10**9

    def make(seed=1):
        tr = Trainer(_hip_step(ds, graph, seed=seed, standardize=False).to(dev), lr=1e-3, use_graph=True)
        data = DeviceWeatherDataset(state, forcing, times, ar_steps=2, num_past_forcing_steps=1, num_future_forcing_steps=1,
                                    standardization=tr.module.standardization_stats())
        return tr, data

    B, epochs = 2, 2

    def run(tr, data, start=(0, 0), stop=None):
        losses = []
        nb = len(data) // B
        for epoch in range(start[0], epochs):
            perm = data.epoch_permutation(seed=epoch)
            for k in range(start[1] if epoch == start[0] else 0, nb):
                if stop is not None and (epoch, k) == stop:
                    return losses, ck.save_checkpoint(tmp_path / "last.ckpt", tr, epoch=epoch, global_step=tr.opt.t,
                                                      extra={"epoch": epoch, "batch": k})
                losses.append(float(tr.step_from(data, perm[k * B : (k + 1) * B])))
        return losses, None

    full_tr, data = make()
    full, _ = run(full_tr, data)
    assert len(data) // B >= 3 and len(full) == epochs * (len(data) // B)
    part_tr, data2 = make()
    first, _ = run(part_tr, data2, stop=(0, 2))
    del part_tr
    res_tr, data3 = make(seed=6)
    got = ck.load_checkpoint(tmp_path / "last.ckpt", res_tr)
    cur = got["neural_lam_amd"]["extra"]
    rest, _ = run(res_tr, data3, start=(cur["epoch"], cur["batch"]))
    assert first + rest == full
    _assert_same_state(res_tr, full_tr)


@pytest.mark.gpu
def test_reference_checkpoint_import_matches_torch_adamw(dev, tmp_path):
    """Stock HIP modules under torch.optim.AdamW take 3 steps and save a reference-layout checkpoint; a Trainer loads it
    and takes one step, torch's AdamW takes the same step.  The HIP bias correction uses powf where torch uses Python
    ``**``: agreement within a few fp32 ulps of each parameter's magnitude."""
    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = _batches(ds, dev, 4)
    s = _hip_step(ds, graph).to(dev)
    opt = torch.optim.AdamW(s.parameters(), lr=1e-3, betas=(0.9, 0.95))
    for b in batches[:3]:
        opt.zero_grad(set_to_none=True)
        s(*b)[1].backward()
        opt.step()
    ckpt = ck.save_checkpoint(None, s, opt, epoch=0, global_step=3)
    tr = _trainer(ds, graph, dev, "eager", seed=8)
    ck.load_checkpoint(ckpt, tr)
    assert tr.opt.t == 3
    l_tr = float(tr.step(*batches[3]))
    opt.zero_grad(set_to_none=True)
    l_ref = s(*batches[3])[1]
    l_ref.backward()
    opt.step()
    assert l_tr == float(l_ref)
    worst = 0.0
    eps = torch.finfo(torch.float32).eps
    for (name, a), b in zip(tr.module.named_parameters(), s.parameters()):
        ulps = float((a - b).abs().max()) / (eps * max(float(b.abs().max()), 1e-30))
        worst = max(worst, ulps)
        assert ulps <= 4.0, (name, ulps)
    print(f"reference import parity: worst parameter difference {worst:.3f} ulp of the parameter's magnitude")


@pytest.mark.gpu
def test_flat_leaf_and_stock_optimizer_states_convert_both_ways(dev, tmp_path):
    """From one checkpoint, graphed_training_step(flat=True) under AdamW([flat_parameter]) and the eager module under
    AdamW(module.parameters()) take the same next step bit for bit; the drop-in path's checkpoint equals the stock one and
    restores into the stock module."""
    from neural_lam_amd.trainer import graphed_training_step

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = _batches(ds, dev, 6)
    s0 = _hip_step(ds, graph).to(dev)
    o0 = torch.optim.AdamW(s0.parameters(), lr=1e-3, betas=(0.9, 0.95))
    for b in batches[:2]:
        o0.zero_grad(set_to_none=True)
        s0(*b)[1].backward()
        o0.step()
    stock_ckpt = ck.save_checkpoint(None, s0, o0, epoch=0, global_step=2)

    def eager_step(mod, opt, b):
        opt.zero_grad(set_to_none=True)
        loss = mod(*b)[1]
        loss.backward()
        opt.step()
        return float(loss)

    s_g = _hip_step(ds, graph, seed=5).to(dev)
    graphed = graphed_training_step(s_g, *batches[0], flat=True)
    o_g = torch.optim.AdamW([graphed.flat_parameter], lr=2e-3)
    ck.load_checkpoint(stock_ckpt, graphed, o_g)   # stock -> drop-in
    s_e = _hip_step(ds, graph, seed=6).to(dev)
    o_e = torch.optim.AdamW(s_e.parameters(), lr=2e-3)
    ck.load_checkpoint(stock_ckpt, s_e, o_e)
    for b in batches[2:4]:
        l0 = eager_step(s0, o0, b)
        le = eager_step(s_e, o_e, b)
        o_g.zero_grad(set_to_none=True)
        lg = graphed(*b)[1]
        lg.backward()
        o_g.step()
        assert l0 == le == float(lg)
        for a, c, d in zip(s0.parameters(), s_e.parameters(), s_g.parameters()):
            assert torch.equal(a, c) and torch.equal(a, d)
    drop_ckpt = ck.save_checkpoint(None, graphed, o_g, epoch=0, global_step=4)   # drop-in -> stock
    _same(drop_ckpt["optimizer_states"], ck.save_checkpoint(None, s_e, o_e, epoch=0, global_step=4)["optimizer_states"])
    s_r = _hip_step(ds, graph, seed=7).to(dev)
    o_r = torch.optim.AdamW(s_r.parameters(), lr=2e-3)
    ck.load_checkpoint(drop_ckpt, s_r, o_r)
    for b in batches[4:]:
        assert eager_step(s_r, o_r, b) == eager_step(s_e, o_e, b)
        for a, c in zip(s_r.parameters(), s_e.parameters()):
            assert torch.equal(a, c)
    leaf = graphed.flat_parameter
    pad = torch.ones(leaf.numel(), dtype=torch.bool, device=dev)
    for p, o in zip(s_g.parameters(), graphed.goffs):
        pad[o : o + p.numel()] = False
    assert not o_g.state[leaf]["exp_avg"][pad].any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "segments"])
def test_restore_opt_false_equals_a_new_trainer_on_the_weights(dev, tmp_path, mode):
    """restore_opt=False: weights only, step 0, zero moments and the trainer's own hyper-parameters -- the trajectory of a
    new trainer built on the loaded weights."""
    from neural_lam_amd.trainer import Trainer

    ds = _datastore(tmp_path)
    graph = _graph(ds)
    batches = _batches(ds, dev, 5)
    b_ = _trainer(ds, graph, dev, mode, lr=5e-4)
    for b in batches[:3]:
        b_.step(*b)
    ckpt = ck.save_checkpoint(None, b_, epoch=0, global_step=3)
    live = _trainer(ds, graph, dev, mode, seed=9)
    live.step(*batches[0])
    ck.load_checkpoint(ckpt, live, restore_opt=False)
    assert live.opt.t == 0 and int(live.opt.t_dev.item()) == 0 and live.opt.lr == 1e-3
    assert not live.opt.m.any() and not live.opt.v.any()
    mod = _hip_step(ds, graph, seed=3).to(dev)
    mod.load_state_dict(ckpt["state_dict"])
    new = Trainer(mod, lr=1e-3, **_MODES[mode])
    for b in batches[3:]:
        assert float(live.step(*b)) == float(new.step(*b))
    _assert_same_state(live, new)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, out_dir, two_gpus):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dev = torch.device(f"cuda:{rank}" if two_gpus else "cuda:0")
    torch.cuda.set_device(dev)
    if two_gpus:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)   # "nccl" is RCCL on ROCm
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            probe = torch.ones(4, device=dev)
            dist.all_reduce(probe)
        except Exception as exc:  # this torch build's gloo cannot reduce device tensors
            torch.save({"unsupported": repr(exc)}, f"{out_dir}/rank{rank}.pt")
            dist.destroy_process_group()
            return
    from neural_lam_amd import checkpoint as ckp
    from neural_lam_amd import gnn_layers as hl
    from neural_lam_amd.trainer import Trainer

    torch.manual_seed(0)
    ei = torch.stack([torch.randint(0, 60, (900,)), torch.randint(0, 50, (900,))])
    ei[1, -1] = 49

    class Step(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = hl.InteractionNet(ei, 64)

        def forward(self, send, rec, edge):
            r, e = self.net(send, rec, edge)
            return (r.square().mean() + e.square().mean(),)

    def make(seed):
        torch.manual_seed(seed)
        return Trainer(Step().to(dev), lr=1e-2, use_graph=True)

    g = torch.Generator().manual_seed(100 + rank)
    batches = [tuple(torch.randn(1, n, 64, generator=g).to(dev) for n in (60, 50, 900)) for _ in range(3)]
    tr = make(1)
    for b in batches[:2]:
        tr.step(*b)
    path = f"{out_dir}/ckpt.pt"
    made = ckp.save_checkpoint(path, tr, epoch=0, global_step=2)
    dist.barrier()
    fresh = make(10 + rank)   # different weights per rank until the load
    ckp.load_checkpoint(path, fresh)
    tr.step(*batches[2])
    fresh.step(*batches[2])
    mismatch = None
    bad = dict(made)
    if rank == 1:
        bad["state_dict"] = {k: v + 1.0 if v.is_floating_point() else v for k, v in made["state_dict"].items()}
    try:
        ckp.load_checkpoint(bad, make(1))
    except ValueError as exc:
        mismatch = str(exc)
    torch.cuda.synchronize()
    torch.save({"flat": fresh.fp.flat.cpu(), "ref": tr.fp.flat.cpu(), "m": fresh.opt.m.cpu(), "t": fresh.opt.t,
                "has_dict": "optimizer_states" in made, "mismatch": mismatch}, f"{out_dir}/rank{rank}.pt")
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_save_on_rank0_load_everywhere(dev, tmp_path):
    """world = 2: rank 0 writes, both ranks load and stay identical; ranks that load different weights are refused.
    Two GPUs: RCCL, one rank each; one GPU: two ranks sharing it over gloo (as tests/test_ddp_gloo.py does)."""
    world = 2
    two_gpus = torch.cuda.device_count() >= 2
    mp.spawn(_two_rank_worker, args=(world, _free_port(), str(tmp_path), two_gpus), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=False)
    if "unsupported" in r0:
        pytest.skip(f"one GPU and gloo cannot all-reduce device tensors here: {r0['unsupported']}")
    assert r0["has_dict"] and r1["has_dict"]
    assert torch.equal(r0["flat"], r1["flat"]) and torch.equal(r0["m"], r1["m"]) and r0["t"] == r1["t"] == 3
    assert torch.equal(r0["flat"], r0["ref"])
    assert r0["mismatch"] is not None and r1["mismatch"] is not None and "ranks" in r0["mismatch"]
