"""Validation / test metrics (models/module.py:491-504, :546-576, :607-681, :923-1071): the C-ABI of nlam_eval_metrics without a
GPU, ops.eval_metrics / ForecasterStep.evaluate argument checks, evaluation.MetricAggregator against a restatement of the
reference's epoch aggregation (one process and two gloo ranks), and on the GPU the kernel and the model-level evaluation
against the reference golden (tests/golden/eval_metrics.pt, tests/golden/make_golden_eval.py), the equality of evaluate's mean
loss with the training loss, determinism and graph replay."""
import ctypes as C
import os
import socket
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, graph_from_case, load_golden, rel_err
from neural_lam_amd import _lib as L

KINDS = ["mse", "mae", "wmse", "wmae", "nll", "crps_gauss"]
NEW_EXPORTS = ["nlam_eval_metrics", "nlam_eval_workspace_floats"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("eval_metrics")


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_eval_entry_points_reject_bad_arguments_without_a_gpu():
    assert set(NEW_EXPORTS) <= set(L.EXPORTS)
    lib = L.load()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    fake = 1 << 20   # never dereferenced: every call below must fail its argument checks before a launch
    B, T, N, F = 2, 3, 40, 5
    nws = lib.nlam_eval_workspace_floats(B, T, N, F)
    assert nws >= B * T * (3 * F + 1)
    for bad in ((0, T, N, F), (B, 0, N, F), (B, T, 0, F), (B, T, N, 0), (B, T, N, L.EVAL_MAX_VARS + 1)):
        assert lib.nlam_eval_workspace_floats(*bad) == -1, bad

    def args(**kw):
        p = L.Eval()
        p.pred = p.target = p.var_std = p.row_weight = p.workspace = p.step_loss = p.sq = p.maps = fake
        p.workspace_floats, p.batch, p.steps, p.nodes, p.nvars, p.kind, p.nmaps = nws, B, T, N, F, L.LOSS_NLL, 2
        p.map_steps[0], p.map_steps[1] = 0, T - 1
        for k, v in kw.items():
            if k == "map_steps":
                for i, s in enumerate(v):
                    p.map_steps[i] = s
            else:
                setattr(p, k, v)
        return C.byref(p)

    assert lib.nlam_eval_metrics(None, None) == -1
    for bad in (dict(kind=0), dict(kind=7), dict(pred=None), dict(target=None), dict(row_weight=None), dict(workspace=None),
                dict(var_std=None), dict(batch=0), dict(steps=0), dict(nodes=0), dict(nvars=0), dict(nmaps=-1),
                dict(maps=None), dict(map_steps=[0, T]), dict(map_steps=[-1, 0]), dict(workspace_floats=nws - 1),
                dict(std_mean=fake)):   # a mean std needs the per-entry std
        assert lib.nlam_eval_metrics(args(**bad), None) == -1, bad
    assert lib.nlam_eval_metrics(args(nvars=L.EVAL_MAX_VARS + 1), None) == -2
    assert lib.nlam_eval_metrics(args(nvars=L.LOSS_MAX_VARS + 1), None) == -2
    assert lib.nlam_eval_metrics(args(nmaps=L.EVAL_MAX_MAPS + 1), None) == -2


def test_eval_struct_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "nlam_hip.h"\n'
        'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(nlam_eval_t), offsetof(nlam_eval_t, workspace),'
        " offsetof(nlam_eval_t, maps), offsetof(nlam_eval_t, workspace_floats), offsetof(nlam_eval_t, batch),"
        " offsetof(nlam_eval_t, nmaps), offsetof(nlam_eval_t, map_steps), NLAM_EVAL_MAX_MAPS, NLAM_EVAL_MAX_VARS); return 0;}\n"
    )
    exe = tmp_path / "sz"
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(L.Eval), L.Eval.workspace.offset, L.Eval.maps.offset, L.Eval.workspace_floats.offset,
                   L.Eval.batch.offset, L.Eval.nmaps.offset, L.Eval.map_steps.offset, L.EVAL_MAX_MAPS, L.EVAL_MAX_VARS]


def test_eval_metrics_host_checks_raise_value_error():
    from neural_lam_amd.ops import eval_metrics

    B, T, N, F = 1, 2, 10, 5
    x = torch.zeros(B, T, N, F)
    rw = torch.full((N,), 0.1)
    with pytest.raises(ValueError, match="GPU"):
        eval_metrics(x, x, None, torch.ones(F), rw, "wmse")
    with pytest.raises(ValueError, match="unknown loss kind"):
        eval_metrics(x, x, None, torch.ones(F), rw, "huber")
    with pytest.raises(ValueError, match="unknown loss kind"):
        eval_metrics(x, x, None, torch.ones(F), rw, 9)
    with pytest.raises(ValueError, match=r"\(B, T, N, F\)"):
        eval_metrics(x, x[:, :1], None, torch.ones(F), rw, "wmse")
    with pytest.raises(ValueError, match="needs pred_std or var_std"):
        eval_metrics(x, x, None, None, rw, "nll")


def _small_step(tmp_path, **kw):
    from neural_lam_amd import graph as G
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    ds = SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)
    ext = ds.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state")), max(ext[1] - ext[0], ext[3] - ext[2]))
    torch.manual_seed(1)
    return ds, hm.ForecasterStep(hm.ARForecaster(hm.GraphLAM(ds, graph=graph, **kw), ds), ds)


def test_evaluate_rejects_an_unknown_phase(tmp_path):
    ds, step = _small_step(tmp_path, hidden_dim=8, processor_layers=1)
    N = ds.num_grid_points
    batch = [torch.zeros(1, 2, N, 5), torch.zeros(1, 2, N, 5), torch.zeros(1, 2, N, 6)]
    for phase in ("train", "Test", "validation", None):
        with pytest.raises(ValueError, match="phase"):
            step.evaluate(*batch, phase=phase)


# the reference's epoch formulas, restated (they cannot be imported without Lightning):
#   _log_step_loss (module.py:512-544) under Lightning's on_epoch=True, batch_size=B: sum_i B_i x_i / sum_i B_i
#   aggregate_and_plot_metrics (:923-993): cat, all_gather_cat, mean over samples, sqrt for "mse" (-> "rmse"), * state_std;
#   create_metric_log_dict (:867-921) for the metrics_watch scalars; on_test_epoch_end (:994-1071): nanmean of the maps
def _reference_epoch(batches, state_std, var_names, prefix, steps_to_log, metrics_watch, var_leads_metrics_watch):
    logs = {}
    sizes = torch.tensor([float(b["B"]) for b in batches])
    logs[f"{prefix}_mean_loss"] = sum(torch.mean(b["time_step_loss"]) * b["B"] for b in batches) / sizes.sum()
    T = batches[0]["time_step_loss"].shape[0]
    for step in steps_to_log:
        if step <= T:
            logs[f"{prefix}_loss_unroll{step}"] = sum(b["time_step_loss"][step - 1] * b["B"] for b in batches) / sizes.sum()
    metrics = {"mse": "entry_mse"}
    if prefix == "test":
        metrics.update(mae="entry_mae", output_std="output_std")
    for metric_name, key in metrics.items():
        if batches[0].get(key) is None:
            continue
        metric_tensor = torch.cat([b[key] for b in batches], dim=0)
        averaged = torch.mean(metric_tensor, dim=0)
        if "mse" in metric_name:
            averaged = torch.sqrt(averaged)
            metric_name = metric_name.replace("mse", "rmse")
        rescaled = averaged * state_std
        full = f"{prefix}_{metric_name}"
        logs[full] = rescaled
        if full in metrics_watch:
            for var_i, timesteps in var_leads_metrics_watch.items():
                for step in timesteps:
                    logs[f"{full}_{var_names[var_i]}_step_{step}"] = rescaled[step - 1, var_i]
    if prefix == "test":
        logs["test_mean_spatial_loss"] = torch.nanmean(torch.cat([b["spatial_loss"] for b in batches], dim=0), dim=0)
    return logs


def _fake_batches(seed, sizes, T=3, N=12, F=4, S=2, std=True):
    from neural_lam_amd.models import EvalResult

    g = torch.Generator().manual_seed(seed)
    out = []
    for B in sizes:
        tsl = torch.rand(T, generator=g)
        maps = torch.rand(B, S, N, generator=g)
        maps[..., ::3] = float("nan")
        d = {"B": B, "time_step_loss": tsl, "entry_mse": torch.rand(B, T, F, generator=g),
             "entry_mae": torch.rand(B, T, F, generator=g), "output_std": torch.rand(B, T, F, generator=g) if std else None,
             "spatial_loss": maps}
        d["result"] = EvalResult("test", torch.zeros(B, T, N, F), tsl, torch.mean(tsl), d["entry_mse"], d["entry_mae"], maps,
                                 d["output_std"], (1, 3))
        out.append(d)
    return out


def _check_logs(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        assert torch.allclose(torch.as_tensor(got[k]), v, rtol=1e-6, atol=0, equal_nan=True), k


@pytest.mark.parametrize("prefix", ["val", "test"])
def test_metric_aggregator_matches_restated_reference_epoch(prefix):
    from neural_lam_amd.evaluation import MetricAggregator

    state_std = torch.tensor([1.0, 2.0, 0.5, 1.5])
    names = ["a", "b", "c", "d"]
    watch = (f"{prefix}_rmse", "test_mae")
    leads = {1: [1, 3], 3: [2]}
    batches = _fake_batches(7, (2, 1, 3))
    if prefix == "val":   # validation_step keeps only the mse
        for b in batches:
            b["entry_mae"] = b["output_std"] = b["spatial_loss"] = None
            r = b["result"]
            r.entry_mae = r.output_std = r.spatial_loss = None
    agg = MetricAggregator(state_std, names, prefix=prefix, steps_to_log=(1, 3, 5), metrics_watch=watch,
                           var_leads_metrics_watch=leads)
    for b in batches:
        agg.update(b["result"])
    got = agg.compute()
    want = _reference_epoch(batches, state_std, names, prefix, (1, 3, 5), watch, leads)
    _check_logs(got, want)
    assert f"{prefix}_loss_unroll5" not in got and f"{prefix}_rmse_b_step_3" in got
    assert ("test_mae_d_step_2" in got) == (prefix == "test")
    # sample-weighted means, not batch means
    assert not torch.allclose(got[f"{prefix}_mean_loss"], torch.stack([torch.mean(b["time_step_loss"]) for b in batches]).mean())


def test_metric_aggregator_reads_the_datastore(tmp_path):
    from neural_lam_amd.datastore import SyntheticDatastore
    from neural_lam_amd.evaluation import MetricAggregator

    ds = SyntheticDatastore(6, 5, 4, 2, 1, root_path=tmp_path, boundary="random", seed=1)
    names = list(ds.get_vars_names(category="state"))
    state_std = torch.tensor(ds.get_standardization_dataarray("state").state_std.values, dtype=torch.float32)
    batches = _fake_batches(3, (1, 2), N=ds.num_grid_points)
    agg = MetricAggregator(ds, prefix="test", steps_to_log=(1, 3), metrics_watch=("test_rmse",), var_leads_metrics_watch={0: [2]})
    for b in batches:
        agg.update(b["result"])
    _check_logs(agg.compute(), _reference_epoch(batches, state_std, names, "test", (1, 3), ("test_rmse",), {0: [2]}))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _agg_worker(rank, world, port, out_dir):
    import torch.distributed as dist

    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from neural_lam_amd.evaluation import MetricAggregator

    agg = MetricAggregator(torch.tensor([1.0, 2.0, 0.5, 1.5]), list("abcd"), prefix="test", steps_to_log=(1, 2),
                           metrics_watch=("test_mae",), var_leads_metrics_watch={2: [1, 3]})
    for b in _fake_batches(50 + rank, (2, 2)):
        agg.update(b["result"])
    torch.save(agg.compute(), f"{out_dir}/rank{rank}.pt")
    dist.destroy_process_group()


def test_metric_aggregator_two_rank_gloo_equals_one_rank_with_both_batches(tmp_path):
    import torch.multiprocessing as mp

    from neural_lam_amd.evaluation import MetricAggregator

    mp.spawn(_agg_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=False)
    one = MetricAggregator(torch.tensor([1.0, 2.0, 0.5, 1.5]), list("abcd"), prefix="test", steps_to_log=(1, 2),
                           metrics_watch=("test_mae",), var_leads_metrics_watch={2: [1, 3]})
    # all_gather_cat orders the samples by rank: rank 0's batches, then rank 1's
    for b in _fake_batches(50, (2, 2)) + _fake_batches(51, (2, 2)):
        one.update(b["result"])
    want = one.compute()
    for got in (r0, r1):
        assert set(got) == set(want)
        for k in want:
            assert torch.allclose(got[k], want[k], rtol=1e-6, atol=0, equal_nan=True), k


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L.load()
    return torch.device("cuda:0")


def _misaligned(t):
    """The same values at a 4-byte offset: a contiguous view whose data pointer is not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


def _nan_rel_err(got, want):
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    fin = ~torch.isnan(want)
    return rel_err(got[fin], want[fin])


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True])
def test_eval_kernel_matches_reference_golden(dev, golden, misalign):
    """nlam_eval_metrics for every kind x std form x F in {5, 17} (batch 2 in one case, ties in two): per-step loss, per-variable
    MSE / MAE / mean std, loss maps with NaN exactly off the interior; the 16-byte path and the scalar one (misaligned)."""
    from neural_lam_amd.ops import eval_metrics

    put = (lambda t: _misaligned(t.to(dev))) if misalign else (lambda t: t.to(dev))
    for grp in golden["elementwise"] + golden["ties"]:
        pred, target = put(grp["pred"]), put(grp["target"])
        T = pred.shape[1]
        interior = grp["interior"].to(torch.float32)
        rw = (interior / interior.sum()).to(dev)
        steps = [s - 1 for s in grp["steps_to_log"] if s <= T]
        assert len(steps) < len(grp["steps_to_log"]) or len(grp["steps_to_log"]) == 1   # an entry past T was dropped
        std = put(grp["std"]) if grp["per_entry"] else None
        var_std = None if grp["per_entry"] else grp["std"].to(dev)
        for i, kind in enumerate(grp["kinds"]):
            what = (kind, grp["per_entry"], tuple(pred.shape), misalign)
            m = eval_metrics(pred, target, std, var_std, rw, kind, steps, want_mae=True, want_std=grp["per_entry"])
            torch.cuda.synchronize()
            assert rel_err(m["step_loss"].cpu(), grp["ref_step_loss"][i]) <= 1e-5, what
            assert rel_err(m["sq"].cpu(), grp["ref_sq"]) <= 1e-5, what
            assert rel_err(m["ab"].cpu(), grp["ref_ab"]) <= 1e-5, what
            if grp["per_entry"]:
                assert rel_err(m["std_mean"].cpu(), grp["ref_std_mean"]) <= 1e-5, what
            maps = m["maps"].cpu()
            assert bool(torch.isnan(maps).eq(~grp["interior"]).all()), what   # NaN exactly at the boundary nodes
            assert _nan_rel_err(maps, grp["ref_maps"][i]) <= 1e-5, what


def _golden_step(golden, model, dev, tmp_path, kind=None):
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore

    base, case = load_golden("graphlam_30x27_variants"), golden["models"][model]
    ds = SyntheticDatastore(root_path=tmp_path, **base["ds_kwargs"])
    fc = hm.ARForecaster(hm.GraphLAM(ds, graph=(base["ref_hierarchical"], graph_from_case(base)), **case["model_kwargs"]), ds)
    names = case["param_names"]
    assert [k for k, _ in fc.named_parameters()] == names
    sd = fc.state_dict()
    if "params" in case:
        for k, v in zip(names, torch.split(case["params"], case["param_numels"])):
            sd[k] = v.view_as(sd[k])
    else:
        sd.update({k: base["state_dict"][k] for k in names})
    fc.load_state_dict(sd, strict=True)
    batch = [t.contiguous().to(dev) for t in (base["init"], base["target"], base["forcing"])]
    return hm.ForecasterStep(fc, ds, loss=kind or case["kind"]).to(dev), batch


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["mean", "std"])
def test_evaluate_matches_reference_golden(dev, golden, tmp_path, model):
    """ForecasterStep.evaluate(phase="test") against the reference's ARForecaster + test_step tensors (the training tests'
    tolerances), and phase "val" gives the same loss and MSE without the test-only tensors."""
    case = golden["models"][model]
    step, batch = _golden_step(golden, model, dev, tmp_path)
    steps_to_log = golden["models"]["steps_to_log"]
    r = step.evaluate(*batch, phase="test", steps_to_log=steps_to_log)
    assert r.map_steps == tuple(s for s in steps_to_log if s <= golden["models"]["T"])
    assert rel_err(r.prediction.cpu(), case["ref_prediction"]) < 1e-4
    assert rel_err(r.time_step_loss.cpu(), case["ref_time_step_loss"]) < 1e-4
    assert abs(float(r.mean_loss) - float(case["ref_time_step_loss"].mean())) < 1e-4 * abs(float(case["ref_time_step_loss"].mean()))
    assert rel_err(r.entry_mse.cpu(), case["ref_entry_mse"]) < 1e-4
    assert rel_err(r.entry_mae.cpu(), case["ref_entry_mae"]) < 1e-4
    assert _nan_rel_err(r.spatial_loss.cpu(), case["ref_spatial_loss"]) < 1e-4
    if case["ref_output_std"] is not None:
        assert rel_err(r.output_std.cpu(), case["ref_output_std"]) < 1e-4
    else:
        assert r.output_std is None
    v = step.evaluate(*batch, phase="val", steps_to_log=steps_to_log)
    assert v.entry_mae is None and v.spatial_loss is None and v.output_std is None
    assert torch.equal(v.time_step_loss, r.time_step_loss) and torch.equal(v.entry_mse, r.entry_mse)


@pytest.mark.gpu
@pytest.mark.parametrize("model,kind", [("mean", k) for k in KINDS] + [("std", k) for k in KINDS])
def test_evaluate_mean_loss_equals_training_loss(dev, golden, tmp_path, model, kind):
    """evaluate's mean_loss is the loss ForecasterStep.forward trains on (the batch mean of time_step_loss, module.py:412)."""
    step, batch = _golden_step(golden, model, dev, tmp_path, kind)
    with torch.no_grad():
        _, loss = step(*batch)
    r = step.evaluate(*batch, phase="val")
    assert abs(float(r.mean_loss) - float(loss)) <= 1e-6 * abs(float(loss)), (float(r.mean_loss), float(loss))


@pytest.mark.gpu
def test_evaluate_is_bit_identical_run_to_run(dev, golden, tmp_path):
    step, batch = _golden_step(golden, "std", dev, tmp_path, "crps_gauss")
    a = step.evaluate(*batch, phase="test", steps_to_log=(1, 2, 3))
    b = step.evaluate(*batch, phase="test", steps_to_log=(1, 2, 3))
    for k in ("prediction", "time_step_loss", "mean_loss", "entry_mse", "entry_mae", "output_std"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.spatial_loss, b.spatial_loss) or bool(
        (a.spatial_loss.isnan() == b.spatial_loss.isnan()).all() and torch.equal(a.spatial_loss.nan_to_num(), b.spatial_loss.nan_to_num()))


@pytest.mark.gpu
@pytest.mark.parametrize("model,phase", [("mean", "val"), ("std", "test")])
def test_graphed_eval_step_equals_eager_evaluate(dev, golden, tmp_path, model, phase):
    """One graph replay = eager evaluate, bit for bit; a second batch copied into the same buffers gives that batch's eager
    result; another batch shape falls through to the eager evaluate."""
    from neural_lam_amd.trainer import graphed_eval_step

    step, batch = _golden_step(golden, model, dev, tmp_path)
    g = torch.Generator().manual_seed(11)
    other = [t + 0.1 * torch.randn(t.shape, generator=g).to(dev) for t in batch]
    fields = ("prediction", "time_step_loss", "mean_loss", "entry_mse", "entry_mae", "output_std", "spatial_loss")

    def same(a, b):
        for k in fields:
            x, y = getattr(a, k), getattr(b, k)
            assert (x is None) == (y is None), k
            if x is not None:
                assert torch.equal(x.nan_to_num(), y.nan_to_num()) and torch.equal(x.isnan(), y.isnan()), k

    graphed = graphed_eval_step(step, *batch, phase=phase, steps_to_log=(1, 3))
    for b in (batch, other, batch):
        got = graphed(*b)
        want = step.evaluate(*b, phase=phase, steps_to_log=(1, 3))
        same(got, want)
    short = [batch[0], batch[1][:, :2].contiguous(), batch[2][:, :2].contiguous()]
    got = graphed(*short)
    assert got.prediction.shape[1] == 2
    same(got, step.evaluate(*short, phase=phase, steps_to_log=(1, 3)))
