"""Generate tests/golden/eval_metrics.pt by running the REFERENCE's own metrics.py (and, for the model cases, its
ARForecaster + GraphLAM) through tests/golden/ref_harness.py: the tensors of validation_step / test_step
(models/module.py:491-504, :546-576, :607-681).

Run in the build container only (needs the reference checkout), after make_golden.py:

    python tests/golden/make_golden_eval.py

Contents:
  "elementwise"  per input set (std form, shape): pred, target, std (per variable (F,) or per entry), interior mask,
                 steps_to_log (1-based; one entry past T, skipped as in test_step) and, in "kinds" order,
                   ref_step_loss (K, B, T)      get_metric(kind)(..., mask=interior)                  (_compute_prediction_and_loss)
                   ref_maps      (K, B, S, N)   get_metric(kind)(..., average_grid=False), NaN off the interior, the logged steps
                 plus ref_sq / ref_ab (B, T, F) = metrics.mse / metrics.mae (sum_vars=False) and, per entry, ref_std_mean (B, T, F)
                 = the interior mean of the std (:626-630).  F of 5 and 17, a batch of 2, ties where pred == target.
  "models"       test_step tensors on the datastore, graph and batch of graphlam_30x27_variants.pt (its full rollout of 3 steps):
                 "mean" = GraphLAM without a predicted std (its own weights, "params") with loss wmse, "std" = that golden's output_std
                 GraphLAM and weights without the clamping, with loss nll.  Per model: prediction, time_step_loss, entry_mse,
                 entry_mae, spatial_loss at steps_to_log, output_std (std model).
"""
import sys
import tempfile
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))

import ref_harness as rh  # noqa: E402
from make_golden import NOTE  # noqa: E402
from make_golden_losses import load_weights  # noqa: E402
from neural_lam_amd.datastore import SyntheticDatastore  # noqa: E402

KINDS = ["mse", "mae", "wmse", "wmae", "nll", "crps_gauss"]


def test_step_tensors(ref, kind, prediction, target, std, interior, steps_to_log, per_entry_std):
    """test_step's tensors (module.py:607-665) for one batch: the per-step loss before its batch mean, mse / mae per variable,
    the mean std (a predicted one only), the loss maps with NaN off the interior at the logged steps."""
    loss = ref.metrics.get_metric(kind)
    step_loss = loss(prediction, target, std, mask=interior)
    sq = ref.metrics.mse(prediction, target, std, mask=interior, sum_vars=False)
    ab = ref.metrics.mae(prediction, target, std, mask=interior, sum_vars=False)
    std_mean = torch.mean(std[..., interior, :], dim=-2) if per_entry_std else None
    spatial = loss(prediction, target, std, average_grid=False)
    spatial[..., ~interior] = float("nan")
    maps = spatial[:, [s - 1 for s in steps_to_log if s <= spatial.shape[1]]]
    return step_loss, sq, ab, std_mean, maps


def elementwise_group(ref, per_entry, B, T, N, F, seed, steps_to_log, ties=False):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, T, N, F, generator=g)
    target = torch.randn(B, T, N, F, generator=g)
    interior = torch.rand(N, generator=g) > 0.3
    if per_entry:
        std = torch.nn.functional.softplus(torch.randn(B, T, N, F, generator=g)) + 0.05
    else:
        std = torch.rand(F, generator=g) + 0.5
    if ties:
        pred.view(-1)[::3] = target.view(-1)[::3]
    out = {"kinds": list(KINDS), "per_entry": per_entry, "pred": pred, "target": target, "std": std, "interior": interior,
           "steps_to_log": list(steps_to_log)}
    step_losses, maps = [], []
    for kind in KINDS:
        sl, sq, ab, sm, mp = test_step_tensors(ref, kind, pred, target, std, interior, steps_to_log, per_entry)
        step_losses.append(sl)
        maps.append(mp)
    out.update(ref_step_loss=torch.stack(step_losses), ref_maps=torch.stack(maps), ref_sq=sq, ref_ab=ab, ref_std_mean=sm)
    return out


def model_cases(ref, steps_to_log):
    base = torch.load(HERE / "graphlam_30x27_variants.pt", weights_only=True)
    tmp = tempfile.mkdtemp()
    ds = SyntheticDatastore(root_path=tmp, **base["ds_kwargs"])
    gdir = Path(tmp) / "graph" / "g"
    ref.create_graph.create_graph(str(gdir), ds.get_xy("state"), **base["graph_kwargs"])
    init, target, forcing = base["init"], base["target"], base["forcing"]
    n_state = ds.get_num_data_vars("state")
    st = ds.get_standardization_dataarray("state")
    diff_std = torch.tensor(st.state_diff_std_standardized.values, dtype=torch.float32)
    per_var_std = diff_std / torch.sqrt(torch.tensor([1.0 / n_state] * n_state, dtype=torch.float32))   # module.py:157-178
    interior = (1.0 - torch.tensor(ds.boundary_mask.values, dtype=torch.float32)).to(torch.bool)
    std_kwargs = {k: v for k, v in base["model_kwargs"].items() if not k.startswith("output_clamping")}
    out = {"T": target.shape[1], "steps_to_log": list(steps_to_log)}
    for name, kwargs, kind in (("mean", dict(std_kwargs, output_std=False), "wmse"), ("std", std_kwargs, "nll")):
        torch.manual_seed(48)
        predictor = ref.GraphLAM(ds, graph_name="g", **kwargs)
        forecaster = ref.ARForecaster(predictor, ds)
        if name == "std":
            load_weights(forecaster, base["state_dict"])
        named = list(forecaster.named_parameters())
        case = {"model_kwargs": kwargs, "kind": kind, "param_names": [k for k, _ in named], "param_numels": [p.numel() for _, p in named]}
        if name == "mean":
            case["params"] = torch.cat([p.detach().reshape(-1) for _, p in named])
        with torch.no_grad():
            prediction, pred_std = forecaster(init, forcing, target)
            predicts_std = pred_std is not None
            std = pred_std if predicts_std else per_var_std
            sl, sq, ab, sm, mp = test_step_tensors(ref, kind, prediction, target, std, interior, steps_to_log, predicts_std)
        case.update(ref_prediction=prediction, ref_time_step_loss=torch.mean(sl, dim=0), ref_entry_mse=sq, ref_entry_mae=ab,
                    ref_output_std=sm, ref_spatial_loss=mp)
        print(f"  model {name} {kind}: mean loss={float(torch.mean(sl)):.6f}")
        out[name] = case
    return out


def main():
    ref = rh.load_reference()
    elementwise = []
    seed = 300
    for per_entry in (False, True):
        for shape in ((2, 3, 23, 5), (1, 4, 30, 17)):
            elementwise.append(elementwise_group(ref, per_entry, *shape, seed, steps_to_log=(1, 3, shape[1] + 1)))
            seed += 1
    ties = [elementwise_group(ref, per_entry, 1, 2, 20, 17, 400 + i, steps_to_log=(2,), ties=True)
            for i, per_entry in enumerate((False, True))]
    models = model_cases(ref, steps_to_log=(1, 3, 4))
    torch.save({"note": NOTE, "elementwise": elementwise, "ties": ties, "models": models}, HERE / "eval_metrics.pt")
    print(f"  {len(elementwise)} elementwise input sets, {len(ties)} tie sets, models {[k for k in models if k in ('mean', 'std')]}")


if __name__ == "__main__":
    main()
