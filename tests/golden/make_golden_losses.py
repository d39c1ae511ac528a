"""Generate tests/golden/losses.pt by running the REFERENCE's own metrics.py (and, for the model cases, its
ARForecaster + GraphLAM) through tests/golden/ref_harness.py.

Run in the build container only (needs the reference checkout), after make_golden.py:

    python tests/golden/make_golden_losses.py

Contents:
  "elementwise"  per (kind, std form, shape): pred, target, std, interior mask -> the training reduction of
                 metrics.<kind> (masked grid mean, variable sum, batch mean, step mean; models/module.py:491-504, :412)
                 with its autograd gradients w.r.t. pred and std.  Shapes with a total that is / is not a multiple of 4.
                 One entry per (std form, shape): its inputs and the results of the six kinds stacked in "kinds" order.
  "ties"         mae / wmae with interior entries where pred == target (sign(0) = 0 in the gradient).
  "models"       training steps on the datastore, graph and batch of graphlam_30x27_variants.pt (first two AR steps):
                 "mean" = GraphLAM without a predicted std (its own weights, "params") trained with each loss, "std" = that golden's
                 output_std GraphLAM and weights without the clamping, trained with nll / crps_gauss.  Per model the
                 prediction, per kind the loss and every parameter gradient (flattened in param_names order).
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
from neural_lam_amd.datastore import SyntheticDatastore  # noqa: E402

KINDS = ["mse", "mae", "wmse", "wmae", "nll", "crps_gauss"]


def ref_loss(ref, kind, prediction, target, std, interior):
    """training_step's reduction of metrics.<kind> (models/module.py:491-504, :412)."""
    time_step_loss = torch.mean(ref.metrics.get_metric(kind)(prediction, target, std, mask=interior), dim=0)
    return torch.mean(time_step_loss)


def elementwise_inputs(per_entry, B, T, N, F, seed, ties=False):
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
    return pred, target, std, interior


def elementwise_group(ref, kinds, per_entry, inputs):
    """One input set and, stacked in `kinds` order, the loss and gradients of every kind on it (one tensor per field)."""
    pred0, target, std0, interior = inputs
    losses, dpreds, dstds = [], [], []
    for kind in kinds:
        pred, std = pred0.clone().requires_grad_(), std0.clone().requires_grad_()
        loss = ref_loss(ref, kind, pred, target, std, interior)
        loss.backward()
        losses.append(loss.detach())
        dpreds.append(pred.grad)
        dstds.append(std.grad if std.grad is not None else torch.zeros_like(std0))   # mse / mae: the std is not read
    return {
        "kinds": list(kinds), "per_entry": per_entry, "pred": pred0, "target": target, "std": std0, "interior": interior,
        "ref_loss": torch.stack(losses), "ref_dpred": torch.stack(dpreds), "ref_dstd": torch.stack(dstds) if per_entry else None,
    }


def load_weights(forecaster, state_dict):
    """The golden's parameters into a model without its clamping (the clamping buffers are the only other entries)."""
    sd = forecaster.state_dict()
    sd.update({k: state_dict[k] for k, _ in forecaster.named_parameters()})
    forecaster.load_state_dict(sd, strict=True)


def model_cases(ref, T=2):
    base = torch.load(HERE / "graphlam_30x27_variants.pt", weights_only=True)
    tmp = tempfile.mkdtemp()
    ds = SyntheticDatastore(root_path=tmp, **base["ds_kwargs"])
    gdir = Path(tmp) / "graph" / "g"
    ref.create_graph.create_graph(str(gdir), ds.get_xy("state"), **base["graph_kwargs"])
    init, target, forcing = base["init"], base["target"][:, :T].contiguous(), base["forcing"][:, :T].contiguous()
    n_state = ds.get_num_data_vars("state")
    st = ds.get_standardization_dataarray("state")
    diff_std = torch.tensor(st.state_diff_std_standardized.values, dtype=torch.float32)
    per_var_std = diff_std / torch.sqrt(torch.tensor([1.0 / n_state] * n_state, dtype=torch.float32))   # module.py:157-178
    interior = (1.0 - torch.tensor(ds.boundary_mask.values, dtype=torch.float32)).to(torch.bool)
    std_kwargs = {k: v for k, v in base["model_kwargs"].items() if not k.startswith("output_clamping")}
    out = {"T": T}
    for name, kwargs, kinds in (("mean", dict(std_kwargs, output_std=False), KINDS), ("std", std_kwargs, ["nll", "crps_gauss"])):
        torch.manual_seed(48)
        predictor = ref.GraphLAM(ds, graph_name="g", **kwargs)
        forecaster = ref.ARForecaster(predictor, ds)
        for k, v in base["ref_graph_loaded"].items():   # the graph the test builds from the base golden
            mine = getattr(predictor, k)
            assert all(torch.equal(a.to(b.dtype), b) for a, b in zip(v if isinstance(v, list) else [v], mine if isinstance(mine, list) else [mine])), k
        if name == "std":
            load_weights(forecaster, base["state_dict"])
        case = {"model_kwargs": kwargs, "kinds": {}}
        named = list(forecaster.named_parameters())
        case["param_names"], case["param_numels"] = [k for k, _ in named], [p.numel() for _, p in named]
        if name == "mean":   # its own weights, flattened in param_names order
            case["params"] = torch.cat([p.detach().reshape(-1) for _, p in named])
        for kind in kinds:
            forecaster.zero_grad(set_to_none=True)
            prediction, pred_std = forecaster(init, forcing, target)
            loss = ref_loss(ref, kind, prediction, target, per_var_std if pred_std is None else pred_std, interior)
            loss.backward()
            case["ref_prediction"] = prediction.detach()
            case["kinds"][kind] = {   # every parameter gradient, flattened in param_names order (one tensor: a small file)
                "ref_loss": loss.detach(),
                "ref_grads": torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for _, p in named]),
            }
            print(f"  model {name} {kind}: loss={float(loss.detach()):.6f}")
        out[name] = case
    return out


def main():
    ref = rh.load_reference()
    elementwise = []
    seed = 100
    for per_entry in (False, True):
        for shape in ((2, 1, 20, 4), (1, 2, 19, 5)):   # total a multiple of 4 (16-byte path) and not (scalar path)
            elementwise.append(elementwise_group(ref, KINDS, per_entry, elementwise_inputs(per_entry, *shape, seed)))
            seed += 1
    ties = [elementwise_group(ref, ("mae", "wmae"), per_entry, elementwise_inputs(per_entry, 1, 2, 20, 4, 200 + i, ties=True))
            for i, per_entry in enumerate((False, True))]
    models = model_cases(ref)
    torch.save({"note": NOTE, "elementwise": elementwise, "ties": ties, "models": models}, HERE / "losses.pt")
    print(f"  {len(elementwise)} elementwise input sets, {len(ties)} tie sets, models {[k for k in models if k != 'T']}")


if __name__ == "__main__":
    main()
