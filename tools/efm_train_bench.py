#!/usr/bin/env python3
"""The Graph-EFM training step (models.EFMForecasterStep) against the same objective composed from torch ops, one process,
alternating, both through Trainer(use_graph=True).

    python tools/efm_train_bench.py [--ar-steps 1 4] [--steps 30] [--rounds 3] [--out profiles/efm_train/bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/efm_train_bench.py --trace fused --ar-steps 1 --steps 50
    python tools/efm_train_bench.py --parse-stats DIR/t_kernel_stats.csv --steps 50     # kernels per step, share of the new launches

A GraphEFM (hierarchical mesh, three levels) on the MEPS-shaped grid (238 x 268, 17 state variables) at hidden_dim 64, batch 1.
Route "fused": the step as it ships -- nlam_latent_kl_fwd / _bwd for the draw and the KL, the fused step tails for the state update
and the likelihood.  Route "torch": the same modules with torch.distributions (Normal, rsample, kl_divergence), the predictor's
unfused tail (FUSED_STATE_UPDATE off) and models.nll on the interior -- the composition tests/test_efm_training.py checks the
step against.  Route "fused_eager": the fused step without the recording (use_graph=False), the like-for-like partner of a
"torch" route whose recording failed (``recorded`` false: Trainer then runs it with eager launches).  Per route and rollout
length: ms per step (HIP events around ``--steps`` synchronised steps; median over the alternating rounds and their spread), and
whether the step really ran as a recorded graph.

    python tools/efm_train_bench.py --crps-members 2 [--out profiles/efm_crps/bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/efm_train_bench.py --crps-members 2 --trace crps_fused --ar-steps 1 --steps 50
    python tools/efm_train_bench.py --crps-members 2 --parse-stats DIR/t_kernel_stats.csv --steps 50

With ``--crps-members M`` the routes are those of the fine-tuning stage instead, all three recorded: "elbo" (the step without members),
"crps_fused" (``crps_members=M``, the term on nlam_crps_ens_fwd / _bwd) and "crps_torch" (the same member rollout with
NLAM_FUSED_CRPS=0: the term from torch ops on the same member states).
"""
import argparse
import csv
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

NEW_KERNELS = ("latent_kl_fwd_kernel", "latent_kl_finish_kernel", "latent_kl_bwd_kernel")
CRPS_KERNELS = ("latent_draw_fwd_kernel", "latent_draw_bwd_kernel", "crps_ens_fwd_kernel", "crps_ens_finish_kernel", "crps_ens_bwd_kernel")
SETUP_KERNELS = ("spin_kernel",)   # the one-off stream-layout probe of ops._streams_share_queue: no part of a step


def parse_stats(path, steps, new_kernels=NEW_KERNELS):
    """Kernels per pass and the share of the new launches from a rocprofv3 kernel_stats.csv of a ``--trace`` run of ``steps``
    steps: the run makes steps + 2 passes (the two warm-up passes of the recording run eagerly, the recording itself runs nothing).
    SETUP_KERNELS are left out; the other one-off launches of the set-up (weight initialisation, graph layouts) are not."""
    rows = [r for r in csv.DictReader(open(path)) if not any(k in r["Name"] for k in SETUP_KERNELS)]
    calls = sum(int(r["Calls"]) for r in rows)
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    new = [r for r in rows if any(k in r["Name"] for k in new_kernels)]
    passes = steps + 2
    return {"stats_file": str(path), "passes": passes, "kernels_per_step": calls / passes, "kernel_ms_per_step": total / passes / 1e6,
            "new_launches_per_step": sum(int(r["Calls"]) for r in new) / passes,
            "new_launches_share_of_kernel_time": sum(float(r["TotalDurationNs"]) for r in new) / total if total else None,
            "new_launches": {r["Name"][:60]: {"calls": int(r["Calls"]), "avg_us": float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3}
                             for r in new}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ar-steps", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", choices=("fused", "fused_eager", "torch", "elbo", "crps_fused", "crps_torch"), default=None,
                    help="run one route for --steps steps and exit (for a kernel trace)")
    ap.add_argument("--crps-members", type=int, default=0, help="M > 0: time the fine-tuning stage (routes elbo, crps_fused, crps_torch)")
    ap.add_argument("--crps-weight", type=float, default=1.0)
    ap.add_argument("--parse-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parse_stats is not None:
        print(json.dumps(parse_stats(args.parse_stats, args.steps, CRPS_KERNELS if args.crps_members else NEW_KERNELS), indent=1))
        return

    import torch
    from torch import nn
    from torch.distributions import kl_divergence

    from neural_lam_amd import _lib as L
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore
    from neural_lam_amd.trainer import Trainer

    # Normal(..) validates its arguments with a read-back to the host, which no stream capture permits: off, so that the torch
    # composition can be recorded like the fused step (the values are the same)
    torch.distributions.Distribution.set_default_validate_args(False)
    dev = torch.device("cuda:0")
    NX, NY, NS, NF, NST, D = 238, 268, 17, 6, 4, 64
    ds = SyntheticDatastore(NX, NY, NS, NF, NST, root_path="/tmp/nlam_efm_bench", boundary="frame", seed=0)
    ext = ds.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state"), n_max_levels=3, hierarchical=True),
                              max(ext[1] - ext[0], ext[3] - ext[2]))
    N = ds.num_grid_points

    class TorchElbo(nn.Module):
        """The objective of EFMForecasterStep from torch ops on the same modules."""

        def __init__(self, step):
            super().__init__()
            self.step = step

        def forward(self, init, target, forcing):
            step, fc, model = self.step, self.step.forecaster, self.step.forecaster.predictor
            prev_prev, prev = init[:, 0], init[:, 1]
            liks, kls, preds = [], [], []
            with model.static_cache():
                for t in range(target.shape[1]):
                    grid_prev_emb, graph_emb = model.embedd_grid_and_graph(prev, prev_prev, forcing[:, t])
                    prior = model.prior_model(grid_prev_emb, graph_emb=graph_emb)
                    post = model.encoder(model.embedd_grid_with_target(prev, prev_prev, forcing[:, t], target[:, t]), graph_emb=graph_emb)
                    z = post.rsample()
                    kls.append(kl_divergence(post, prior).sum((1, 2)))
                    pred_state, pred_std = model.decode(grid_prev_emb, graph_emb, z, prev)
                    new = fc.boundary_mask * target[:, t] + fc.interior_mask * pred_state
                    liks.append(hm.nll(new, target[:, t], pred_std if pred_std is not None else step.per_var_std, mask=step.interior_index))
                    preds.append(new)
                    prev_prev, prev = prev, new
            loss = torch.stack(liks).mean() + step.kl_beta / step.n_interior * torch.stack(kls).mean()
            return torch.stack(preds, dim=1), loss

    def make(route, T):
        torch.manual_seed(42)
        model = graph_efm.GraphEFM(ds, graph=graph, hidden_dim=D)
        members = args.crps_members if route in ("crps_fused", "crps_torch") else 0
        step = hm.EFMForecasterStep(hm.EFMForecaster(model, ds), ds, seed=1, crps_members=members,
                                    crps_weight=args.crps_weight if members else 0.0).to(dev)
        module = TorchElbo(step) if route == "torch" else step
        tr = Trainer(module, lr=1e-4, use_graph=route != "fused_eager")
        g = torch.Generator().manual_seed(123)
        batch = tuple(t.to(dev) for t in (torch.randn(1, 2, N, NS, generator=g), torch.randn(1, T, N, NS, generator=g),
                                          torch.randn(1, T, N, NF * 3, generator=g)))

        def run(n):
            hm.FUSED_STATE_UPDATE = route != "torch"
            hm.FUSED_CRPS = route != "crps_torch"
            try:
                for _ in range(n):
                    loss = tr.step(*batch)
            finally:
                hm.FUSED_STATE_UPDATE = hm.FUSED_CRPS = True
            return loss

        return tr, run

    def window_ms(run, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        loss = run(n)
        e1.record()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(loss)):
            raise RuntimeError("the loss is not finite")
        return e0.elapsed_time(e1) / n

    if args.trace:
        tr, run = make(args.trace, args.ar_steps[0])
        run(args.steps)
        torch.cuda.synchronize()
        print(json.dumps({"route": args.trace, "ar_steps": args.ar_steps[0], "steps": args.steps, "recorded": tr.use_graph and tr._graph is not None}))
        return

    out = {"grid": [NX, NY], "nodes": N, "state_vars": NS, "hidden_dim": D, "batch": 1, "steps": args.steps, "rounds": args.rounds,
           "crps_members": args.crps_members,
           "source_stamp": L.source_stamp(), "device": torch.cuda.get_device_name(0), "ar_steps": {}}
    for T in args.ar_steps:
        names = ("elbo", "crps_fused", "crps_torch") if args.crps_members else ("fused", "fused_eager", "torch")
        routes = {name: make(name, T) for name in names}
        for _, run in routes.values():
            run(3)   # warm-up passes and the recording
        ms = {name: [] for name in routes}
        for _ in range(args.rounds):
            for name, (_, run) in routes.items():
                ms[name].append(window_ms(run, args.steps))
        row = {name: {"ms_per_step": statistics.median(v), "ms_per_step_rounds": v, "spread_ms": max(v) - min(v),
                      "recorded": routes[name][0].use_graph and routes[name][0]._graph is not None} for name, v in ms.items()}
        if args.crps_members:
            row["crps_torch_over_crps_fused"] = row["crps_torch"]["ms_per_step"] / row["crps_fused"]["ms_per_step"]
            row["crps_fused_over_elbo"] = row["crps_fused"]["ms_per_step"] / row["elbo"]["ms_per_step"]
        else:
            row["torch_over_fused"] = row["torch"]["ms_per_step"] / row["fused"]["ms_per_step"]
            row["torch_over_fused_eager"] = row["torch"]["ms_per_step"] / row["fused_eager"]["ms_per_step"]
        out["ar_steps"][str(T)] = row
        del routes
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
