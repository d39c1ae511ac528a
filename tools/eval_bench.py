"""Evaluation (validation_step / test_step) cost on the MI355X: the nlam_eval_metrics kernel pair against the reference's torch
metric chain, alone and inside the eval step.

    python tools/eval_bench.py [--reps 50] [--rounds 5] [--out profiles/eval/eval_bench.json]     # timings (events, no profiler)
    rocprofv3 --kernel-trace --stats -d OUT -o eval -- python tools/eval_bench.py --part kernels  # kernel times, a run of its own
    python tools/eval_bench.py --part roofline --stats OUT/.../eval_kernel_stats.csv               # kernel time vs HBM roofline

Shapes: the MEPS-shaped metric pass alone (B = 1, T = 10, N = 63 784, F = 17; per-variable std with wmse, per-entry std with
nll), and the cfg2 model (GraphLAM d = 64, L = 4, the same grid) with a rollout of 10 steps, phase "test", steps_to_log
(1, 5, 10), eager ``ForecasterStep.evaluate`` / ``trainer.graphed_eval_step`` / the rollout followed by the torch chain.
The torch chain is test_step's (models/module.py:491-504, :607-665): the loss with the boolean interior mask, metrics.mse and
metrics.mae (sum_vars=False), the spatial loss with NaN written off the interior, the mean predicted std -- each a pass of its
own over (B, T, N, F), each boolean index a host synchronisation.  Variants alternate round by round; medians are reported."""
import argparse
import csv
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

B, T, F = 1, 10, 17
STEPS_TO_LOG = (1, 5, 10)
HBM_BYTES_PER_S = 6.29e12   # measured float4 copy rate (the practical HBM roof of the MI355X)


def meps_inputs(dev, N):
    g = torch.Generator().manual_seed(7)
    pred = torch.randn(B, T, N, F, generator=g).to(dev)
    target = torch.randn(B, T, N, F, generator=g).to(dev)
    std = (torch.nn.functional.softplus(torch.randn(B, T, N, F, generator=g)) + 0.05).to(dev)
    var_std = (torch.rand(F, generator=g) + 0.5).to(dev)
    interior = torch.ones(N, dtype=torch.bool)
    interior[torch.randperm(N, generator=g)[: N // 20]] = False
    return pred, target, std, var_std, interior.to(dev)


def min_bytes(N, per_entry):
    """inputs read once (pred, target, the per-entry std or F stds, the N row weights), outputs written once."""
    n = B * T * N * F
    reads = (3 if per_entry else 2) * n + (0 if per_entry else F) + N
    writes = B * T + 2 * B * T * F + (B * T * F if per_entry else 0) + B * len(STEPS_TO_LOG) * N
    return 4 * (reads + writes)


def torch_chain(prediction, target, pred_std, interior, kind, steps_to_log):
    """test_step's metric chain (module.py:491-504, :607-665) with the reference formulas (models.get_metric / mse / mae)."""
    from neural_lam_amd import models as hm

    loss = hm.get_metric(kind)
    time_step_loss = torch.mean(loss(prediction, target, pred_std, mask=interior), dim=0)
    mean_loss = torch.mean(time_step_loss)
    mse = hm.mse(prediction, target, pred_std, mask=interior, sum_vars=False)
    mae = hm.mae(prediction, target, pred_std, mask=interior, sum_vars=False)
    out_std = torch.mean(pred_std[..., interior, :], dim=-2) if pred_std.dim() == 4 else None
    spatial = loss(prediction, target, pred_std, average_grid=False)
    spatial[..., ~interior] = float("nan")
    maps = spatial[:, [s - 1 for s in steps_to_log if s <= spatial.shape[1]]]
    return time_step_loss, mean_loss, mse, mae, out_std, maps


def timed(fns, reps, rounds, warmup=5):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / reps * 1e3)
    return {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_all": [round(x, 4) for x in v]}
            for k, v in times.items()}


def metric_fns(dev, N):
    from neural_lam_amd.ops import eval_metrics

    pred, target, std, var_std, interior = meps_inputs(dev, N)
    rw = interior.float() / interior.float().sum()
    maps = [s - 1 for s in STEPS_TO_LOG]
    return {
        "kernel_per_var_std_wmse": lambda: eval_metrics(pred, target, None, var_std, rw, "wmse", maps, want_mae=True),
        "kernel_per_entry_std_nll": lambda: eval_metrics(pred, target, std, None, rw, "nll", maps, want_mae=True, want_std=True),
        "torch_per_var_std_wmse": lambda: torch_chain(pred, target, var_std, interior, "wmse", STEPS_TO_LOG),
        "torch_per_entry_std_nll": lambda: torch_chain(pred, target, std, interior, "nll", STEPS_TO_LOG),
    }


def eval_step_fns(dev):
    import bench
    from neural_lam_amd import graph as G
    from neural_lam_amd import models as hm
    from neural_lam_amd.datastore import SyntheticDatastore
    from neural_lam_amd.trainer import graphed_eval_step

    cfg = bench.CONFIGS["cfg2"]
    ds = SyntheticDatastore(cfg["nx"], cfg["ny"], cfg["ns"], cfg["nf"], cfg["nst"],
                            root_path=tempfile.mkdtemp(prefix="nlam_eval_bench_"), boundary=cfg["boundary"], seed=0)
    ext = ds.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state"), **cfg["graph"]), max(ext[1] - ext[0], ext[3] - ext[2]))
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(123)
    batch = [torch.randn(B, 2, N, cfg["ns"], generator=g).to(dev), torch.randn(B, T, N, cfg["ns"], generator=g).to(dev),
             torch.randn(B, T, N, cfg["nf"] * 3, generator=g).to(dev)]
    torch.manual_seed(42)
    fc = hm.ARForecaster(hm.MODELS[cfg["model"]](ds, graph=graph, hidden_dim=cfg["d"], processor_layers=cfg["L"]), ds)
    step = hm.ForecasterStep(fc, ds).to(dev)
    graphed = graphed_eval_step(step, *batch, phase="test", steps_to_log=STEPS_TO_LOG)

    def torch_step():
        with torch.no_grad():
            prediction, _ = step.forecaster(batch[0], batch[2], batch[1])
            return torch_chain(prediction, batch[1], step.per_var_std, step.interior_mask_bool, "wmse", STEPS_TO_LOG)

    def rollout():
        with torch.no_grad():
            return step.forecaster(batch[0], batch[2], batch[1])

    # the three routes agree (the graph bit for bit with eager; the torch chain to fp32 summation order)
    e, gr, tc = step.evaluate(*batch, phase="test", steps_to_log=STEPS_TO_LOG), graphed(*batch), torch_step()
    assert torch.equal(e.mean_loss, gr.mean_loss) and torch.equal(e.entry_mse, gr.entry_mse)
    assert abs(float(e.mean_loss) - float(tc[1])) <= 1e-5 * abs(float(tc[1]))
    return {
        "rollout_only": rollout,
        "evaluate_eager": lambda: step.evaluate(*batch, phase="test", steps_to_log=STEPS_TO_LOG),
        "evaluate_graphed": lambda: graphed(*batch),
        "rollout_plus_torch_chain": torch_step,
    }, N


def roofline(stats_path, N):
    """kernel_stats.csv of rocprofv3 --stats: average ns per launch of each eval kernel -> the pair's time per pass and its
    fraction of the HBM roofline on the minimum bytes."""
    rows = list(csv.DictReader(open(stats_path)))
    avg = {r["Name"]: float(r["AverageNs"]) for r in rows if "eval_" in r["Name"]}
    finish = sum(v for k, v in avg.items() if "eval_finish_kernel" in k)
    out = {}
    for name, per_entry in (("per_var_std_wmse", False), ("per_entry_std_nll", True)):
        tmpl = f"<{5 if per_entry else 3}, {'true' if per_entry else 'false'}>"
        part = [v for k, v in avg.items() if "eval_partials_kernel" in k and tmpl in k]
        if not part:
            continue
        us = (part[0] + finish) / 1e3
        nbytes = min_bytes(N, per_entry)
        out[name] = {"partials_us": round(part[0] / 1e3, 2), "finish_us": round(finish / 1e3, 2), "pair_us": round(us, 2),
                     "min_bytes": nbytes, "achieved_TBps": round(nbytes / (us * 1e-6) / 1e12, 3),
                     "fraction_of_6.29TBps": round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["timing", "kernels", "roofline"], default="timing")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv (--part roofline)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N = 238 * 268   # the cfg2 / MEPS grid
    if args.part == "roofline":
        print(json.dumps(roofline(args.stats, N), indent=1))
        return
    dev = torch.device("cuda:0")
    if args.part == "kernels":   # under rocprofv3: the two kernel variants, a fixed number of launches each
        fns = metric_fns(dev, N)
        for k in ("kernel_per_var_std_wmse", "kernel_per_entry_std_nll"):
            for _ in range(args.reps):
                fns[k]()
        torch.cuda.synchronize()
        return
    # the command that produced the numbers, without where they were written
    cmd = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out") and not a.startswith("--out=")]
    res = {"command": " ".join(["python", "tools/eval_bench.py", *cmd]), "shape": {"B": B, "T": T, "N": N, "F": F},
           "steps_to_log": list(STEPS_TO_LOG), "reps": args.reps, "rounds": args.rounds,
           "min_bytes": {"per_var_std": min_bytes(N, False), "per_entry_std": min_bytes(N, True)}}
    res["metric_pass"] = timed(metric_fns(dev, N), args.reps, args.rounds)
    torch.cuda.empty_cache()
    fns, _ = eval_step_fns(dev)
    res["eval_step_cfg2_T10"] = timed(fns, max(1, args.reps // 5), args.rounds)
    for part in ("metric_pass", "eval_step_cfg2_T10"):
        for k, v in res[part].items():
            print(f"{part:>20} {k:>26}: {v['ms_median']:.4f} ms")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
