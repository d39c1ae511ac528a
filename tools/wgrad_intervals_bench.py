"""Step time against the number of 32-row chunks wgrad_dma_kernel requests per barrier (NLAM_TUNE_WGRAD_DMA_R).

    python tools/wgrad_intervals_bench.py --parent-tree DIR [--configs cfg2] [--arms parent,r0,r1,r2,r4] [--reps 2]
                                          [--regions 5] [--steps 40] [--out profiles/wgrad_intervals/bench.json]

The method of tools/ema_bench.py: device-synchronised timings (a host clock around ``steps`` replayed steps of the captured
training step that end in a device synchronise; ``regions`` such regions per process behind 10 warm-up steps), every
measurement a fresh process, the processes alternating over the arms, ``reps`` times inside one call, so every arm runs more
than once and its spread is known before a difference is read.  Arm ``parent`` imports bench.py and the package from DIR, an
exported tree of the parent commit with its own built library (``git archive <parent> | tar -x -C DIR``, then build inside
it); arm ``rN`` runs this tree with NLAM_WGRAD_DMA_R=N in the worker's environment (r0: the built-in choice per source
count).  A difference counts only if it exceeds the larger of the two arms' min..max spreads; the summary says so per arm.
``bench.CONFIGS`` and ``bench.build`` are used as they are, bench.py is not changed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def worker(args):
    tree = Path(args.tree).resolve()
    sys.path.insert(0, str(tree))
    import torch

    import bench
    from neural_lam_amd.trainer import Trainer

    assert Path(bench.__file__).resolve().parent == tree, (bench.__file__, tree)
    dev = torch.device("cuda:0")
    _, _, _, _, step, batch = bench.build(bench.CONFIGS[args.config], dev)
    tr = Trainer(step, lr=1e-3, use_graph=True)
    for _ in range(10):
        tr.step(*batch)
    torch.cuda.synchronize()
    regions = []
    for _ in range(args.regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step(*batch)
        torch.cuda.synchronize()
        regions.append((time.perf_counter() - t0) / args.steps * 1e3)
    assert tr._graph is not None and tr._opt_in_graph
    print("WGRAD_BENCH " + json.dumps({"regions_ms": regions}), flush=True)


def run_worker(arm, config, args):
    tree = Path(args.parent_tree) if arm == "parent" else ROOT
    env = {k: v for k, v in os.environ.items() if k != "NLAM_WGRAD_DMA_R"}
    if arm != "parent":
        env["NLAM_WGRAD_DMA_R"] = arm[1:]
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--tree", str(tree), "--config", config,
           "--regions", str(args.regions), "--steps", str(args.steps)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout, env=env)
    if out.returncode != 0:
        raise RuntimeError(f"worker {cmd} failed with {out.returncode}:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("WGRAD_BENCH ")][-1]
    return json.loads(line[len("WGRAD_BENCH "):])


def summary(runs):
    every = [x for r in runs for x in r["regions_ms"]]
    return {"median_ms": statistics.median(every), "min_ms": min(every), "max_ms": max(every),
            "spread_ms": max(every) - min(every), "process_medians_ms": [statistics.median(r["regions_ms"]) for r in runs],
            "regions_ms": [r["regions_ms"] for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--configs", default="cfg2")
    ap.add_argument("--arms", default="parent,r0,r1,r2,r4")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--worker-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    arms = args.arms.split(",")
    assert all(a == "parent" or (a[0] == "r" and a[1:] in ("0", "1", "2", "4")) for a in arms), arms
    assert "parent" not in arms or args.parent_tree, "--parent-tree DIR is needed for the parent arm"
    result = {"steps_per_region": args.steps, "regions_per_process": args.regions, "processes_per_arm": args.reps, "configs": {}}
    for config in args.configs.split(","):
        runs = {a: [] for a in arms}
        for rep in range(args.reps):
            for a in arms:   # alternating: what drifts over the call drifts under every arm
                t0 = time.perf_counter()
                runs[a].append(run_worker(a, config, args))
                print(f"{config} {a} #{rep}: {['%.4f' % x for x in runs[a][-1]['regions_ms']]} ms/step "
                      f"({time.perf_counter() - t0:.0f} s)", flush=True)
        entry = {a: summary(r) for a, r in runs.items()}
        if "parent" in entry:
            for a in arms:
                if a == "parent":
                    continue
                d = entry[a]["median_ms"] - entry["parent"]["median_ms"]
                margin = max(entry[a]["spread_ms"], entry["parent"]["spread_ms"])
                entry[a]["minus_parent_ms"], entry[a]["margin_ms"] = d, margin
                entry[a]["verdict"] = "faster" if d < -margin else ("slower" if d > margin else "within the spread")
        result["configs"][config] = entry
        print(json.dumps({config: {a: {k: v for k, v in e.items() if k != "regions_ms"} for a, e in entry.items()}}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
