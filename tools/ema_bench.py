"""Step time of the trainer with and without the moving average of the weights (``Trainer(ema_decay=...)``).

    python tools/ema_bench.py [--parent-tree DIR] [--configs cfg2,cfg3] [--reps 2] [--regions 5] [--steps 40]
                              [--out profiles/ema/bench.json]

Two questions, answered with device-synchronised timings (a host clock around ``steps`` replayed steps that end in a device
synchronise; ``regions`` such regions per process behind 10 warm-up steps):

* the default path: ``Trainer`` without the option on this tree against the same on DIR, an exported tree of the parent
  commit with its own built library (``git archive <parent> | tar -x -C DIR``, then build inside it).  These are the same
  launches; equality within the spread is expected.  The parent arm runs at the first of ``--configs`` only.
* the option: the same step with ``ema_decay=0.999``, whose update launch reads and writes 8 more bytes per parameter.

Two trees are two packages, so every measurement is a fresh process; the processes alternate parent / off / on, ``reps`` times
inside one call of this tool, so every arm runs more than once and its spread (what repetitions of the SAME arm differ by) is
known before a difference is read.  A worker (``--worker``) imports bench.py and the package from ``--tree``, so the same
file drives both trees.  ``bench.CONFIGS`` and ``bench.build`` are used as they are, bench.py is not changed."""
import argparse
import json
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
    kw = dict(ema_decay=0.999) if args.ema else {}
    tr = Trainer(step, lr=1e-3, use_graph=True, **kw)
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
    print("EMA_BENCH " + json.dumps({"regions_ms": regions, "params": int(tr.fp.numel), "executor": tr.executor}), flush=True)


def run_worker(tree, config, ema, args):
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--tree", str(tree), "--config", config,
           "--regions", str(args.regions), "--steps", str(args.steps)] + (["--ema"] if ema else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout)
    if out.returncode != 0:
        raise RuntimeError(f"worker {cmd} failed with {out.returncode}:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("EMA_BENCH ")][-1]
    return json.loads(line[len("EMA_BENCH "):])


def summary(runs):
    every = [x for r in runs for x in r["regions_ms"]]
    return {"median_ms": statistics.median(every), "min_ms": min(every), "max_ms": max(every),
            "process_medians_ms": [statistics.median(r["regions_ms"]) for r in runs], "regions_ms": [r["regions_ms"] for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--worker-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    configs = args.configs.split(",")
    result = {"steps_per_region": args.steps, "regions_per_process": args.regions, "processes_per_arm": args.reps, "configs": {}}
    for ci, config in enumerate(configs):
        arms = {"off": (ROOT, False), "on": (ROOT, True)}
        if args.parent_tree and ci == 0:
            arms = {"parent": (Path(args.parent_tree), False), **arms}
        runs = {name: [] for name in arms}
        for rep in range(args.reps):
            for name, (tree, ema) in arms.items():   # alternating: what drifts over the call drifts under every arm
                t0 = time.perf_counter()
                runs[name].append(run_worker(tree, config, ema, args))
                print(f"{config} {name} #{rep}: {['%.4f' % x for x in runs[name][-1]['regions_ms']]} ms/step "
                      f"({time.perf_counter() - t0:.0f} s)", flush=True)
        entry = {name: summary(r) for name, r in runs.items()}
        entry["params"] = runs["off"][0]["params"]
        entry["executor"] = runs["off"][0]["executor"]
        entry["extra_bytes_per_update"] = 8 * entry["params"]
        entry["overhead_ms"] = entry["on"]["median_ms"] - entry["off"]["median_ms"]
        entry["off_spread_ms"] = entry["off"]["max_ms"] - entry["off"]["min_ms"]
        if "parent" in entry:
            entry["off_minus_parent_ms"] = entry["off"]["median_ms"] - entry["parent"]["median_ms"]
            entry["parent_spread_ms"] = entry["parent"]["max_ms"] - entry["parent"]["min_ms"]
        result["configs"][config] = entry
        print(json.dumps({config: {k: v for k, v in entry.items() if not isinstance(v, dict)}}), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
