"""Step time of clamped and predicted-std models with their tail inside the step-tail pass (ops.StepTailExtFunction) and on
the torch-op route it replaces (``NLAM_FUSED_CLAMPED_TAIL=0``).

    python tools/clamped_tail_bench.py [--parent-tree DIR] [--models plain,std,clamp,both] [--reps 2] [--regions 5] [--steps 40]
                                       [--count-launches] [--out profiles/clamped_tail/bench.json]

cfg2-size GraphLAM (``bench.CONFIGS["cfg2"]`` shapes and inputs, ``Trainer(use_graph=True)``) as four models:
``plain`` (bench.py's own model), ``std`` (``output_std=True``, loss nll), ``clamp`` (clamps on three of the 17 variables, one
per mode, loss wmse) and ``both`` (the two together, loss nll).  Three arms, each a fresh process, alternating ``reps`` times so
that the spread of an arm (what repetitions of the SAME arm differ by) is known before a difference is read:

* ``parent``: DIR, an exported tree of the parent commit with its own built library (``git archive <parent> | tar -x -C DIR``,
  then build inside it); it has only the torch-op route;
* ``off``: this tree with the switch off; ``on``: this tree with it on.

Timings are device-synchronised (a host clock around ``steps`` replayed steps that end in a device synchronise; ``regions`` such
regions per process behind 10 warm-up steps).  ``--count-launches`` adds, for ``both``, the kernels per replayed step of the
``off`` and ``on`` arms from a torch.profiler kernel trace of five steps.  bench.py is used as it is."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
MODELS = {"plain": (False, False, "wmse"), "std": (True, False, "nll"), "clamp": (False, True, "wmse"), "both": (True, True, "nll")}


def build(bench, cfg, dev, output_std, clamps, loss):
    """bench.build's datastore, graph, seeds and batch, with the extra model kwargs."""
    import torch

    from neural_lam_amd import models as hm

    ds, graph, _, forecaster, step, batch = bench.build(cfg, dev)
    if not output_std and not clamps:
        return step, batch
    names = ds.get_vars_names("state")
    kw = dict(output_std=output_std)
    if clamps:   # one variable per mode: lower, both, upper (un-standardised limits around the synthetic statistics)
        kw.update(output_clamping_lower={names[0]: -3.0, names[5]: -4.0}, output_clamping_upper={names[5]: 4.0, names[11]: 3.0})
    torch.manual_seed(42)
    predictor = hm.MODELS[cfg["model"]](ds, graph=graph, hidden_dim=cfg["d"], processor_layers=cfg["L"], **kw)
    step = hm.ForecasterStep(hm.ARForecaster(predictor, ds), ds, standardize=True, loss=loss).to(dev)
    return step, batch


def worker(args):
    tree = Path(args.tree).resolve()
    sys.path.insert(0, str(tree))
    import torch

    import bench
    from neural_lam_amd.trainer import Trainer

    assert Path(bench.__file__).resolve().parent == tree, (bench.__file__, tree)
    dev = torch.device("cuda:0")
    step, batch = build(bench, bench.CONFIGS["cfg2"], dev, *MODELS[args.model])
    tr = Trainer(step, lr=1e-3, use_graph=True)
    for _ in range(10):
        tr.step(*batch)
    torch.cuda.synchronize()
    assert tr._graph is not None
    out = {"executor": tr.executor}
    if args.count_launches:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                tr.step(*batch)
            torch.cuda.synchronize()
        kernels = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and not e.name.startswith(("Memcpy", "Memset"))]
        out["kernels_per_step"] = len(kernels) / 5
    regions = []
    for _ in range(args.regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.step(*batch)
        torch.cuda.synchronize()
        regions.append((time.perf_counter() - t0) / args.steps * 1e3)
    out["regions_ms"] = regions
    print("TAIL_BENCH " + json.dumps(out), flush=True)


def run_worker(tree, model, fused, count, args):
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--tree", str(tree), "--model", model,
           "--regions", str(args.regions), "--steps", str(args.steps)] + (["--count-launches"] if count else [])
    env = dict(os.environ, NLAM_FUSED_CLAMPED_TAIL="1" if fused else "0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout, env=env)
    if out.returncode != 0:
        raise RuntimeError(f"worker {cmd} failed with {out.returncode}:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("TAIL_BENCH ")][-1]
    return json.loads(line[len("TAIL_BENCH "):])


def summary(runs):
    every = [x for r in runs for x in r["regions_ms"]]
    s = {"median_ms": statistics.median(every), "min_ms": min(every), "max_ms": max(every),
         "process_medians_ms": [statistics.median(r["regions_ms"]) for r in runs], "regions_ms": [r["regions_ms"] for r in runs]}
    if "kernels_per_step" in runs[0]:
        s["kernels_per_step"] = runs[0]["kernels_per_step"]
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--model", default="both", choices=sorted(MODELS))
    ap.add_argument("--count-launches", action="store_true")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--models", default="plain,std,clamp,both")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--worker-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    result = {"steps_per_region": args.steps, "regions_per_process": args.regions, "processes_per_arm": args.reps, "models": {}}
    for model in args.models.split(","):
        arms = {"off": (ROOT, False), "on": (ROOT, True)}
        if args.parent_tree:
            arms = {"parent": (Path(args.parent_tree), False), **arms}
        if model == "plain":   # the switch does not reach a plain model: its two arms are the parent's tree and this one
            arms.pop("off")
        runs = {name: [] for name in arms}
        for rep in range(args.reps):
            for name, (tree, fused) in arms.items():   # alternating: what drifts over the call drifts under every arm
                t0 = time.perf_counter()
                count = args.count_launches and model == "both" and name != "parent" and rep == 0
                runs[name].append(run_worker(tree, model, fused, count, args))
                print(f"{model} {name} #{rep}: {['%.4f' % x for x in runs[name][-1]['regions_ms']]} ms/step "
                      f"({time.perf_counter() - t0:.0f} s)", flush=True)
        entry = {name: summary(r) for name, r in runs.items()}
        for name in arms:
            entry[f"{name}_spread_ms"] = entry[name]["max_ms"] - entry[name]["min_ms"]
        if "off" in entry:
            entry["on_minus_off_ms"] = entry["on"]["median_ms"] - entry["off"]["median_ms"]
        if "parent" in entry:
            entry["on_minus_parent_ms"] = entry["on"]["median_ms"] - entry["parent"]["median_ms"]
        result["models"][model] = entry
        print(json.dumps({model: {k: v for k, v in entry.items() if not isinstance(v, dict)}}), flush=True)
        if args.out:   # after every model: a call that is cut short keeps what it measured
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
