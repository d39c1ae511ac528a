"""Step time of the trainer inside an accumulation window (``Trainer(accumulate_grad_batches=K)``) against the plain step.

    python tools/grad_accumulation_bench.py --parent-tree DIR [--configs cfg2,cfg3] [--reps 2] [--k 8] [--rounds 30]
                                            [--out profiles/grad_accumulation/bench.json]

Two questions, answered with device-synchronised timings (a host clock around steps that end in a device synchronise):

* the default: `Trainer` without the option on this tree against the same on DIR, an exported tree of the parent commit with
  its own built library.  These are the same launches.  Two trees are two packages, so every measurement is a fresh process;
  the processes alternate parent / this tree / this tree with K, `reps` times inside one call of this tool, so the parent arm
  runs more than once and its spread (what repetitions of the SAME tree differ by) is known before a difference is read.
* K micro-steps per update: the mean time of a HOLDING micro-step (the parent's forward and backward, a gated zero in place
  of the memset, three early-returning launches in place of AdamW) and of the CLOSING one (the norm of the window's
  gradient, the decision, the update).

Every arm runs the same loop: K - 1 steps between two synchronises, then one step and a synchronise.  `ms_many` is the first
interval / (K - 1), `ms_single` the second: a step timed alone carries the synchronise and is compared only with steps timed
alone.  With the option the first interval holds the K - 1 holding micro-steps and the second the closing one.

A worker (`--worker`) imports bench.py and the package from `--tree`, so the same file drives both trees.  `bench.CONFIGS` and
`bench.build` are used as they are, bench.py is not changed."""
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
    cfg = bench.CONFIGS[args.config]
    _, _, _, _, step, batch = bench.build(cfg, dev)
    kw = dict(accumulate_grad_batches=args.k) if args.accumulate else {}
    tr = Trainer(step, lr=1e-3, use_graph=True, **kw)
    for _ in range(2 * args.k):
        tr.step(*batch)
    torch.cuda.synchronize()
    many, single = [], []
    for _ in range(args.rounds):
        if args.accumulate:
            assert tr.micro_step == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.k - 1):
            tr.step(*batch)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tr.step(*batch)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        many.append((t1 - t0) / (args.k - 1) * 1e3)
        single.append((t2 - t1) * 1e3)
    loss = float(tr.step(*batch))
    assert loss == loss
    out = {"tree": args.label, "config": args.config, "accumulate": args.k if args.accumulate else 1, "executor": tr.executor,
           "updates": tr.global_step if hasattr(tr, "global_step") else tr.opt.t, "calls": 2 * args.k + args.rounds * args.k + 1,
           "ms_many": statistics.median(many), "ms_single": statistics.median(single),
           "ms_many_min": min(many), "ms_single_min": min(single),
           "optimizer_captured": bool(tr._opt_in_graph or tr._tail_graph is not None or getattr(tr._graph, "tail", None) is not None)}
    print("RESULT " + json.dumps(out))


def spawn(tree, label, config, accumulate, args):
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--tree", str(tree), "--label", label, "--config", config,
           "--k", str(args.k), "--rounds", str(args.rounds)] + (["--accumulate"] if accumulate else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout, cwd=str(tree))
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"worker failed ({label}, {config}): exit {r.returncode}")   # nothing more is started on the GPU
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1][len("RESULT "):])
    print(f"{config} {label} K={out['accumulate']}: many {out['ms_many']:.4f} ms, single {out['ms_single']:.4f} ms "
          f"({out['updates']} updates in {out['calls']} calls)", flush=True)
    return out


def summarise(runs, config, k):
    arms = {}
    for r in runs:
        arms.setdefault(f"{r['tree']}/K={r['accumulate']}", []).append(r)
    rows = {}
    for name, rs in arms.items():
        rows[name] = {q: {"median": round(statistics.median(r[q] for r in rs), 4), "processes": [round(r[q], 4) for r in rs],
                          "spread": round(max(r[q] for r in rs) - min(r[q] for r in rs), 4)} for q in ("ms_many", "ms_single")}
    out = {"config": config, "rows": rows}
    p, t1, tk = rows.get("parent/K=1"), rows.get("this/K=1"), rows.get(f"this/K={k}")
    if p and t1:
        out["default_path"] = {"parent_ms": p["ms_many"]["median"], "this_ms": t1["ms_many"]["median"],
                               "difference_ms": round(t1["ms_many"]["median"] - p["ms_many"]["median"], 4),
                               "parent_spread_ms": p["ms_many"]["spread"]}
    if p and tk:
        out["accumulation"] = {
            "holding_ms": tk["ms_many"]["median"], "parent_step_ms": p["ms_many"]["median"],
            "holding_minus_parent_ms": round(tk["ms_many"]["median"] - p["ms_many"]["median"], 4), "parent_spread_ms": p["ms_many"]["spread"],
            "closing_ms_timed_alone": tk["ms_single"]["median"], "parent_step_ms_timed_alone": p["ms_single"]["median"],
            "closing_minus_parent_ms": round(tk["ms_single"]["median"] - p["ms_single"]["median"], 4),
            "parent_spread_ms_timed_alone": p["ms_single"]["spread"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--accumulate", action="store_true")
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--label", default="this")
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--parent-tree", default=None, help="an exported tree of the parent commit with its library built")
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = {"command": " ".join(["python", "tools/grad_accumulation_bench.py", *sys.argv[1:]]), "k": args.k, "rounds": args.rounds,
           "reps": args.reps, "configs": []}
    for config in args.configs.split(","):
        runs = []
        for _ in range(args.reps):
            if args.parent_tree:
                runs.append(spawn(Path(args.parent_tree).resolve(), "parent", config, False, args))
            runs.append(spawn(ROOT, "this", config, False, args))
            runs.append(spawn(ROOT, "this", config, True, args))
        s = summarise(runs, config, args.k)
        s["processes"] = runs
        res["configs"].append(s)
        print(json.dumps({k: v for k, v in s.items() if k != "processes"}, indent=1), flush=True)
        if args.out:   # after every config: a later failure keeps what was measured
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
