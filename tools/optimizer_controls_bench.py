"""Step time of the trainer with and without the optimizer controls (max_grad_norm, lr_schedule, skip_nonfinite).

    python tools/optimizer_controls_bench.py --parent-tree DIR [--configs cfg2,cfg3] [--reps 3] [--steps 60] [--rounds 5]
                                             [--out profiles/optimizer_controls/bench.json]

Three questions, each answered with device-synchronised timings (a host clock around `steps` steps that end in a device
synchronise), variants alternating, and the spread measured before a difference is read:

* default path: `Trainer` without options on this tree against the same on DIR, an exported tree of the parent commit with its
  own built library.  Two trees are two packages, so each measurement is a fresh process; the processes alternate
  parent / this tree `reps` times and the spread is what repetitions of the SAME tree differ by.
* options on against off, on this tree, inside one process, alternating round by round; next to it the same variant
  "off" a second time (two identical trainers: the in-process spread).  The bytes predict one extra read of the flat
  gradient and one extra small launch.
* schedule (cfg2): `opt.lr` set by hand before every step -- after the second change the optimizer runs uncaptured behind the
  replay, on the parent and here alike -- against the in-graph `warmup_cosine` of this tree.

A worker (`--worker`) imports bench.py and the package from `--tree`, so the same file drives both trees; variants the
parent's package does not know are only asked of this tree.  `bench.CONFIGS` is read, bench.py is not changed."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PEAK_HBM_GBS = 8000.0   # MI355X HBM3E (bench.PEAK_HBM_GBS)


def worker(args):
    tree = Path(args.tree).resolve()
    sys.path.insert(0, str(tree))
    import torch

    import bench
    from neural_lam_amd import ops
    from neural_lam_amd.trainer import Trainer

    assert Path(bench.__file__).resolve().parent == tree, (bench.__file__, tree)
    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS[args.config]
    variants = args.variants.split(",")
    total = args.warmup + args.steps * args.rounds + args.rounds + 8

    def controls(name):
        if name in ("off", "off_again", "lr_by_hand"):
            return {}
        sch = ops.LRSchedule("warmup_cosine", warmup_steps=max(1, total // 10), total_steps=total, min_ratio=0.1)
        if name == "schedule_in_graph":
            return dict(lr_schedule=sch)
        if name == "on":
            return dict(max_grad_norm=1.0, lr_schedule=sch, skip_nonfinite=True)
        raise ValueError(name)

    trs, batch = {}, None
    for name in variants:
        _, _, _, _, step, batch = bench.build(cfg, dev)
        trs[name] = Trainer(step, lr=1e-3, use_graph=True, **controls(name))

    def run(name, n):
        tr = trs[name]
        if name == "lr_by_hand":   # what a host-driven warm-up does: a new rate in front of every step
            for _ in range(n):
                tr.opt.lr = 1e-3 * min(1.0, (tr.opt.t + 1) / total)
                tr.step(*batch)
        else:
            for _ in range(n):
                tr.step(*batch)

    for name in variants:
        run(name, args.warmup)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.steps)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"tree": str(args.label), "config": args.config, "flat_mbytes": trs[variants[0]].fp.numel * 4 / 1e6, "variants": {}}
    for name in variants:
        tr = trs[name]
        loss = float(tr.step(*batch))
        assert loss == loss, name
        out["variants"][name] = {
            "ms_median": statistics.median(times[name]), "ms_min": min(times[name]), "ms_all": [round(x, 4) for x in times[name]],
            "optimizer_captured": bool(tr._opt_in_graph or tr._tail_graph is not None or getattr(tr._graph, "tail", None) is not None),
            "optimizer_uncaptured_schedule_mode": bool(tr._opt_eager), "executor": tr.executor}
        if name in ("on", "schedule_in_graph"):
            out["variants"][name].update(grad_norm=float(tr.grad_norm), last_lr=float(tr.last_lr), skipped_steps=tr.skipped_steps)
    print("RESULT " + json.dumps(out))


def spawn(tree, label, config, variants, args):
    cmd = [sys.executable, str(Path(__file__).resolve()), "--worker", "--tree", str(tree), "--label", label, "--config", config,
           "--variants", ",".join(variants), "--steps", str(args.steps), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout, cwd=str(tree))
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"worker failed ({label}, {config}): exit {r.returncode}")   # nothing more is started on the GPU
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    print(f"{config} {label}: " + ", ".join(f"{k} {v['ms_median']:.4f} ms" for k, v in out["variants"].items()), flush=True)
    return out


def summarise(runs, config):
    """Per (tree, variant): every process's median; the spread of a variant = max - min of its processes' medians."""
    table = {}
    for r in runs:
        for name, v in r["variants"].items():
            table.setdefault((r["tree"], name), []).append(v["ms_median"])
    rows = {f"{tree}/{name}": {"ms_median_of_processes": statistics.median(v), "ms_processes": [round(x, 4) for x in v],
                               "spread_ms": round(max(v) - min(v), 4)} for (tree, name), v in table.items()}
    flat_mb = runs[0]["flat_mbytes"]
    out = {"config": config, "flat_gradient_mbytes": round(flat_mb, 3), "rows": rows,
           "predicted_extra_read_us_at_hbm_peak": round(flat_mb * 1e6 / (PEAK_HBM_GBS * 1e9) * 1e6, 2)}

    def med(key):
        return rows[key]["ms_median_of_processes"] if key in rows else None

    if med("parent/off") is not None and med("this/off") is not None:
        out["default_path"] = {"parent_ms": med("parent/off"), "this_ms": med("this/off"),
                               "difference_ms": round(med("this/off") - med("parent/off"), 4),
                               "spread_ms": max(rows["parent/off"]["spread_ms"], rows["this/off"]["spread_ms"])}
    if med("this/on") is not None:
        out["options"] = {"off_ms": med("this/off"), "off_again_ms": med("this/off_again"), "on_ms": med("this/on"),
                          "overhead_us": round((med("this/on") - med("this/off")) * 1e3, 2),
                          "in_process_spread_us": round(abs(med("this/off_again") - med("this/off")) * 1e3, 2)}
    if med("this/schedule_in_graph") is not None:
        out["schedule"] = {"parent_lr_by_hand_ms": med("parent/lr_by_hand"), "this_lr_by_hand_ms": med("this/lr_by_hand"),
                           "this_in_graph_warmup_cosine_ms": med("this/schedule_in_graph")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--label", default="this")
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--variants", default="off")
    ap.add_argument("--parent-tree", default=None, help="an exported tree of the parent commit with its library built")
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = {"command": " ".join(["python", "tools/optimizer_controls_bench.py", *sys.argv[1:]]), "steps": args.steps, "rounds": args.rounds,
           "reps": args.reps, "configs": []}
    for config in args.configs.split(","):
        mine = ["off", "on", "off_again"] + (["lr_by_hand", "schedule_in_graph"] if config == "cfg2" else [])
        theirs = ["off"] + (["lr_by_hand"] if config == "cfg2" else [])
        runs = []
        for _ in range(args.reps):
            if args.parent_tree:
                runs.append(spawn(Path(args.parent_tree).resolve(), "parent", config, theirs, args))
            runs.append(spawn(ROOT, "this", config, mine, args))
        s = summarise(runs, config)
        s["processes"] = runs
        res["configs"].append(s)
        print(json.dumps({k: v for k, v in s.items() if k != "processes"}, indent=1), flush=True)
        if args.out:   # after every config: a later failure keeps what was measured
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
