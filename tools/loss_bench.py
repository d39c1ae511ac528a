"""cfg2 trainer step time per --loss kind (ForecasterStep(loss=...)), on one box, kinds alternating round by round.

    python tools/loss_bench.py [--steps 40] [--rounds 5] [--out profiles/losses/loss_bench.json]

Every kind gets its own Trainer (HIP-graph step, AdamW) over the same cfg2 model and batch; a round times `steps` steps of
each kind in turn (synchronize around each region), and the per-kind value is the median over rounds.  A second table does the
same for the cfg2 model with a predicted std (output_std=True): wmse there is the torch elementwise chain, nll / crps_gauss
the one-pass loss kernels."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from neural_lam_amd import graph as G  # noqa: E402
from neural_lam_amd import models as hm  # noqa: E402
from neural_lam_amd.datastore import SyntheticDatastore  # noqa: E402
from neural_lam_amd.trainer import Trainer  # noqa: E402

KINDS = ["wmse", "mse", "mae", "wmae", "nll", "crps_gauss"]


def trainers(cfg, dev, kinds, **model_kw):
    ds = SyntheticDatastore(cfg["nx"], cfg["ny"], cfg["ns"], cfg["nf"], cfg["nst"], root_path="/tmp/nlam_loss_bench",
                            boundary=cfg["boundary"], seed=0)
    ext = ds.get_xy_extent("state")
    graph = G.normalise_graph(G.create_regular_grid_graph(ds.get_xy("state"), **cfg["graph"]), max(ext[1] - ext[0], ext[3] - ext[2]))
    N, B, T = ds.num_grid_points, cfg["B"], cfg["T"]
    g = torch.Generator().manual_seed(123)
    batch = [torch.randn(B, 2, N, cfg["ns"], generator=g).to(dev), torch.randn(B, T, N, cfg["ns"], generator=g).to(dev),
             torch.randn(B, T, N, cfg["nf"] * 3, generator=g).to(dev)]
    out = {}
    for kind in kinds:
        torch.manual_seed(42)
        fc = hm.ARForecaster(hm.MODELS[cfg["model"]](ds, graph=graph, hidden_dim=cfg["d"], processor_layers=cfg["L"], **model_kw), ds)
        out[kind] = Trainer(hm.ForecasterStep(fc, ds, loss=kind).to(dev), lr=1e-3, use_graph=True)
    return out, batch


def measure(trs, batch, steps, rounds, warmup=5):
    for tr in trs.values():
        for _ in range(warmup):
            tr.step(*batch)
    torch.cuda.synchronize()
    times = {k: [] for k in trs}
    for _ in range(rounds):
        for k, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(*batch)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps * 1e3)
        assert all(bool(torch.isfinite(torch.as_tensor(float(tr.step(*batch))))) for tr in trs.values())
    return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_all": [round(x, 4) for x in v]} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS["cfg2"]
    res = {"config": "cfg2", "steps": args.steps, "rounds": args.rounds, "command": " ".join(["python", "tools/loss_bench.py", *sys.argv[1:]])}
    trs, batch = trainers(cfg, dev, KINDS)
    res["per_var_std"] = measure(trs, batch, args.steps, args.rounds)
    del trs
    torch.cuda.empty_cache()
    trs, batch = trainers(cfg, dev, ["wmse", "nll", "crps_gauss"], output_std=True)
    res["predicted_std"] = measure(trs, batch, args.steps, args.rounds)
    base = res["per_var_std"]["wmse"]["ms_median"]
    for k, v in res["per_var_std"].items():
        v["vs_wmse"] = round(v["ms_median"] / base - 1.0, 4)
        print(f"per-variable std  {k:>10}: {v['ms_median']:.4f} ms  ({100 * v['vs_wmse']:+.2f} % vs wmse)")
    base = res["predicted_std"]["wmse"]["ms_median"]
    for k, v in res["predicted_std"].items():
        v["vs_wmse"] = round(v["ms_median"] / base - 1.0, 4)
        print(f"predicted std     {k:>10}: {v['ms_median']:.4f} ms  ({100 * v['vs_wmse']:+.2f} % vs wmse, the torch chain)")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
