"""Time and achieved bytes/s of the standardization-statistics passes (``neural_lam_amd.stats``, ``nlam_window_moments``)
at a MEPS-shaped forecast size: 63 784 nodes, 17 state and 6 forcing variables, 65 lead times (ar_steps = 63), 2 members,
``--analysis`` analysis times (samples = analysis times x members).

Legs:
  values_state     the values pass over the 65 state rows of every sample
  values_forcing   the values pass over the 63 forcing rows of every sample
  diff_state       the standardized one-step differences (step_length 3) over the 65 state rows
  compute          compute_standardization_stats end to end (both passes, the float64 combination, one copy to the host)
  cpu_reference    compute_standardization_stats.py's loop restated in torch on the CPU (fp32, the same formulas) over
                   the first ``--cpu-samples`` samples of the same data, extrapolated to all of them

Kernel legs are timed between two HIP events around ``--reps`` back-to-back calls (best of 3); bytes come from shapes:
every element of the rows a pass reads, read once (the partial sums are < 1 % on top).  The copy rate to compare with is
the 6.29 TB/s of a float4 copy measured on MI355X.

  python tools/stats_bench.py [--analysis 4] [--reps 10] [--cpu-samples 2] [--out F.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from neural_lam_amd.data import DeviceWeatherDataset  # noqa: E402
from neural_lam_amd.stats import _moments, compute_standardization_stats  # noqa: E402

N, NS, NF, LEADS, M, AR, STEP = 238 * 268, 17, 6, 65, 2, 63, 3
COPY_TBPS = 6.29


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


def cpu_reference(state, forcing, n_samples, batch_size=32):
    """The reference's two passes over samples (s, m) in flat order, fp32 torch on the CPU."""
    def batches():
        idx = list(range(n_samples))
        for b0 in range(0, len(idx), batch_size):
            sel = idx[b0 : b0 + batch_size]
            st = torch.stack([state[i // M, :, i % M] for i in sel])   # (B, 65, N, NS)
            fo = torch.stack([forcing[i // M, 2:] for i in sel])        # (B, 63, N, NF)
            yield st[:, :2], st[:, 2:], fo

    means, squares, fmeans, fsquares = [], [], [], []
    for init, target, frc in batches():
        batch = torch.cat((init, target), dim=1)
        means.append(torch.mean(batch, dim=(1, 2)))
        squares.append(torch.mean(batch**2, dim=(1, 2)))
        fmeans.append(torch.mean(frc[..., 0]))
        fsquares.append(torch.mean(frc[..., 0] ** 2))
    mean = torch.mean(torch.cat(means), dim=0)
    std = torch.sqrt(torch.mean(torch.cat(squares), dim=0) - mean**2)
    used = (LEADS // STEP) * STEP
    dm, dq = [], []
    for init, target, _ in batches():
        batch = torch.cat(((init - mean) / std, (target - mean) / std), dim=1)
        stepped = torch.cat([batch[:, k:used:STEP] for k in range(STEP)], dim=0)
        diffs = stepped[:, 1:] - stepped[:, :-1]
        dm.append(torch.mean(diffs, dim=(1, 2)))
        dq.append(torch.mean(diffs**2, dim=(1, 2)))
    return mean, std


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--analysis", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu-samples", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(3)
    A = args.analysis
    state = torch.randn((A, LEADS, M, N, NS), device=dev, generator=g) * 3.0 + 10.0
    forcing = torch.randn((A, LEADS, N, NF), device=dev, generator=g)
    ds = DeviceWeatherDataset(state, forcing, ar_steps=AR, num_past_forcing_steps=0, num_future_forcing_steps=0, device=dev,
                              is_forecast=True)
    n = len(ds)
    res = {"shape": dict(analysis_times=A, members=M, lead_times=LEADS, nodes=N, d_state=NS, d_forcing=NF, samples=n,
                         ar_steps=AR, step_length=STEP), "copy_TBps": COPY_TBPS}
    mean = torch.zeros(NS, device=dev)
    std = torch.ones(NS, device=dev)
    legs = {
        "values_state": (lambda: _moments(ds, ds.state, 0, n, 0, AR + 2), n * (AR + 2) * N * NS * 4),
        "values_forcing": (lambda: _moments(ds, ds.forcing, 0, n, 2, AR), n * AR * N * NF * 4),
        "diff_state": (lambda: _moments(ds, ds.state, 0, n, 0, AR + 2, step=STEP, mean=mean, std=std),
                       n * ((AR + 2) // STEP) * STEP * N * NS * 4),
    }
    for name, (fn, nbytes) in legs.items():
        us = timed(fn, args.reps)
        tbps = nbytes / us * 1e-6
        res[name] = {"us": round(us, 2), "bytes": nbytes, "TBps": round(tbps, 3), "of_copy_rate": round(tbps / COPY_TBPS, 3)}
        print(name, res[name], flush=True)
    compute_standardization_stats(ds, step_length=STEP, batch_size=32)
    torch.cuda.synchronize()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        compute_standardization_stats(ds, step_length=STEP, batch_size=32)
        walls.append(time.perf_counter() - t0)
    res["compute"] = {"ms": round(min(walls) * 1e3, 3)}
    print("compute", res["compute"], flush=True)

    k = min(args.cpu_samples, n)
    if k > 0:
        a_host = (k + M - 1) // M
        st_cpu, fo_cpu = state[:a_host].cpu(), forcing[:a_host].cpu()
        t0 = time.perf_counter()
        cpu_reference(st_cpu, fo_cpu, k)
        sec = time.perf_counter() - t0
        res["cpu_reference"] = {"samples_timed": k, "s": round(sec, 3), "s_per_sample": round(sec / k, 3),
                                "s_all_samples_extrapolated": round(sec / k * n, 3), "threads": torch.get_num_threads()}
        res["speedup_vs_cpu_reference"] = round(sec / k * n / (min(walls)), 1)
        print("cpu_reference", res["cpu_reference"], flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
