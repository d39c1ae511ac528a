"""Kernel time and achieved bytes/s of the data-path launches at the cfg2 shape (bench.py's data path: B = 1, T = 1,
63 784 nodes, 17 state + 6 forcing variables, forcing window 1 + 1 + 1, standardisation folded in).

Cases:
  analysis_m1   analysis series, one member: nlam_window_batch and nlam_window_batch_ens on the same samples
  analysis_m2   analysis series, 2 members: nlam_window_batch_ens
  forecast_m2   forecast series, 2 members, 65 lead times given (3 / 4 kept resident): nlam_window_batch_ens

Every case runs on fp32 series and on the same series packed as int16 (storage="int16": nlam_window_batch_q16), back to back
in one process; --storage picks one of the two.

Each launch is timed as 50 launches replayed from one HIP graph between two HIP events (the Python call is longer than
the kernel).  Bytes come from shapes: every output float is read once (4 bytes from an fp32 series, 2 from a packed one) and
written once.  ``resident_bytes`` is what the case's series take in HBM in that storage.

  python tools/window_bench.py [--case all|analysis_m1|analysis_m2|forecast_m2] [--storage both|float32|int16] [--reps 50] [--out F.json]
Under ``rocprofv3 --kernel-trace --stats -- python tools/window_bench.py --case analysis_m1`` the two kernels of the
single-member case are listed side by side.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from neural_lam_amd.data import DeviceWeatherDataset  # noqa: E402

N, NS, NF, B, T, PAST, FUT = 238 * 268, 17, 6, 1, 1, 1, 1


def stats():
    g = torch.Generator(device="cpu").manual_seed(1)
    return {"state_mean": torch.randn(NS, generator=g), "state_std": 0.5 + torch.rand(NS, generator=g),
            "forcing_mean": torch.randn(NF, generator=g), "forcing_std": 0.5 + torch.rand(NF, generator=g)}


def time_launch(ds, idx, reps):
    outs = ds.batch(idx, standardize=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            ds.batch(idx, standardize=True, out=outs)
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    per_float = 4 + (2 if ds.storage == "int16" else 4)
    nbytes = per_float * sum(t.numel() for t in outs[:3])
    return {"kernel": ds.kernel, "storage": ds.storage, "us": best, "bytes": nbytes, "GBps": nbytes / best * 1e-3}


def make(case, dev, storage="float32"):
    gen = torch.Generator(device=dev).manual_seed(7)
    kw = dict(ar_steps=T, num_past_forcing_steps=PAST, num_future_forcing_steps=FUT, standardization=stats(), storage=storage)
    if case == "analysis_m1":
        return DeviceWeatherDataset(torch.randn(24, N, NS, device=dev, generator=gen), torch.randn(24, N, NF, device=dev, generator=gen),
                                    None, **kw)
    if case == "analysis_m2":
        return DeviceWeatherDataset(torch.randn(24, 2, N, NS, device=dev, generator=gen),
                                    torch.randn(24, 2, N, NF, device=dev, generator=gen), None, **kw)
    if case == "forecast_m2":
        A, L = 4, 65
        ds = DeviceWeatherDataset(torch.randn(A, L, 2, N, NS, device=dev, generator=gen),
                                  torch.randn(A, L, 2, N, NF, device=dev, generator=gen), None, is_forecast=True, **kw)
        torch.cuda.empty_cache()   # the 65-lead sources are gone: only the resident leads remain
        return ds
    raise ValueError(case)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all", "analysis_m1", "analysis_m2", "forecast_m2"])
    ap.add_argument("--storage", default="both", choices=["both", "float32", "int16"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = ["analysis_m1", "analysis_m2", "forecast_m2"] if args.case == "all" else [args.case]
    res = {"shape": {"nodes": N, "d_state": NS, "d_forcing": NF, "batch": B, "ar_steps": T, "window": PAST + FUT + 1},
           "device": torch.cuda.get_device_name(0), "cases": {}}
    storages = ["float32", "int16"] if args.storage == "both" else [args.storage]
    for case in cases:
        rows, resident = [], {}
        for storage in storages:
            ds = make(case, dev, storage)
            idx = ds.epoch_permutation(seed=0)[:B]
            if case == "analysis_m1" and storage == "float32":
                rows.append(time_launch(ds, idx, args.reps))
                ds.kernel = "nlam_window_batch_ens"
            rows.append(time_launch(ds, idx, args.reps))
            resident[storage] = ds.resident_bytes
            res["cases"][case] = {"resident_state": list(ds.state.shape), "resident_forcing": list(ds.forcing.shape),
                                  "len": len(ds), "launches": rows, "resident_bytes": resident}
            del ds
            torch.cuda.empty_cache()
        for r in rows:
            print(f"{case:12s} {r['storage']:8s} {r['kernel']:22s} {r['us']:8.2f} us  {r['GBps']:7.1f} GB/s  ({r['bytes'] / 1e6:.1f} MB)")
        print(f"{case:12s} resident bytes: " + ", ".join(f"{k} {v}" for k, v in resident.items()))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
