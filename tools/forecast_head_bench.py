"""Kernel time of the strided forecast head alone at the cfg2 shape (window_bench.py's analysis_m2 case: 63 784 nodes, 17 state +
6 forcing variables, window 1 + 1 + 1, two members), on fp32 series (nlam_forecast_head_strided) and on the same series packed as
int16 (nlam_forecast_head_q16).  tools/forecast_bench.py times the fp32 head inside an engine; nothing else times the packed one.

Each launch is timed as 50 launches replayed from one HIP graph between two HIP events, best of 5 (window_bench.py's method).

  python tools/forecast_head_bench.py [--reps 50] [--out F.json]
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import window_bench as WB  # noqa: E402
from neural_lam_amd import _lib as L  # noqa: E402
from neural_lam_amd.forecast import dataset_source  # noqa: E402


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
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
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.load()
    res = {}
    for storage in ("float32", "int16"):
        data = WB.make("analysis_m2", dev, storage)
        nodes, ds = data.state.shape[-2:]
        df = data.forcing.shape[-1]
        truth = torch.empty(1, nodes, ds, device=dev)
        fw = torch.empty(1, nodes, df * data.window, device=dev)
        idx = torch.full((1,), 3, dtype=torch.int64, device=dev)
        lead = torch.zeros(1, dtype=torch.int32, device=dev)
        p = L.Forecast()
        p.lead, p.truth, p.forcing_windowed = _ptr(lead), _ptr(truth), _ptr(fw)
        p.state_mean, p.state_std = _ptr(data.stats["state_mean"]), _ptr(data.stats["state_std"])
        p.forcing_mean, p.forcing_std = _ptr(data.stats["forcing_mean"]), _ptr(data.stats["forcing_std"])
        p.nodes, p.d_state, p.d_forcing, p.batch = nodes, ds, df, 1
        p.max_lead, p.num_past_forcing_steps, p.num_future_forcing_steps = 1, WB.PAST, WB.FUT
        src, q = dataset_source(data, idx), data.packed_source()
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
        if storage == "int16":
            head = lambda: L.check(lib.nlam_forecast_head_q16(C.byref(p), C.byref(src), C.byref(q), stream()), "head_q16")   # noqa: E731
        else:
            head = lambda: L.check(lib.nlam_forecast_head_strided(C.byref(p), C.byref(src), stream()), "head_strided")   # noqa: E731
        res[f"head_{storage}_us"] = timed(head, args.reps)
        print(f"{storage:8s} {res[f'head_{storage}_us']:8.3f} us", flush=True)
        del data
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
