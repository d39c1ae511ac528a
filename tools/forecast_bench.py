#!/usr/bin/env python3
"""Forecast engine (neural_lam_amd/forecast.py) against the existing route, one process, alternating with warm-up.

    python tools/forecast_bench.py [--config cfg2] [--leads 40 240] [--rounds 3] [--layout plain|forecast|members]
                                   [--out profiles/forecast/bench.json]

Route "engine": ``Forecast(step, dataset, max_lead=L).run(starts)`` -- init + L replays of one recorded step, the series resident.
Route "existing": what bench.py's forecast leg does, at T = L: ``ARForecaster.forward`` under no_grad captured as ONE graph of T
steps, replayed; its pre-built inputs (forcing windows and boundary states of the whole horizon) stay outside its timing.
Per route and horizon: ms per lead time (HIP events around a synchronised window of ``--repeats`` forecasts; median over the rounds
and the rounds' spread max - min), kernel launches per lead (kernel nodes of the recorded graph / leads in it), and the peak memory
above what both routes share (the model and the resident series): for the existing route with and without its inputs.
``--layout forecast`` / ``members`` keep the engine's series as forecast-type data or with a member axis (the strided head and
init); the existing route's inputs are synthetic either way, so its numbers do not depend on the layout.
For the engine also the head and tail kernels alone: 50 launches replayed from one graph between two events, and their minimum
bytes (every float they must read or write, once) over that time.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def event_ms(fn, repeats):
    import torch

    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats


def kernel_ms(launch, n=50):
    """One launch's time: n of them recorded into one graph, replayed between two events (the Python call is longer than the kernel)."""
    import torch

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            launch()
    g.replay()
    return min(event_ms(g.replay, 1) for _ in range(5)) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--leads", type=int, nargs="+", default=[40, 240])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="forecasts per timed window")
    ap.add_argument("--verify", action="store_true", help="the engine also scores every lead (sq / ab)")
    ap.add_argument("--layout", choices=["plain", "forecast", "members"], default="plain",
                    help="the resident series: a plain analysis series, forecast-type data (analysis time, lead time, member), or an "
                         "analysis series with a member axis; the last two go through nlam_forecast_init_strided / _head_strided")
    ap.add_argument("--members", type=int, default=2, help="size of the member axis of the forecast and members layouts")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import bench
    from neural_lam_amd import _lib as L
    from neural_lam_amd.data import DeviceWeatherDataset
    from neural_lam_amd.forecast import Forecast, _kernel_nodes

    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS[args.config]
    ds, _, _, _, step, _ = bench.build(cfg, dev)
    N, F, DF, B = ds.num_grid_points, cfg["ns"], cfg["nf"], cfg["B"]
    past = fut = 1
    window = past + fut + 1
    g = torch.Generator().manual_seed(123)
    M = args.members
    kw = dict(num_past_forcing_steps=past, num_future_forcing_steps=fut, standardization=step.standardization_stats())
    if args.layout == "forecast":   # B analysis times x the lead times of the longest horizon x M members, the forcing shared
        steps = 2 + max(args.leads) + fut
        state = torch.randn(B, steps, M, N, F, generator=g).to(dev)
        forcing = torch.randn(B, steps, N, DF, generator=g).to(dev)
        data = DeviceWeatherDataset(state, forcing, None, ar_steps=max(args.leads), is_forecast=True, **kw)
    else:                           # an analysis series, with a member axis of M ("members") or without one ("plain")
        n_times = max(args.leads) + 2 + fut + 4
        member_axis = (M,) if args.layout == "members" else ()
        state = torch.randn(n_times, *member_axis, N, F, generator=g).to(dev)
        forcing = torch.randn(n_times, N, DF, generator=g).to(dev)
        data = DeviceWeatherDataset(state, forcing, None, ar_steps=1, **kw)
    strided = data.kernel != "nlam_window_batch"
    starts = torch.arange(B, dtype=torch.int64, device=dev) * data.members + (data.members - 1)   # sample b, its last member
    torch.cuda.synchronize()
    shared = torch.cuda.memory_allocated()
    out = {"config": args.config, "layout": args.layout, "members": M if strided else 1,
           "nodes": N, "state_vars": F, "forcing_vars": DF, "batch": B, "rounds": args.rounds,
           "repeats": args.repeats, "verify": args.verify, "source_stamp": L.source_stamp(), "device": torch.cuda.get_device_name(0),
           "shared_bytes": shared, "horizons": {}}

    for lead in args.leads:
        row = {}
        # ---- engine
        torch.cuda.reset_peak_memory_stats()
        fc = Forecast(step, data, lead, batch_size=B, verify=args.verify)
        fc.run(starts)
        torch.cuda.synchronize()
        row["engine"] = {"launches_per_lead": fc.launches_per_lead, "peak_bytes": torch.cuda.max_memory_allocated() - shared,
                         "output_bytes": fc.out_state.numel() * 4}
        # ---- existing route: the captured T-step rollout of bench.py's forecast leg, inputs pre-built
        torch.cuda.synchronize()
        before_inputs = torch.cuda.memory_allocated()
        init = torch.randn(B, 2, N, F, generator=g).to(dev)
        target = torch.randn(B, lead, N, F, generator=g).to(dev)
        forc = torch.randn(B, lead, N, DF * window, generator=g).to(dev)
        torch.cuda.synchronize()
        input_bytes = torch.cuda.memory_allocated() - before_inputs
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            for _ in range(2):
                step.forecaster(init, forc, target)
            torch.cuda.synchronize()
            fgraph = torch.cuda.CUDAGraph(keep_graph=True)
            t0 = time.perf_counter()
            with torch.cuda.graph(fgraph):
                step.forecaster(init, forc, target)
            nodes = _kernel_nodes(fgraph)
            fgraph.instantiate()
            record_s = time.perf_counter() - t0
        fgraph.replay()
        torch.cuda.synchronize()
        row["existing"] = {"launches_per_lead": nodes / lead, "record_seconds": record_s, "input_bytes": input_bytes,
                           "peak_bytes_without_inputs": torch.cuda.max_memory_allocated() - before_inputs - input_bytes,
                           "peak_bytes": torch.cuda.max_memory_allocated() - before_inputs}
        # ---- alternating timed rounds
        ms = {"engine": [], "existing": []}
        for _ in range(args.rounds):
            ms["engine"].append(event_ms(lambda: fc.run(starts), args.repeats) / lead)
            ms["existing"].append(event_ms(fgraph.replay, args.repeats) / lead)
        for name in ms:
            row[name].update(ms_per_lead=statistics.median(ms[name]), ms_per_lead_rounds=ms[name], spread_ms=max(ms[name]) - min(ms[name]))
        row["engine_minus_existing_ms"] = row["engine"]["ms_per_lead"] - row["existing"]["ms_per_lead"]
        row["largest_spread_ms"] = max(row["engine"]["spread_ms"], row["existing"]["spread_ms"])
        # ---- the engine's own kernels
        fc.run(starts, leads=1)
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
        delta = torch.randn(B * N, fc._p.delta_ld, generator=g).to(dev) * 0.01
        fc._p.delta = C.c_void_p(delta.data_ptr())
        if strided:
            head_ms = kernel_ms(lambda: L.check(fc._lib.nlam_forecast_head_strided(C.byref(fc._p), C.byref(fc._src), stream()),
                                                "nlam_forecast_head_strided"))
        else:
            head_ms = kernel_ms(lambda: L.check(fc._lib.nlam_forecast_head(C.byref(fc._p), stream()), "nlam_forecast_head"))
        tail_ms = kernel_ms(lambda: L.check(fc._lib.nlam_forecast_tail(C.byref(fc._p), stream()), "nlam_forecast_tail"))
        head_bytes = 2 * 4 * B * N * (F + DF * window)
        tail_bytes = 4 * B * N * (fc._p.delta_ld + 5 * F + (F if fc.has_std else 0))
        row["engine"]["kernels"] = {
            "head": {"ms": head_ms, "min_bytes": head_bytes, "gb_per_s": head_bytes / head_ms / 1e6},
            "tail": {"ms": tail_ms, "min_bytes": tail_bytes, "gb_per_s": tail_bytes / tail_ms / 1e6}}
        out["horizons"][str(lead)] = row
        del fc, fgraph, init, target, forc, delta
        torch.cuda.empty_cache()

    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
