#!/usr/bin/env python3
"""What the per-lead DCT variance spectra (nlam_dct_spectra) cost inside the forecast engines, one process.

    python tools/bench_spectra.py [--config cfg2] [--members 4 16] [--leads 40] [--rounds 3] [--out profiles/spectra/bench.json]

Engines: ``Forecast(step, data, L, batch_size=1, verify=True)`` and ``EnsembleForecast(step, data, L, members=M)`` with the
configuration's GraphLAM, each with ``spectra=None``, with 2 variables and with all variables over the whole grid, alternating.
Per route: ms per lead (HIP events around a synchronised window of ``--repeats`` forecasts; median over the rounds and the rounds'
spread max - min), kernel launches per lead and peak memory.  The launch alone: 50 calls recorded into one graph and replayed
between two events; its 2 cx cy (cx + cy) flop per field over that time as a fraction of the fp32 matrix peak (157.3 TFLOP/s)."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

FP32_MATRIX_PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--members", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--leads", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2, help="forecasts per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import bench
    from forecast_bench import event_ms, kernel_ms
    from neural_lam_amd import _lib as L
    from neural_lam_amd.data import DeviceWeatherDataset
    from neural_lam_amd.forecast import EnsembleForecast, Forecast

    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS[args.config]
    ds, _, _, _, step, _ = bench.build(cfg, dev)
    N, F, DF = ds.num_grid_points, cfg["ns"], cfg["nf"]
    nx, ny = ds.nx, ds.ny
    g = torch.Generator().manual_seed(123)
    state = torch.randn(args.leads + 8, N, F, generator=g).to(dev)
    forcing = torch.randn(args.leads + 8, N, DF, generator=g).to(dev)
    data = DeviceWeatherDataset(state, forcing, None, ar_steps=1, num_past_forcing_steps=1, num_future_forcing_steps=1,
                                standardization=step.standardization_stats())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    out = {"config": args.config, "nodes": N, "grid": [nx, ny], "state_vars": F, "leads": args.leads, "rounds": args.rounds,
           "repeats": args.repeats, "source_stamp": L.source_stamp(), "device": torch.cuda.get_device_name(0), "engines": {}}
    variants = {"none": None, "two": [0, F // 2], "all": list(range(F))}

    for label, M in [("forecast", 0)] + [(f"ensemble_M{m}", m) for m in args.members]:
        engines, row = {}, {}
        for vname, spectra in variants.items():
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            kw = dict(spectra=spectra, grid_shape=(nx, ny))
            eng = (Forecast(step, data, args.leads, batch_size=1, verify=True, **kw) if M == 0
                   else EnsembleForecast(step, data, args.leads, members=M, **kw))
            run = lambda e=eng: e.run([0])   # noqa: E731
            run()
            torch.cuda.synchronize()
            engines[vname] = (eng, run)
            row[vname] = {"launches_per_lead": eng.launches_per_lead, "peak_bytes": torch.cuda.max_memory_allocated() - before}
        ms = {name: [] for name in engines}
        for _ in range(args.rounds):
            for name, (_, run) in engines.items():
                ms[name].append(event_ms(run, args.repeats) / args.leads)
        for name in ms:
            row[name].update(ms_per_lead=statistics.median(ms[name]), ms_per_lead_rounds=ms[name], spread_ms=max(ms[name]) - min(ms[name]))
        for name in ("two", "all"):   # the launch alone (the counter at 0: it writes slot 0)
            eng = engines[name][0]
            eng.run([0], leads=1)
            eng.lead.zero_()
            sp = eng._sp
            t_ms = kernel_ms(lambda: L.check(eng._lib.nlam_dct_spectra(C.byref(sp), stream()), "nlam_dct_spectra"))
            fields = sum(sp.src[k].batch for k in range(sp.sources)) * sp.vars
            flop = 2.0 * sp.cx * sp.cy * (sp.cx + sp.cy) * fields
            row[name]["launch_alone"] = {"ms": t_ms, "fields": fields, "flop": flop, "tflops": flop / t_ms / 1e9,
                                         "fraction_of_fp32_matrix_peak": flop / (t_ms * 1e-3) / FP32_MATRIX_PEAK}
            row[name]["minus_none_ms"] = row[name]["ms_per_lead"] - row["none"]["ms_per_lead"]
        out["engines"][label] = row
        del engines
        torch.cuda.empty_cache()

    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
