#!/usr/bin/env python3
"""Ensemble engine (neural_lam_amd/forecast.py, EnsembleForecast) against the deterministic engine, one process, alternating.

    python tools/ensemble_bench.py [--config cfg2] [--members 4 16] [--leads 40] [--rounds 3] [--out profiles/ensemble/bench.json]
    python tools/ensemble_bench.py --kernels-only      # under rocprofv3 --kernel-trace --stats: the two launches alone
    python tools/ensemble_bench.py --products [--kernels-only] [--out profiles/ensemble_products/bench.json]
    python tools/ensemble_bench.py --neighbourhoods [0 1 2 5 10] [--out profiles/ensemble_neighbourhood/bench.json]

Route "forecast": ``Forecast(step, data, L, batch_size=M, verify=True).run([start] * M)`` with the configuration's GraphLAM.
Route "ensemble": ``EnsembleForecast(step, data, L, members=M).run([start])`` with the same predictor: the same batch, the same
network, plus nlam_ens_scores and its finishing pass per lead (no sampling launch: the predictor is deterministic).
Route "efm": the engine with a GraphEFMMultiScale on the configuration's graph and width, in absolute terms.
Per route: ms per lead (HIP events around a synchronised window of ``--repeats`` forecasts; median over the alternating rounds and
the rounds' spread max - min), kernel launches per lead and peak memory above what the routes share (model and resident series).
The two new launches alone: 50 of them recorded into one graph and replayed between two events, with their minimum bytes
(nlam_ens_scores: 4 S N F (M + 3) + 8 S N F; nlam_latent_sample: parameters in, latent out) over that time.
``--products`` adds the route "ensemble_products": the "ensemble" engine with 4 events and 3 quantile levels (nlam_ens_products and
its finishing pass per lead), alternating with the others, and times that launch pair alone against its minimum bytes
(4 S N F (M + 1) + 4 S N (E + Q F)).  Without the option the run is what it was.
``--neighbourhoods [radii]`` (default 0 1 2 5 10; it implies ``--products``) adds the route "ensemble_neighbourhood": the
"ensemble_products" engine with those window radii on the configuration's grid (nlam_ens_neighbourhood, five more launches per
lead), alternating with the others, and times that launch alone beside nlam_ens_products.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--members", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--leads", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2, help="forecasts per timed window")
    ap.add_argument("--kernels-only", action="store_true", help="launch nlam_ens_scores and nlam_latent_sample alone (for a kernel trace)")
    ap.add_argument("--products", action="store_true", help="add the route with 4 events and 3 quantiles, and time nlam_ens_products alone")
    ap.add_argument("--neighbourhoods", type=int, nargs="*", default=None, metavar="RADIUS",
                    help="add the route with neighbourhood probabilities and the FSS at these radii (default 0 1 2 5 10) on top of --products")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.neighbourhoods is not None:
        args.products = True
        args.neighbourhoods = args.neighbourhoods or [0, 1, 2, 5, 10]

    import torch

    import bench
    from forecast_bench import event_ms, kernel_ms
    from neural_lam_amd import _lib as L
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm
    from neural_lam_amd.data import DeviceWeatherDataset
    from neural_lam_amd.forecast import EnsembleForecast, Forecast

    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS[args.config]
    ds, graph, _, _, step, _ = bench.build(cfg, dev)
    N, F, DF = ds.num_grid_points, cfg["ns"], cfg["nf"]
    n_times = args.leads + 8
    g = torch.Generator().manual_seed(123)
    state = torch.randn(n_times, N, F, generator=g).to(dev)
    forcing = torch.randn(n_times, N, DF, generator=g).to(dev)
    data = DeviceWeatherDataset(state, forcing, None, ar_steps=1, num_past_forcing_steps=1, num_future_forcing_steps=1,
                                standardization=step.standardization_stats())
    torch.manual_seed(42)
    efm = graph_efm.GraphEFMMultiScale(ds, graph=graph, hidden_dim=cfg["d"])
    efm_step = hm.ForecasterStep(hm.ARForecaster(efm, ds), ds, standardize=True).to(dev)
    torch.cuda.synchronize()
    shared = torch.cuda.memory_allocated()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    out = {"config": args.config, "nodes": N, "state_vars": F, "leads": args.leads, "rounds": args.rounds, "repeats": args.repeats,
           "source_stamp": L.source_stamp(), "device": torch.cuda.get_device_name(0), "shared_bytes": shared, "members": {}}

    for M in args.members:
        row = {}
        engines = {}
        routes = [("forecast", lambda: Forecast(step, data, args.leads, batch_size=M, verify=True)),
                  ("ensemble", lambda: EnsembleForecast(step, data, args.leads, members=M)),
                  ("efm", lambda: EnsembleForecast(efm_step, data, args.leads, members=M))]
        if args.products:   # standardised data: thresholds around the bulk and in the tails, the median and the 10 % / 90 % envelope
            events = [(0, ">", 0.0), (0, "<", -1.0), (F // 2, ">", 1.5), (F - 1, "<", 0.5)]
            routes.append(("ensemble_products", lambda: EnsembleForecast(step, data, args.leads, members=M, events=events,
                                                                         quantiles=[0.1, 0.5, 0.9])))
        if args.neighbourhoods:
            routes.append(("ensemble_neighbourhood", lambda: EnsembleForecast(step, data, args.leads, members=M, events=events,
                                                                              quantiles=[0.1, 0.5, 0.9], neighbourhoods=args.neighbourhoods,
                                                                              grid_shape=(ds.nx, ds.ny))))
        for name, make in routes:
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            eng = make()
            run = (lambda e=eng: e.run([0] * M)) if name == "forecast" else (lambda e=eng: e.run([0]))
            if args.kernels_only and name == "forecast":
                continue
            run()
            torch.cuda.synchronize()
            engines[name] = (eng, run)
            row[name] = {"launches_per_lead": eng.launches_per_lead, "peak_bytes": torch.cuda.max_memory_allocated() - before}
        if not args.kernels_only:
            ms = {name: [] for name in engines}
            for _ in range(args.rounds):
                for name, (_, run) in engines.items():
                    ms[name].append(event_ms(run, args.repeats) / args.leads)
            for name in ms:
                row[name].update(ms_per_lead=statistics.median(ms[name]), ms_per_lead_rounds=ms[name], spread_ms=max(ms[name]) - min(ms[name]))
            row["ensemble_minus_forecast_ms"] = row["ensemble"]["ms_per_lead"] - row["forecast"]["ms_per_lead"]
            row["efm"]["ms_per_lead_and_member"] = row["efm"]["ms_per_lead"] / M
        # the two launches alone (the counter at 0: they write slot 0)
        ens, efm_eng = engines["ensemble"][0], engines["efm"][0]
        ens.run([0], leads=1)
        ens.lead.zero_()
        scores_ms = kernel_ms(lambda: L.check(ens._lib.nlam_ens_scores(C.byref(ens._e), stream()), "nlam_ens_scores"))
        scores_bytes = 4 * N * F * (M + 3) + 8 * N * F
        efm_eng.run([0], leads=1)
        efm_eng.lead.zero_()
        params = torch.randn(M, efm_eng._s.rows, efm_eng._s.latent_dim * (2 if efm_eng._s.diagonal else 1), generator=g).to(dev)
        efm_eng._s.params = C.c_void_p(params.data_ptr())
        sample_ms = kernel_ms(lambda: L.check(efm_eng._lib.nlam_latent_sample(C.byref(efm_eng._s), stream()), "nlam_latent_sample"))
        sample_bytes = 4 * (params.numel() + efm_eng.latent.numel())
        row["kernels"] = {"ens_scores_and_finish": {"ms": scores_ms, "min_bytes": scores_bytes, "gb_per_s": scores_bytes / scores_ms / 1e6},
                          "latent_sample": {"ms": sample_ms, "min_bytes": sample_bytes, "gb_per_s": sample_bytes / sample_ms / 1e6,
                                            "rows": efm_eng._s.rows, "latent_dim": efm_eng._s.latent_dim}}
        if args.products:
            pe = engines["ensemble_products"][0]
            pe.run([0], leads=1)
            pe.lead.zero_()
            prod_ms = kernel_ms(lambda: L.check(pe._lib.nlam_ens_products(C.byref(pe._pr), stream()), "nlam_ens_products"))
            prod_bytes = 4 * N * F * (M + 1) + 4 * N * (pe._pr.events + pe._pr.quantiles * F)
            row["kernels"]["ens_products_and_finish"] = {"ms": prod_ms, "min_bytes": prod_bytes, "gb_per_s": prod_bytes / prod_ms / 1e6,
                                                         "events": pe._pr.events, "quantiles": pe._pr.quantiles}
            if not args.kernels_only:
                row["products_minus_ensemble_ms"] = row["ensemble_products"]["ms_per_lead"] - row["ensemble"]["ms_per_lead"]
            del pe
        if args.neighbourhoods:
            ne = engines["ensemble_neighbourhood"][0]
            ne.run([0], leads=1)
            ne.lead.zero_()
            nbr_ms = kernel_ms(lambda: L.check(ne._lib.nlam_ens_neighbourhood(C.byref(ne._nb), stream()), "nlam_ens_neighbourhood"))
            nbr_bytes = 4 * N * F * (M + 1) + 4 * N * ne._nb.events * ne._nb.scales
            row["kernels"]["ens_neighbourhood"] = {"ms": nbr_ms, "min_bytes": nbr_bytes, "gb_per_s": nbr_bytes / nbr_ms / 1e6,
                                                   "events": ne._nb.events, "radii": list(args.neighbourhoods),
                                                   "grid": [ds.nx, ds.ny]}
            if not args.kernels_only:
                row["neighbourhood_minus_products_ms"] = row["ensemble_neighbourhood"]["ms_per_lead"] - row["ensemble_products"]["ms_per_lead"]
            del ne
        out["members"][str(M)] = row
        del engines, ens, efm_eng
        torch.cuda.empty_cache()

    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
