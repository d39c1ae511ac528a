#!/usr/bin/env python
"""bench.py -- training-step throughput of the GraphCast-LAM hot path on MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``: for N > 1 either
launched under torch.distributed.run (one rank per GPU over RCCL), or on its own, in
which case it re-launches itself that way (127.0.0.1 rendezvous, free port).  W untimed
warm-up steps, then exactly K training steps bracketed by barrier +
synchronize; the max over ranks is the job time; rank 0 prints ONE JSON line.
``--dump-outputs DIR`` writes what the last timed step computed to DIR/*.npy (see dump_outputs).
A plain run does only that: set up, warm up, time, dump, print.  Everything else it can measure or
check -- the legs and baselines listed below, forecast throughput, the loss on the initial weights --
runs only under ``--full`` (that loss before the warm-up, the rest after the timed steps and the
dump); the ``--no-*`` options thin a ``--full`` run.

A step = ``ForecasterModule.training_step``-equivalent on one pre-resident
synthetic batch per GPU: standardised inputs -> AR rollout
(ar_steps) through GraphLAM -> masked wmse -> backward -> gradient all-reduce
(N > 1) -> AdamW.  Workload at N = 1 = BASELINE.json configs[1]: GraphCast-LAM
multiscale mesh on the synthetic MEPS-shaped 238x268 grid, 17 state variables,
hidden_dim 64, 4 processor layers, batch 1 per GPU, ar_steps 1, fp32.

Launch mode: zero-grad + forward + loss + backward are captured once into a HIP
graph and replayed per step (the gradient all-reduce for N > 1 and the fused AdamW
run after each replay); ``--eager`` issues every launch from Python instead.

Extra objects on the JSON line (``--full``; a plain run prints ``roofline`` as null and leaves out the rest):
  forecast_steps_per_s
                inference rollouts (no grad) per second, same launch mode as the training step.
  roofline      per launch shape (HIP events on the launch stream, second instrumented
                eager pass): algorithmic FLOPs and HBM bytes, the matrix instruction
                actually issued, frac = max(executed MFMA FLOPs / dense peak of THAT
                instruction, algorithmic bytes / 8 TB/s).  The top-level fields are the
                dominant launch (largest share of the step); "kernels" lists the top
                six, "step" the whole-step totals; "traffic" = PMC-measured HBM bytes
                per launch (profiles/round3/pmc_traffic.json, tools/pmc_collect.py).
  cpu_baseline  the oracle (pure-torch restatement of the reference) timed on this
                box's host cores on the same workload (median of >= 10 steps).
  gpu_reference_equivalent
                the same restatement run on cuda:0 through stock PyTorch-ROCm ops (eager,
                autograd, torch.optim.AdamW), with and without
                torch.use_deterministic_algorithms: the "reference PyG-CUDA-equivalent"
                step time the >= 5x target of BASELINE.json is measured against.
  oracle_loss_step0 / loss_step0
                the CPU oracle's loss and the HIP path's loss on the initial weights.
  from_device_dataset, lightning_shaped, also
                the same step fed by the HBM-resident dataset, the Lightning-shaped loop, the wide
                configurations (cfg3 / cfg5 at N = 1, cfg3 at N > 1).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (no sparsity)
PEAK_HBM_GBS = 8000.0

CONFIGS = {
    # name: (nx, ny, n_state, n_forcing, n_static, hidden, proc_layers, ar_steps, batch_per_gpu, model, graph kwargs)
    "cfg2": dict(nx=238, ny=268, ns=17, nf=6, nst=4, d=64, L=4, T=1, B=1, model="graph_lam",
                 graph=dict(n_max_levels=None, hierarchical=False), boundary="frame"),
    "cfg1": dict(nx=64, ny=64, ns=5, nf=2, nst=1, d=16, L=4, T=1, B=2, model="graph_lam",
                 graph=dict(n_max_levels=1, hierarchical=False), boundary="random"),
    # the other BASELINE.json configs, one sample per GPU (not the default bench line; numbers go to profiles/)
    "cfg3": dict(nx=238, ny=268, ns=17, nf=6, nst=4, d=256, L=8, T=4, B=1, model="graph_lam",
                 graph=dict(n_max_levels=None, hierarchical=False), boundary="frame"),
    "cfg4": dict(nx=238, ny=268, ns=17, nf=6, nst=4, d=128, L=4, T=1, B=1, model="hi_lam",
                 graph=dict(n_max_levels=3, hierarchical=True), boundary="frame"),
    "cfg4p": dict(nx=238, ny=268, ns=17, nf=6, nst=4, d=128, L=4, T=1, B=1, model="hi_lam_parallel",
                  graph=dict(n_max_levels=3, hierarchical=True), boundary="frame"),
    "cfg5": dict(nx=238, ny=268, ns=17, nf=6, nst=4, d=512, L=8, T=8, B=1, model="graph_lam",
                 graph=dict(n_max_levels=None, hierarchical=False), boundary="frame"),
}


def build(cfg, device, seed_offset=0, oracle=False):
    from neural_lam_amd import graph as G
    from neural_lam_amd.datastore import SyntheticDatastore

    ds = SyntheticDatastore(cfg["nx"], cfg["ny"], cfg["ns"], cfg["nf"], cfg["nst"], root_path="/tmp/nlam_bench",
                            boundary=cfg["boundary"], seed=0)
    ext = ds.get_xy_extent("state")
    raw = G.create_regular_grid_graph(ds.get_xy("state"), **cfg["graph"])
    graph = G.normalise_graph(raw, max(ext[1] - ext[0], ext[3] - ext[2]))
    torch.manual_seed(42)  # weights: default init under seed 42
    if oracle:
        from oracle import models as om

        predictor = om.MODELS[cfg["model"]](ds, graph, hidden_dim=cfg["d"], processor_layers=cfg["L"])
        forecaster = om.ARForecaster(predictor, ds)
        step = None
    else:
        from neural_lam_amd import models as hm

        predictor = hm.MODELS[cfg["model"]](ds, graph=graph, hidden_dim=cfg["d"], processor_layers=cfg["L"])
        forecaster = hm.ARForecaster(predictor, ds)
        step = hm.ForecasterStep(forecaster, ds, standardize=True).to(device)   # the step starts with on_after_batch_transfer
    N, B, T = ds.num_grid_points, cfg["B"], cfg["T"]
    g = torch.Generator().manual_seed(123 + seed_offset)  # inputs ~ N(0,1), seed 123 (+rank)
    init = torch.randn(B, 2, N, cfg["ns"], generator=g)
    target = torch.randn(B, T, N, cfg["ns"], generator=g)
    forcing = torch.randn(B, T, N, cfg["nf"] * 3, generator=g)
    batch = tuple(t.to(device) for t in (init, target, forcing))
    return ds, graph, raw, forecaster, step, batch


def cpu_baseline_sample(cfg, threads=32):
    """The wide configurations (cfg3 / cfg4 / cfg5: 10-200 s per oracle step on the host) on a BOUNDED sample: one training
    step of the same model with ONE autoregressive step of the rollout (same graph, weights, widths; ar_steps 1 of the
    T), one warm-up + one timed step, fixed thread count.  The metric counts B x T sample-steps per training step, so the
    per-sample-step rate of the sample is directly comparable with `value`."""
    from oracle import models as om

    ncpu = os.cpu_count() or 1
    threads = max(1, min(threads, ncpu))
    ds, _, _, forecaster, _, batch = build(cfg, torch.device("cpu"), oracle=True)
    batch = (batch[0], batch[1][:, :1].contiguous(), batch[2][:, :1].contiguous())
    pvs, mask = om.per_var_std_uniform(ds), om.interior_mask_bool(ds)
    opt = torch.optim.AdamW(forecaster.parameters(), lr=1e-3, betas=(0.9, 0.95))
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    times = []
    try:
        for it in range(2):
            t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            _, loss = om.training_loss(forecaster, om.standardize_batch(ds, *batch), pvs, mask)
            loss.backward()
            opt.step()
            times.append(time.perf_counter() - t0)
            if times[-1] > 45.0:   # the warm-up alone used the budget: it is the sample
                break
    finally:
        torch.set_num_threads(old)
    t = times[-1]
    return {
        "value": cfg["B"] * 1 / t,
        "unit": "sample-steps/s",
        "ms_per_step": t * 1e3,
        "cores": threads,
        "kind": "port",
        "sample": f"ONE training step with ar_steps 1 of the {cfg['T']} (same model, graph, weights; B x 1 sample-steps), "
                  f"{'second of two steps' if len(times) > 1 else 'single step (no warm-up: it alone took > 45 s)'}, oracle = PyG-free torch "
                  f"fp32 restatement of the reference, torch.set_num_threads({threads}) on a {ncpu}-core host",
    }


def cpu_baseline(cfg, budget_s=30.0):
    """Oracle training step (fwd + wmse + bwd + AdamW) on the host cores: median of >= 10 steps."""
    from oracle import models as om

    if cfg["d"] > 64:
        return cpu_baseline_sample(cfg)
    ncpu = os.cpu_count() or 1
    ds, _, _, forecaster, _, batch = build(cfg, torch.device("cpu"), oracle=True)
    pvs, mask = om.per_var_std_uniform(ds), om.interior_mask_bool(ds)
    opt = torch.optim.AdamW(forecaster.parameters(), lr=1e-3, betas=(0.9, 0.95))

    def one():
        opt.zero_grad(set_to_none=True)
        _, loss = om.training_loss(forecaster, om.standardize_batch(ds, *batch), pvs, mask)
        loss.backward()
        opt.step()

    # torch's CPU scatter/index_add paths degrade badly when oversubscribed on a
    # many-core host: probe a few thread counts (one step each) and keep the best.
    best, cores = None, 1
    for n in sorted({min(ncpu, c) for c in (8, 16, 32, 64)}):
        torch.set_num_threads(n)
        t0 = time.perf_counter()
        one()
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, cores = dt, n
        if time.perf_counter() - t0 > budget_s / 3:
            break
    torch.set_num_threads(cores)
    for _ in range(3):
        one()  # warm-ups (>= 3)
    times = []
    t_start = time.perf_counter()
    while len(times) < 12 and (len(times) < 3 or (time.perf_counter() - t_start) < budget_s):
        t0 = time.perf_counter()
        one()
        times.append(time.perf_counter() - t0)
    med = sorted(times)[len(times) // 2]
    return {
        "value": cfg["B"] * cfg["T"] / med,
        "unit": "sample-steps/s",
        "ms_per_step": med * 1e3,
        "cores": cores,
        "kind": "port",
        "sample": f"{len(times)} full training steps of the same workload (median; 3 warm-ups), oracle = PyG-free torch fp32 "
                  f"restatement of the reference, torch.set_num_threads({cores}) = best of a {{8,16,32,64}}-thread probe "
                  f"on a {ncpu}-core host",
    }


def gpu_reference_equivalent(cfg, device, steps=20, autocast=False, budget_s=4.0):
    """BASELINE.md section 4 / north_star ">= 5x the reference PyG-CUDA-equivalent step time": the reference's
    formulation -- gather (index_select) -> cat -> Linear -> SiLU -> Linear -> LayerNorm -> index_add_, un-fused,
    autograd, torch.optim.AdamW -- through stock PyTorch-ROCm ops on THIS GPU, same weights and batch, eager (the
    reference trains eagerly under Lightning) with and without ``torch.use_deterministic_algorithms(True)``
    (the reference sets ``deterministic=True``, train_model.py:566).  PyG itself is not installable here, so the
    "reference-equivalent" is the oracle restatement moved to the device; it is a reported baseline, never part of
    the product path."""
    from oracle import models as om

    out = {"what": "oracle restatement of the reference on cuda:0 through stock PyTorch-ROCm ops (eager, autograd, "
                   "torch.optim.AdamW), same weights / batch as the timed workload; loss_first_step = its loss on the initial weights"
                   + ("; inside torch.autocast(bfloat16), as Lightning --precision bf16-mixed runs the reference" if autocast else ""),
           "steps": steps}
    for name, det in (("nondeterministic", False), ("deterministic", True)):
        ds, _, _, forecaster, _, batch = build(cfg, torch.device("cpu"), oracle=True)   # fresh seed-42 weights per mode
        forecaster = forecaster.to(device)
        batch = tuple(b.to(device) for b in batch)
        pvs, mask = om.per_var_std_uniform(ds).to(device), om.interior_mask_bool(ds).to(device)
        st = ds.get_standardization_dataarray("state")
        fs = ds.get_standardization_dataarray("forcing")
        eps = torch.finfo(torch.float32).eps
        s_mean = torch.tensor(st.state_mean.values, dtype=torch.float32, device=device)
        s_std = torch.clamp(torch.tensor(st.state_std.values, dtype=torch.float32, device=device), min=eps)
        window = batch[2].shape[-1] // max(1, len(fs.forcing_mean.values))
        f_mean = torch.tensor(fs.forcing_mean.values, dtype=torch.float32, device=device).repeat_interleave(window)
        f_std = torch.clamp(torch.tensor(fs.forcing_std.values, dtype=torch.float32, device=device), min=eps).repeat_interleave(window)
        opt = torch.optim.AdamW(forecaster.parameters(), lr=1e-3, betas=(0.9, 0.95))

        def one():
            opt.zero_grad(set_to_none=True)
            b = ((batch[0] - s_mean) / s_std, (batch[1] - s_mean) / s_std, (batch[2] - f_mean) / f_std)   # on_after_batch_transfer
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                _, loss = om.training_loss(forecaster, b, pvs, mask)
            loss.backward()
            opt.step()
            return loss.detach()

        try:
            torch.use_deterministic_algorithms(det)
            first = float(one())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            one()
            torch.cuda.synchronize()
            nsteps = max(2, min(steps, int(budget_s / max(time.perf_counter() - t0, 1e-4))))   # ~budget_s of timed steps per mode
            one()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(nsteps):
                one()
            torch.cuda.synchronize()
            out[f"ms_per_step_{name}"] = (time.perf_counter() - t0) / nsteps * 1e3
            out[f"steps_{name}"] = nsteps
            out[f"loss_first_step_{name}"] = first
        except Exception as exc:   # an op without a deterministic implementation on this build
            out[f"ms_per_step_{name}"] = None
            out[f"error_{name}"] = repr(exc)[:200]
        finally:
            torch.use_deterministic_algorithms(False)
        del forecaster, opt
    return out


def lightning_shaped(cfg, device, steps, precision="fp32"):
    """The step a neural-lam maintainer gets after swapping the two import sites of INTEGRATION.md level 1 and nothing else:
    the HIP modules driven the way ``pl.Trainer`` drives ``ForecasterModule`` (models/module.py:394-417, train_model.py:564-578) --
    ``optimizer.zero_grad()``; ``loss = training_step(batch)``; ``loss.backward()``; ``torch.optim.AdamW(betas=(0.9, 0.95)).step()``
    (module.py:293-304) -- every launch issued from Python, gradients owned by autograd (``AccumulateGrad`` hooks fire, which is
    what torch DDP needs), no flat buffers, no fused optimizer.  Timed twice: as it is (``eager``), and with
    ``trainer.graphed_training_step`` inside ``training_step`` (forward and backward each one HIP-graph replay; the optimizer
    still torch's).  Reported beside ``value``, never as it."""
    import gc

    from neural_lam_amd.trainer import graphed_training_step

    out = {"what": "HIP modules under a Lightning-shaped loop: zero_grad + training_step + loss.backward() + torch.optim.AdamW(lr=1e-3, betas=(0.9, 0.95)).step(), "
                   "gradients through autograd; eager = every launch from Python; graphed = trainer.graphed_training_step (forward and backward one "
                   "HIP-graph replay each, weight gradients on side streams inside the backward graph, optimizer unchanged); graphed_fused_adamw = the same with torch.optim.AdamW(fused=True)"}
    amp = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16")   # noqa: E731
    out["what"] += ("; graphed_flat = graphed_training_step(..., flat=True): the parameters are views of ONE flat leaf, autograd gets one gradient, "
                    "torch.optim.AdamW([step.flat_parameter]) (the same element-wise update; one AccumulateGrad instead of ~130)")
    for name in ("eager", "graphed", "graphed_fused_adamw", "graphed_flat", "graphed_flat_fused_adamw"):
        _, _, _, _, step, batch = build(cfg, device)
        # (the reference constructs torch.optim.AdamW with its defaults, models/module.py:293-304: the multi-tensor "foreach"
        # implementation, ~1 ms of host time per step for ~130 parameter tensors; fused=True is the same optimizer as one kernel)
        fn = step
        if name != "eager":
            with amp():
                fn = graphed_training_step(step, *batch, flat="flat" in name)
        opt = torch.optim.AdamW([fn.flat_parameter] if "flat" in name else step.parameters(), lr=1e-3, betas=(0.9, 0.95),
                                fused=True if name.endswith("fused_adamw") else None)

        def one():
            opt.zero_grad(set_to_none=True)
            with amp():
                _, loss = fn(*batch)
            loss.backward()
            opt.step()
            return loss

        for _ in range(3):
            one()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one()
        torch.cuda.synchronize()
        n = max(3, min(steps, int(2.0 / max(time.perf_counter() - t0, 1e-4))))   # ~2 s of timed steps
        t0 = time.perf_counter()
        for _ in range(n):
            loss = one()
        torch.cuda.synchronize()
        out[f"ms_per_step_{name}_torch_adamw"] = (time.perf_counter() - t0) / n * 1e3
        out[f"steps_{name}"] = n
        out[f"final_loss_{name}"] = float(loss)
        del step, opt, fn, one, loss
        gc.collect()   # the captured callable and its replay function reference each other
        torch.cuda.empty_cache()
    return out


def oracle_loss_step0(cfg, device=None):
    """Loss of the oracle on the benchmark's own weights and batch (forward only, fp32): printed beside the HIP loss.  On the
    host for cfg1 / cfg2; the wide configurations (minutes and tens of GB on the host) run the same restatement on ``device``."""
    from oracle import models as om

    ds, _, _, forecaster, _, batch = build(cfg, torch.device("cpu"), oracle=True)
    pvs, mask = om.per_var_std_uniform(ds), om.interior_mask_bool(ds)
    batch = om.standardize_batch(ds, *batch)
    if device is not None and cfg["d"] > 64:
        forecaster, batch, pvs, mask = forecaster.to(device), tuple(b.to(device) for b in batch), pvs.to(device), mask.to(device)
    with torch.no_grad():
        _, loss = om.training_loss(forecaster, batch, pvs, mask)
    return float(loss)


DUMP_BYTES_MAX = 64_000_000


def dump_outputs(out_dir, trainer, loss):
    """--dump-outputs: what the last timed step computed, as a caller of the training step holds it afterwards -- the loss,
    the parameters after the optimizer update and the gradients of that step -- written as float32 .npy files, so that two
    builds run with the same arguments (same seeded graph, weights and batch) can be compared output for output.  Parameters
    and gradients are concatenated in the module's registration order (``module.parameters()``), without the flat buffer's
    alignment padding.  When both would exceed DUMP_BYTES_MAX together, the same fixed, seeded sample of positions is kept
    from each and its positions are written to params_sample_index.npy (float64, exact below 2**53)."""
    import numpy as np

    fp = trainer.fp
    views = [(fp.offsets[i], p.numel()) for i, p in enumerate(fp.params)]
    params = torch.cat([fp.flat[o : o + n] for o, n in views]).float().cpu()
    grads = torch.cat([fp.grad[o : o + n] for o, n in views]).float().cpu()
    arrays = {"loss": loss.detach().float().reshape(1).cpu().numpy()}
    n = params.numel()
    keep = (DUMP_BYTES_MAX - 4096) // (4 + 4 + 8)
    if 8 * n > DUMP_BYTES_MAX - 4096:
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:keep].sort().values
        params, grads = params[idx], grads[idx]
        arrays["params_sample_index"] = idx.numpy().astype(np.float64)
    arrays["params"] = params.numpy()
    arrays["grads"] = grads.numpy()
    out_dir.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        np.save(out_dir / f"{name}.npy", a)


def kernel_rooflines(recs, meta, step_ms, traffic):
    """Per-launch roofline records from the instrumented eager pass (HIP events on the launch stream).

    For each launch shape: algorithmic FLOPs and bytes (ops.py computes them from the call geometry), the matrix
    instruction actually issued, and
        mfma_frac = executed MFMA FLOPs / (avg time * dense peak of THAT instruction type)
                    (bf16x3 = 6 bf16 MFMAs per product block against 2.5 PFLOP/s; fp32 MFMA against 157.3 TFLOP/s),
        hbm_frac  = MINIMUM algorithmic bytes (`algorithmic_bytes_min`: inputs once, outputs once) / (avg time * 8 TB/s);
                    `algorithmic_bytes` / `hbm_frac_incl_saved_and_partials` = the same plus what this implementation moves on top
                    (tensors saved for backward, dz1 / dz2 handed to the weight-gradient launch, partial sums),
        frac      = max(mfma_frac, hbm_frac), bound = whichever is larger.
    """
    rows = []
    for key, times in recs.items():
        m = meta.get(key)
        if m is None or not times:
            continue
        avg_ms = sum(times) / len(times)
        per_step = len(times)   # divided by the number of instrumented steps by the caller
        t = avg_ms * 1e-3
        if m["mfmas_per_block"]:
            exe, peak, inst = m["flops"] * m["mfmas_per_block"], PEAK_BF16_MFMA_TFLOPS, "v_mfma_f32_32x32x16_bf16"
        else:
            exe, peak, inst = m["flops"], PEAK_FP32_MFMA_TFLOPS, "v_mfma_f32_32x32x2_f32"
        mfma_frac = exe / t / 1e12 / peak
        bmin = m.get("bytes_min", m["bytes"])   # inputs once, outputs once (no partial sums, no dz1 / dz2, no saved tensors)
        hbm_frac = bmin / t / 1e9 / PEAK_HBM_GBS
        hbm_frac_incl = m["bytes"] / t / 1e9 / PEAK_HBM_GBS
        rows.append({
            "launch": "%s rows=%d %s" % (key[0], key[1], "x".join(str(k) for k in key[2:5] if not isinstance(k, bool))),
            "what": m["what"], "matmul_mode": m["mm"], "mfma_instruction": inst,
            "launches": per_step, "avg_launch_ms": avg_ms, "total_ms": avg_ms * per_step,
            "algorithmic_flops": m["flops"], "executed_mfma_flops": exe,
            "algorithmic_tflops": m["flops"] / t / 1e12, "executed_tflops": exe / t / 1e12, "mfma_peak_tflops": peak,
            "mfma_frac": mfma_frac, "algorithmic_bytes_min": bmin, "hbm_GBps": bmin / t / 1e9, "hbm_frac": hbm_frac,
            "algorithmic_bytes": m["bytes"], "hbm_GBps_incl_saved_and_partials": m["bytes"] / t / 1e9, "hbm_frac_incl_saved_and_partials": hbm_frac_incl,
            "bound": "mfma" if mfma_frac >= hbm_frac else "hbm", "frac": max(mfma_frac, hbm_frac),
            "traffic": traffic.get(":".join(str(k) for k in key[:4])) if traffic else None,
        })
    rows.sort(key=lambda r: -r["total_ms"])
    return rows


def also_leg(name, precision, device, rank, world, args, timed_regions, reference=True):
    """One more BASELINE configuration on the same clock as `value`: build it, 2 warm-up steps, a region
    of <= 10 steps under the same barrier + synchronize contract (median of up to five regions below 0.5 s, as for `value`),
    then -- at world 1 -- the same-GPU reference-equivalent (stock PyTorch-ROCm ops, eager / deterministic) on its weights and
    batch, a few steps each.  Reported under "also"; `value` stays cfg2."""
    import gc

    from neural_lam_amd.trainer import Trainer

    cfg = CONFIGS[name]
    t_leg = time.perf_counter()
    _, _, raw, _, step, batch = build(cfg, device, seed_offset=rank)
    amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16")
    amp.__enter__()
    try:
        tr = Trainer(step, lr=1e-3, use_graph=not args.eager)
        k = max(2, min(args.steps, 10))
        for _ in range(2):
            tr.step(*batch)
        regions, loss = timed_regions(tr, batch, k)
    finally:
        amp.__exit__(None, None, None)
    el = sorted(regions)[len(regions) // 2]
    from neural_lam_amd import ops

    out = {"value": world * cfg["B"] * cfg["T"] * k / el, "unit": "sample-steps/s", "ms_per_step": el / k * 1e3,
           "steps": k, "warmup": 2, "n_gpus": world, "scaling": "weak", "dtype": "f32" if precision == "fp32" else "bf16",
           "matmul_mode": ops.matmul_mode_name() if precision == "fp32" else "bf16 (autocast)",
           "executor": tr.executor, "regions_ms": [x * 1e3 for x in regions], "final_loss": float(loss),
           "config": {"workload": f"{name}: {cfg['model']}, grid {cfg['nx']}x{cfg['ny']}, hidden_dim {cfg['d']}, {cfg['L']} processor layers, "
                                  f"ar_steps {cfg['T']}, batch {cfg['B']}/GPU", "global_batch": world * cfg["B"], "parallelism": f"dp{world}"}}
    del tr, step, batch, loss
    gc.collect()
    torch.cuda.empty_cache()
    if reference and world == 1:
        g = gpu_reference_equivalent(cfg, device, steps=4, autocast=precision == "bf16", budget_s=1.5)
        for kk in ("nondeterministic", "deterministic"):
            v = g.get(f"ms_per_step_{kk}")
            g[f"speedup_vs_{kk}"] = (v / out["ms_per_step"]) if v else None
        g.pop("what", None)
        out["gpu_reference_equivalent"] = g
        gc.collect()
        torch.cuda.empty_cache()
    out["leg_wall_s"] = time.perf_counter() - t_leg
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)   # ~2 ms steps: a timed region of >= 0.5 s
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--full", action="store_true",
                    help="also run every other leg: the loss on the initial weights (before the warm-up) and, after the timed "
                         "steps, forecast throughput, the HBM-resident data path, per-launch rooflines, the Lightning-shaped loop, the wide "
                         "configurations under 'also', the CPU and same-GPU baselines (the --no-* options below leave legs out)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle leg")
    ap.add_argument("--no-gpu-baseline", action="store_true", help="with --full: skip the same-GPU stock-PyTorch leg")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the instrumented per-launch pass")
    ap.add_argument("--no-data-path", action="store_true", help="with --full: skip the leg that trains from the HBM-resident dataset")
    ap.add_argument("--no-lightning-leg", action="store_true", help="with --full: skip the Lightning-shaped (eager / graphed + torch AdamW) leg")
    ap.add_argument("--no-also", action="store_true", help="with --full: skip the cfg3 / cfg5 legs reported under 'also'")
    ap.add_argument("--eager", action="store_true", help="issue every launch from Python instead of replaying a HIP graph")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"],
                    help="bf16 = run the step inside torch.autocast(bfloat16), as Lightning --precision bf16-mixed does (cfg5)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (loss, updated parameters, their gradients) "
                         "as DIR/<name>.npy, e.g. --dump-outputs bench_outputs")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    cfg = CONFIGS[args.config]

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: re-launch under torch.distributed.run, one rank per GPU of this node
        # (the reference's launch mode, train_model.py:564-578 / README.md:486-514); rank 0 of that job prints the JSON
        # line on the inherited stdout.  Under an external torchrun WORLD_SIZE is set and this branch is skipped.
        import socket
        import subprocess

        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on these hosts (RCCL needs it)
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve()), *sys.argv[1:]]
        raise SystemExit(subprocess.call(cmd, env=env))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} ranks (WORLD_SIZE={world})")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback); CPU numbers come from the cpu_baseline leg only")
    # dry run of the N > 1 code on a 1-GPU box: NLAM_BENCH_DRYRUN=1 puts every rank on cuda:0 over gloo (numbers are
    # meaningless then; it only checks the multi-rank control flow)
    dryrun = os.environ.get("NLAM_BENCH_DRYRUN") == "1"
    if dryrun:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    ranks_seen = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if dryrun:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)  # "nccl" is RCCL on ROCm
        probe = torch.ones(1, device=device)
        dist.all_reduce(probe)          # every rank contributes 1: the collective really spans `world` ranks
        ranks_seen = int(probe.item())

    from neural_lam_amd import ops
    from neural_lam_amd.trainer import Trainer

    ds, graph, raw, forecaster, step, batch = build(cfg, device, seed_offset=rank)
    amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=args.precision == "bf16")
    amp.__enter__()   # whole run (capture included) inside the autocast region; exited before the baselines
    loss_step0 = None
    if args.full:
        with torch.no_grad():   # loss on the initial weights, for the parity line against the oracle
            loss_step0 = float(step(*batch)[1])
    trainer = Trainer(step, lr=1e-3, use_graph=not args.eager)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_regions(tr, b, steps, max_regions=5):
        """Regions of EXACTLY `steps` training steps, each bracketed by barrier + synchronize, a region's time = the max over
        ranks.  One region is the contract; when it lasts under 0.5 s (20 steps of cfg2 are 35 ms: one scheduling hiccup is
        3 %) more follow, up to `max_regions`, and the MEDIAN region is reported, all of them listed.  Every rank takes the
        same decision: it is made on the all-reduced time.  The headline measurement passes max_regions=1, so that
        --steps is the number of timed steps."""
        regions, last = [], None
        while True:
            sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                last = tr.step(*b)
            sync()
            el = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([el], device=device, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                el = float(t)
            regions.append(el)
            if (len(regions) == 1 and el >= 0.5) or len(regions) >= max_regions:
                return regions, last

    for _ in range(args.warmup):
        trainer.step(*batch)
    regions, loss = timed_regions(trainer, batch, args.steps, max_regions=1)
    elapsed = regions[0]
    ms_per_step = elapsed / args.steps * 1e3
    value = world * cfg["B"] * cfg["T"] * args.steps / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(Path(args.dump_outputs), trainer, loss)

    launch_mode = "eager" if args.eager else (
        "hip_graph, one-graph executor (zero-grad + fwd + loss + bwd [+ AdamW at world 1] captured once, weight gradients as forked branches; "
        "on_after_batch_transfer writes the graph's inputs before; at world > 1 the all-reduce and the optimizer's own graph follow each replay)"
        if trainer.executor == "forks" else
        "hip_graph, segmented executor (the chain -- zero-grad, fwd, loss, data gradients -- as linear graphs replayed back to back on one stream, "
        f"weight gradients as graphs on side streams behind per-segment events, {trainer.forks_per_segment} fork points per segment; the optimizer's "
        "graph behind the join; at world > 1 gradient buckets are all-reduced per segment)")
    out = {
        "metric": "training sample-steps/s (on_after_batch_transfer+fwd+wmse+bwd+allreduce+AdamW), GraphCast-LAM, MEPS-shaped grid",
        "value": value,
        "unit": "sample-steps/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "timed_regions_ms": [x * 1e3 for x in regions],   # one region of exactly `steps` steps: value / ms_per_step come from it
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32" if args.precision == "fp32" else "bf16",
        "matmul_mode": ops.matmul_mode_name() if args.precision == "fp32" else "bf16 (autocast)",
        "data": "synthetic",
        "launch_mode": launch_mode,
        "rccl_ranks_seen": ranks_seen,
        "final_loss": float(loss),
        "config": {
            "workload": f"{args.config}: {cfg['model']}, grid {cfg['nx']}x{cfg['ny']} ({ds.num_grid_points} nodes), "
                        f"{cfg['ns']} state vars, hidden_dim {cfg['d']}, {cfg['L']} processor layers, "
                        f"ar_steps {cfg['T']}, batch {cfg['B']}/GPU, g2m/m2m/m2g edges "
                        f"{raw['g2m_edge_index'].shape[1]}/{raw['m2m_edge_index'][0].shape[1]}/{raw['m2g_edge_index'].shape[1]}",
            "global_batch": world * cfg["B"],
            "parallelism": f"dp{world}",
        },
        "roofline": None,   # --full: the instrumented per-launch pass
    }
    if not args.full:   # a plain run ends here: its headline figure and nothing else
        amp.__exit__(None, None, None)
        if rank == 0:
            print(json.dumps(out))
        if world > 1:
            dist.destroy_process_group()
        return

    # N > 1: BASELINE configs[2] (GraphLAM d = 256, 8 layers, ar_steps 4, one sample per GPU) is the configuration the
    # 0.9-efficiency target is written for; it is timed as well (same contract, fewer steps) and reported under "also".
    # (N = 1: the wide configurations are timed further down, after the cfg2 legs have released their trainer: `also_wide`.)
    also = None
    if world > 1 and args.config == "cfg2" and os.environ.get("NLAM_BENCH_ALSO", "1") == "1":
        also = {"cfg3": also_leg("cfg3", "fp32", device, rank, world, args, timed_regions, reference=False)}

    # forecast throughput (inference rollout, no grad), reported alongside; same launch mode as training
    fsteps = min(args.steps, 200)
    with torch.no_grad():
        for _ in range(2):
            step.forecaster(batch[0], batch[2], batch[1])
        torch.cuda.synchronize()
        if args.eager:
            run_forecast = lambda: step.forecaster(batch[0], batch[2], batch[1])  # noqa: E731
        else:
            fgraph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(fgraph):
                step.forecaster(batch[0], batch[2], batch[1])
            run_forecast = fgraph.replay
        run_forecast()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(fsteps):
            run_forecast()
        torch.cuda.synchronize()
        fc_elapsed = time.perf_counter() - t0
    forecast_steps_per_s = world * cfg["B"] * cfg["T"] * fsteps / fc_elapsed

    # the same step fed by the data path: samples cut from an HBM-resident series by nlam_window_batch with
    # on_after_batch_transfer folded in, written straight into the captured step's input buffers -- reported beside
    # `value`, which stays the reference-shaped step (a batch handed over on the device)
    data_path = None
    if world == 1 and not args.no_data_path and not args.eager and args.precision == "fp32":
        from neural_lam_amd import models as hm
        from neural_lam_amd.data import DeviceWeatherDataset

        ds2, _, _, fc2, _, _ = build(cfg, device, seed_offset=rank)
        step2 = hm.ForecasterStep(fc2, ds2, standardize=False).to(device)
        tr2 = Trainer(step2, lr=1e-3, use_graph=True)
        n_times, N = 24, ds2.num_grid_points
        gg = torch.Generator(device=device).manual_seed(7)
        series_state = torch.randn(n_times, N, cfg["ns"], device=device, generator=gg)
        series_forcing = torch.randn(n_times, N, cfg["nf"], device=device, generator=gg)
        dset = DeviceWeatherDataset(series_state, series_forcing, None, ar_steps=cfg["T"], num_past_forcing_steps=1,
                                    num_future_forcing_steps=1, standardization=step2.standardization_stats())
        perm = dset.epoch_permutation(seed=0)
        nb = len(dset) // cfg["B"]
        for k in range(args.warmup):
            tr2.step_from(dset, perm[(k % nb) * cfg["B"] : (k % nb + 1) * cfg["B"]])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            tr2.step_from(dset, perm[(k % nb) * cfg["B"] : (k % nb + 1) * cfg["B"]])
        torch.cuda.synchronize()
        dp_ms = (time.perf_counter() - t0) / args.steps * 1e3
        # the window launch alone: HIP events, algorithmic bytes = every output float read once and written once
        idx = perm[: cfg["B"]]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        outs = dset.batch(idx, standardize=True)
        torch.cuda.synchronize()
        wg = torch.cuda.CUDAGraph()   # 50 launches replayed back to back: the Python call (~30 us) is longer than the kernel
        with torch.cuda.graph(wg):
            for _ in range(50):
                dset.batch(idx, standardize=True, out=outs)
        wg.replay()
        e0.record()
        wg.replay()
        e1.record()
        torch.cuda.synchronize()
        w_us = e0.elapsed_time(e1) / 50 * 1e3
        w_bytes = 2 * 4 * sum(t.numel() for t in outs[:3])
        data_path = {"ms_per_step": dp_ms, "samples": "DeviceWeatherDataset: %d-step series resident in HBM, window 1+1+1, indices from a resident permutation" % n_times,
                     "window_launch_us": w_us, "window_algorithmic_bytes": w_bytes, "window_GBps": w_bytes / w_us * 1e-3,
                     "window_hbm_frac": w_bytes / w_us * 1e-3 / PEAK_HBM_GBS}
        del tr2, step2, fc2, dset

    roofline = None
    if not args.no_roofline:
        # second, instrumented pass: HIP events around every fused-MLP / weight-gradient launch, recorded on the stream
        # the launch goes to (torch's current stream at that point: the backward stream or a weight-gradient side stream)
        psteps = min(args.steps, 30)
        ops.PROFILE.reset(enabled=True)
        trainer.use_graph = False   # per-launch HIP events need eager launches
        # ... on ONE stream: with the weight-gradient side streams on, an event pair around a 20 us launch also times the
        # wait for side-stream workgroups to leave its CUs (a 6 561-row launch read 40 us instead of 23), i.e. the
        # schedule, not the kernel.  The schedule is what `ms_per_step` and the committed timeline measure.
        overlap_was, trainer.overlap_wgrad = trainer.overlap_wgrad, False
        for _ in range(psteps):
            trainer.step(*batch)
        torch.cuda.synchronize()
        recs, meta = ops.PROFILE.collect(), dict(ops.PROFILE.meta)
        ops.PROFILE.reset(enabled=False)
        trainer.use_graph = not args.eager
        trainer.overlap_wgrad = overlap_was
        # PMC-measured HBM bytes per launch: rocprofv3 --pmc passes (tools/pmc_collect.py -> tools/make_pmc_traffic.py) cannot run
        # inside this process, so they come from the newest profiles/roundN/pmc_traffic.json -- accepted only when it was
        # collected on THIS build of the kernels (its library_stamp equals the hash of the sources): a stale file is refused
        from neural_lam_amd import _lib as _L

        traffic, traffic_src = None, "no profiles/round*/pmc_traffic.json"
        if True:   # (round 6: the file carries launch keys of the wide configurations too; a key that is absent reads None)
            def round_no(f):
                digits = "".join(ch for ch in f.parent.name if ch.isdigit())
                return int(digits) if digits else -1

            refused = []
            for tfile in sorted((ROOT / "profiles").glob("round*/pmc_traffic.json"), key=round_no, reverse=True):   # newest round first
                try:
                    js = json.loads(tfile.read_text())
                except Exception:
                    continue
                if js.get("library_stamp") == _L.source_stamp():
                    traffic, traffic_src = js.get("bytes_per_launch"), str(tfile.relative_to(ROOT))
                    break
                refused.append(f"{tfile.relative_to(ROOT)} (stamp {js.get('library_stamp')})")
            if traffic is None and refused:
                traffic_src = "refused, collected on another build of the kernels: " + ", ".join(refused)
        rows = kernel_rooflines(recs, meta, ms_per_step, traffic)
        for r in rows:
            r["launches"] = r["launches"] / psteps
            r["total_ms"] = r["total_ms"] / psteps
            r["share_of_step"] = r["total_ms"] / ms_per_step
        if rows:
            top = rows[0]
            tot_flops = sum(r["algorithmic_flops"] * r["launches"] for r in rows)
            tot_exec = sum(r["executed_mfma_flops"] * r["launches"] for r in rows)
            tot_bytes = sum(r["algorithmic_bytes"] * r["launches"] for r in rows)
            tot_bytes_min = sum(r["algorithmic_bytes_min"] * r["launches"] for r in rows)
            t = ms_per_step * 1e-3
            roofline = {
                # the contract's fields describe the DOMINANT launch = largest share of the step's kernel time
                "bound": top["bound"],
                "achieved": top["executed_tflops"] if top["bound"] == "mfma" else top["hbm_GBps"],
                "peak": top["mfma_peak_tflops"] if top["bound"] == "mfma" else PEAK_HBM_GBS,
                "unit": "TFLOP/s" if top["bound"] == "mfma" else "GB/s",
                "frac": top["frac"],
                "traffic": top["traffic"],
                "traffic_source": traffic_src,
                "kernel": top["launch"] + ": " + top["what"],
                "algorithmic_bytes_min": top["algorithmic_bytes_min"], "algorithmic_bytes": top["algorithmic_bytes"],
                "note": "frac = max(executed MFMA FLOPs / dense peak of the instruction issued, MINIMUM algorithmic HBM bytes (inputs once, outputs once) / 8 TB/s); "
                        "times = HIP events on the launch stream, eager instrumented pass of %d steps with every launch on one stream (uncontended kernel durations)" % psteps,
                "kernels": rows[:6],
                "step": {
                    "ms": ms_per_step,
                    "algorithmic_gflop": tot_flops / 1e9, "executed_mfma_gflop": tot_exec / 1e9, "algorithmic_MB": tot_bytes / 1e6,
                    "algorithmic_tflops": tot_flops / t / 1e12, "frac_of_fp32_mfma_peak": tot_flops / t / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                    "algorithmic_MB_min": tot_bytes_min / 1e6,
                    "hbm_GBps_algorithmic": tot_bytes / t / 1e9, "hbm_frac": tot_bytes_min / t / 1e9 / PEAK_HBM_GBS,
                    "hbm_frac_incl_saved_and_partials": tot_bytes / t / 1e9 / PEAK_HBM_GBS,
                    "sum_of_kernel_ms_in_fused_mlp_launches": sum(r["total_ms"] for r in rows),
                },
            }

    amp.__exit__(None, None, None)
    if world == 1:
        # the baseline legs below build their own models: release the timed trainer first (its graphs' private pools hold every saved
        # activation of the step -- ~160 GB at cfg5; the executor object and the trainer reference each other, hence the collection)
        import gc

        del trainer, step, forecaster
        if not args.eager:
            del fgraph, run_forecast
        gc.collect()
        torch.cuda.empty_cache()
    drop_in = None
    if world == 1 and not args.no_lightning_leg:
        drop_in = lightning_shaped(cfg, device, args.steps, args.precision)
        for k in ("eager", "graphed", "graphed_fused_adamw", "graphed_flat", "graphed_flat_fused_adamw"):
            drop_in[f"{k}_vs_value_step"] = drop_in[f"ms_per_step_{k}_torch_adamw"] / ms_per_step
    if world == 1 and args.config == "cfg2" and args.precision == "fp32" and not args.no_also and os.environ.get("NLAM_BENCH_ALSO", "1") == "1":
        # N = 1: the wide BASELINE configurations on the driver's clock too -- configs[2] (d = 256, 8 layers, ar_steps 4, fp32 class)
        # and configs[4] (d = 512, 8 layers, ar_steps 8, bf16 autocast), one sample per GPU, each with its same-GPU
        # reference-equivalent; `value` stays cfg2
        also = {"cfg3": also_leg("cfg3", "fp32", device, rank, world, args, timed_regions),
                "cfg5_bf16": also_leg("cfg5", "bf16", device, rank, world, args, timed_regions)}
    if rank == 0:
        out["forecast_steps_per_s"] = forecast_steps_per_s
        out["loss_step0"] = loss_step0
        out["roofline"] = roofline
        if data_path is not None:
            out["from_device_dataset"] = data_path
        if drop_in is not None:
            out["lightning_shaped"] = drop_in
        if also is not None:
            out["also"] = also
        if world == 1 and not args.no_cpu_baseline:
            o0 = oracle_loss_step0(cfg, device)
            out["oracle_loss_step0"] = o0
            out["loss_step0_rel_diff_vs_oracle"] = abs(loss_step0 - o0) / abs(o0)
            out["cpu_baseline"] = cpu_baseline(cfg)
        if world == 1 and not args.no_gpu_baseline:
            g = gpu_reference_equivalent(cfg, device, autocast=args.precision == "bf16")
            for k in ("nondeterministic", "deterministic"):
                v = g.get(f"ms_per_step_{k}")
                g[f"speedup_vs_{k}"] = (v / ms_per_step) if v else None
            out["gpu_reference_equivalent"] = g
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
