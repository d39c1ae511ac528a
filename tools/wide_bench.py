"""Timings of MLP launches wider than the fused kernels (the tiled-GEMM family, nlam_mlp_fwd_gemm / nlam_mlp_bwd_gemm) at MEPS
size, one sample:

  * the m2m edge layer (InteractionNet over the 57 616 mesh edges, senders = receivers) and the m2g layer (255 136 edges, mesh ->
    grid, no edge update) at d = 512 on the fused family AND on the tiled-GEMM family (routing threshold lowered inside this
    process), and at d = 768 / 1024 (tiled-GEMM family only): forward and backward, median of --reps HIP-event-timed runs;
  * one GraphLAM training step at d = 768 with 4 processor layers (bench.py's cfg2 shape otherwise, HIP-graph replay).

Rates: algorithmic FLOPs of the layer's MLPs (edge MLP 2 E (3d d + d d), node MLP 2 N (2d d + d d); backward: data gradients of
both Linears plus both weight gradients, 2x the forward) over the timed span, and that rate as a share of the matrix peak of the
mode the launches run on (bf16x3: 2.5 PF / 6 MFMAs per product block; bf16: 2.5 PF).  Kernel-level times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this tool (profiles/wide_gemm/README.md).

    python tools/wide_bench.py [--reps 10] [--out FILE] [--no-step] [--widths 512,768,1024]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

BF16_PEAK = 2.5e15
MODE_PEAK = {"bf16x3": BF16_PEAK / 6, "bf16": BF16_PEAK}


def meps_edge_sets():
    from neural_lam_amd import graph as G

    raw = G.create_regular_grid_graph(G.regular_grid_xy(238, 268))
    m2m = raw["m2m_edge_index"]
    m2m = m2m[0] if isinstance(m2m, list) else m2m
    return {"m2m": (m2m.long(), True, True), "m2g": (raw["m2g_edge_index"].long(), False, False)}


def time_layer(name, ei, same, update_edges, d, family, reps):
    from neural_lam_amd import gnn_layers as hl
    from neural_lam_amd import ops

    dev = torch.device("cuda:0")
    ops._MAX_FUSED = None if family == "fused" else min(256, d - 1)   # "gemm" at d <= 512: every launch of the layer on the new family
    ns, nr, E = int(ei[0].max()) + 1, int(ei[1].max()) + 1, ei.shape[1]
    torch.manual_seed(0)
    net = hl.InteractionNet(ei, d, update_edges=update_edges).to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rec = torch.randn(1, nr, d, device=dev, generator=g).requires_grad_()
    send = rec if same else torch.randn(1, ns, d, device=dev, generator=g).requires_grad_()
    edge = torch.randn(1, E, d, device=dev, generator=g).requires_grad_()
    fwd, bwd = [], []
    for it in range(reps + 2):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        net.zero_grad(set_to_none=True)
        for t in (send, rec, edge):
            t.grad = None
        e0.record()
        outs = net(send, rec, edge)
        outs = outs if isinstance(outs, tuple) else (outs,)
        e1.record()
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
        e2.record()
        torch.cuda.synchronize()
        if it >= 2:
            fwd.append(e0.elapsed_time(e1))
            bwd.append(e1.elapsed_time(e2))
        del outs
    ops._MAX_FUSED = None
    fwd.sort()
    bwd.sort()
    tf, tb = fwd[len(fwd) // 2], bwd[len(bwd) // 2]
    flops_f = 2.0 * E * (3 * d * d + d * d) + 2.0 * nr * (2 * d * d + d * d)
    mode = ops.matmul_mode_name()
    peak = MODE_PEAK.get(mode)
    res = {"layer": name, "edges": E, "senders": ns, "receivers": nr, "d": d, "family": family, "mode": mode, "fwd_ms": round(tf, 3),
           "bwd_ms": round(tb, 3), "fwd_tflops": round(flops_f / tf / 1e9, 2), "bwd_tflops": round(2 * flops_f / tb / 1e9, 2)}
    if peak:
        res["fwd_share_of_peak"] = round(flops_f / tf * 1e3 / peak, 3)
        res["bwd_share_of_peak"] = round(2 * flops_f / tb * 1e3 / peak, 3)
    return res


def time_step(d, L, steps):
    import bench
    from neural_lam_amd.trainer import Trainer

    dev = torch.device("cuda:0")
    cfg = dict(bench.CONFIGS["cfg2"], d=d, L=L)
    _, _, _, _, step, batch = bench.build(cfg, dev)
    tr = Trainer(step, lr=1e-3, use_graph=True)
    for _ in range(3):
        loss = tr.step(*batch)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        loss = tr.step(*batch)
    e1.record()
    torch.cuda.synchronize()
    return {"step": "GraphLAM", "d": d, "processor_layers": L, "grid": "238x268", "executor": tr.executor,
            "step_ms": round(e0.elapsed_time(e1) / steps, 3), "loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--widths", default="512,768,1024")
    ap.add_argument("--layers", default="m2m,m2g")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sets = meps_edge_sets()
    rows = []
    for name in args.layers.split(","):
        ei, same, upd = sets[name]
        for d in (int(w) for w in args.widths.split(",")):
            for family in (("fused", "gemm") if d <= 512 else ("gemm",)):
                r = time_layer(name, ei, same, upd, d, family, args.reps)
                print(json.dumps(r), flush=True)
                rows.append(r)
                torch.cuda.empty_cache()
    if not args.no_step:
        r = time_step(768, 4, args.step_steps)
        print(json.dumps(r), flush=True)
        rows.append(r)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
