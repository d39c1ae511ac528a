#!/usr/bin/env python3
"""SHA-256 of everything the step-tail and loss entry points write, on small seeded inputs: one JSON object on stdout.

    NLAM_LIB=/path/to/libnlam_hip.so python tools/step_tail_bits.py > bits.json

Run once per library (NLAM_LIB selects it, the in-tree one by default) and compare the two files: a change that claims to leave
these kernels' arithmetic alone must leave every digest alone.  Covered: nlam_step_tail_fwd / _bwd (the inv_var term) and
nlam_step_tail_loss_fwd / _bwd (the six NLAM_LOSS_* kinds) on the shapes of tests/test_losses.py's
test_step_tail_kernels_match_float64_formula (16-byte loop, scalar loop, quads across the row and the node wrap, misaligned
slices), with and without dstd / dmean and g_pred, one gradient output at a time; nlam_wmse_fwd and nlam_loss_fwd (six kinds,
per-variable std) on the same predictions.  Inputs come from torch's CPU generator, so the digests depend on the library and
the GPU only."""
import ctypes as C
import hashlib
import json
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from neural_lam_amd import _lib as L   # noqa: E402

SHAPES = {"quads": (2, 40, 5), "scalar": (2, 41, 5), "row_wrap": (1, 8, 3), "node_wrap": (2, 6, 1)}   # (B, N, F)
KINDS = ["mse", "mae", "wmse", "wmae", "nll", "crps_gauss"]
SCALE, GLOSS, NPARTS = 0.5, 0.7, 512


def inputs(seed, B, N, F):
    g = torch.Generator().manual_seed(seed)
    d = {k: torch.randn(B, N, F, generator=g) for k in ("delta", "prev", "truth", "target", "g_pred")}
    bmask = torch.zeros(N)
    bmask[torch.randperm(N, generator=g)[: max(1, round(0.3 * N))]] = 1.0
    d["bmask"], d["row_weight"] = bmask, (1 - bmask) / (1 - bmask).sum()
    d["dstd"], d["dmean"] = torch.rand(F, generator=g) + 0.5, torch.randn(F, generator=g)
    d["var_std"] = torch.rand(F, generator=g) + 0.5
    d["inv_var"] = 1.0 / d["var_std"] ** 2
    return d


def misaligned(t):
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    return view


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    lib = L.load()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    out = {"library": str(L.lib_path().name)}

    def reduced(partials):
        loss = torch.zeros((), device=dev)
        L.check(lib.nlam_reduce_partials(ptr(partials), NPARTS, 1, 1, ptr(loss), 0, stream), "nlam_reduce_partials")
        return loss

    for i, (name, (B, N, F)) in enumerate(SHAPES.items()):
        cpu = inputs(100 + i, B, N, F)
        for mis in ((False, True) if name == "quads" else (False,)):
            put = (lambda t: misaligned(t.to(dev))) if mis else (lambda t: t.to(dev).contiguous())
            t = {k: put(v) for k, v in cpu.items()}
            for term in ["inv_var"] + KINDS:
                kind = () if term == "inv_var" else (L.LOSS_KINDS[term],)
                consts = t["inv_var"] if term == "inv_var" else t["var_std"]
                fwd = lib.nlam_step_tail_fwd if term == "inv_var" else lib.nlam_step_tail_loss_fwd
                bwd = lib.nlam_step_tail_bwd if term == "inv_var" else lib.nlam_step_tail_loss_bwd
                for affine in (True, False):
                    dstd, dmean = (t["dstd"], t["dmean"]) if affine else (None, None)
                    key = f"{name}{'+1' if mis else ''}/{term}/{'affine' if affine else 'plain'}"
                    pred, partials = put(torch.zeros(B, N, F)), torch.zeros(NPARTS, device=dev)
                    L.check(fwd(*kind, ptr(t["delta"]), ptr(t["prev"]), ptr(t["truth"]), ptr(t["target"]), ptr(dstd), ptr(dmean),
                                ptr(t["bmask"]), ptr(consts), ptr(t["row_weight"]), SCALE, ptr(pred), ptr(partials), NPARTS, B * N, N, F,
                                stream), key)
                    out[key + "/pred"], out[key + "/partials"] = digest(pred), digest(partials)
                    out[key + "/loss"] = digest(reduced(partials))
                    gloss = torch.tensor(GLOSS, device=dev)
                    for gp in (True, False):
                        for which in ("d_delta", "d_prev"):
                            g = put(torch.zeros(B, N, F))
                            L.check(bwd(*kind, ptr(t["g_pred"]) if gp else None, ptr(gloss), ptr(pred), ptr(t["target"]), ptr(dstd),
                                        ptr(t["bmask"]), ptr(consts), ptr(t["row_weight"]), SCALE, ptr(g) if which == "d_delta" else None,
                                        ptr(g) if which == "d_prev" else None, B * N, N, F, stream), key)
                            out[f"{key}/{'g_pred' if gp else 'last'}/{which}"] = digest(g)
            # the rollout losses on the same numbers: pred = prev, (B, T = 1, N, F)
            key = f"{name}{'+1' if mis else ''}"
            partials = torch.zeros(NPARTS, device=dev)
            L.check(lib.nlam_wmse_fwd(ptr(t["prev"]), ptr(t["target"]), ptr(t["inv_var"]), ptr(t["row_weight"]), B * N, N, F, SCALE,
                                      ptr(partials), NPARTS, stream), "nlam_wmse_fwd")
            out[key + "/wmse_fwd/partials"], out[key + "/wmse_fwd/loss"] = digest(partials), digest(reduced(partials))
            for k in KINDS:
                p = L.Loss()
                p.pred, p.target, p.var_std, p.row_weight = ptr(t["prev"]), ptr(t["target"]), ptr(t["var_std"]), ptr(t["row_weight"])
                p.rows, p.nodes, p.nvars, p.kind, p.scale = B * N, N, F, L.LOSS_KINDS[k], SCALE
                partials = torch.zeros(NPARTS, device=dev)
                p.partials, p.nparts = ptr(partials), NPARTS
                L.check(lib.nlam_loss_fwd(C.byref(p), stream), "nlam_loss_fwd")
                out[f"{key}/loss_fwd/{k}/partials"], out[f"{key}/loss_fwd/{k}/loss"] = digest(partials), digest(reduced(partials))
    torch.cuda.synchronize()
    print(json.dumps(out, indent=0, sort_keys=True))


if __name__ == "__main__":
    main()
