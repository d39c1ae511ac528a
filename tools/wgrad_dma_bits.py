#!/usr/bin/env python3
"""SHA-256 of what nlam_wgrad writes on the LDS-DMA narrow kernel (wgrad_dma_kernel), on small seeded inputs: one JSON object
on stdout.

    NLAM_LIB=/path/to/libnlam_hip.so python tools/wgrad_dma_bits.py > bits.json

Run once per library (NLAM_LIB selects it, the in-tree one by default) and compare the two files: a change that claims to leave
the kernel's summation order alone must leave every digest alone.  Covered: the shapes and slice counts of
tests/test_wgrad_dma_intervals.py, each with NLAM_TUNE_WGRAD_DMA_R = 1, 2 and 4 chunks per barrier interval; per launch the
partials and the dW that nlam_reduce_jobs makes of them.  A library that does not know the key (an older commit) launches what
it has under the same three names, so its output is comparable line by line.  Inputs come from torch's CPU generator, so the
digests depend on the library and the GPU only."""
import ctypes as C
import hashlib
import json
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from neural_lam_amd import _lib as L   # noqa: E402

# (name, m, widths, rows, batch, broadcast sources, gathered sources, SiLU, slice counts)
SHAPES = [
    ("w64x3_r357", 64, (64, 64, 64), 357, 1, (), (), False, (1, 3, 5, 7, 12)),
    ("w60_60_12_b3", 64, (60, 60, 12), 70, 3, (1,), (0, 2), False, (1, 2, 4)),
    ("w64_silu_r357", 64, (64,), 357, 1, (), (), True, (1, 5)),
    ("w64x2_r200", 64, (64, 64), 200, 1, (), (), False, (1, 3)),
    ("w32_r165", 32, (32,), 165, 1, (), (), False, (1, 2)),
    ("w16_b2_r40", 16, (16,), 40, 2, (), (), False, (1,)),
    ("w16x3_b2_r40", 16, (16, 16, 16), 40, 2, (), (1,), False, (1, 3)),
    ("w32x2_r165", 32, (32, 32), 165, 1, (), (0,), False, (2,)),
]


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    lib = L.load()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for i, (name, m, widths, rows, batch, bcast, gather, silu, parts) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(300 + i)
        A = torch.randn(batch * rows, m, generator=g).to(dev)
        q = L.Wgrad()
        q.A, q.m, q.batch, q.rows, q.nsrc, q.n = A.data_ptr(), m, batch, rows, len(widths), sum(widths)
        q.flags = L.F_SILU_B if silu else 0
        keep = []
        for s, w in enumerate(widths):
            nr = rows // 2 + 3 if s in gather else rows
            nb = 1 if s in bcast else batch
            S = (torch.randn(nb, nr, w, generator=g) * 2.0 ** torch.randint(-3, 4, (w,), generator=g).float()).to(dev)
            idx = torch.randint(0, nr, (rows,), generator=g, dtype=torch.int32).to(dev) if s in gather else None
            q.src[s].ptr, q.src[s].idx = S.data_ptr(), None if idx is None else idx.data_ptr()
            q.src[s].bstride, q.src[s].width = 0 if s in bcast else nr * w, w
            keep += [S, idx]
        for nparts in parts:
            for r in (1, 2, 4):
                lib.nlam_set_tuning(L.TUNE_WGRAD_DMA_R, r)   # -1 from a library without the key: it has one kernel for all three
                partials = torch.full((nparts, m, q.n), float("nan"), device=dev)
                q.partials, q.nparts = partials.data_ptr(), nparts
                assert lib.nlam_wgrad_plan(C.byref(q)) == L.WGP_DMA, name
                L.check(lib.nlam_wgrad(C.byref(q), stream), f"nlam_wgrad({name})")
                dw = torch.full((m, q.n), float("nan"), device=dev)
                jobs = L.ReduceJobs()
                jobs.njobs = 1
                j = jobs.job[0]
                j.partials, j.out, j.stride, j.nparts, j.n = partials.data_ptr(), dw.data_ptr(), m * q.n, nparts, m * q.n
                j.accumulate, j.ncols, j.ld = 0, 0, 0
                L.check(lib.nlam_reduce_jobs(C.byref(jobs), stream), "nlam_reduce_jobs")
                torch.cuda.synchronize()
                assert torch.isfinite(partials).all() and torch.isfinite(dw).all(), (name, nparts, r)
                out[f"{name}/np{nparts}/R{r}/partials"], out[f"{name}/np{nparts}/R{r}/dW"] = digest(partials), digest(dw)
    lib.nlam_set_tuning(L.TUNE_WGRAD_DMA_R, 0)
    print(json.dumps(out, indent=0, sort_keys=True))


if __name__ == "__main__":
    main()
