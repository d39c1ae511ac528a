"""Isolated time of one nlam_wgrad_dma_group launch against its members launched one by one (nlam_wgrad).

    python tools/wgrad_dma_group_bench.py [--rows 6561] [--members 5] [--d 64] [--reps 200] [--rounds 7]

Two shapes, as a cfg2 step has them on its mesh: dW1 with two 64-column sources (the second gathered), dW2 with SiLU on the
one source.  Every member has operands of its own.  A round times `reps` back-to-back launches between two events (members:
the `members` launches of one pass count as one sample), so what is measured is launch-to-launch throughput on an idle chip
with the operands warm in the caches -- the same conditions for both arms; the median over the rounds is reported, with min
and max.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from neural_lam_amd import _lib as L   # noqa: E402


def member(lib, rows, d, nsrc, silu, seed):
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    A = torch.randn(rows, d, generator=g).to(dev)
    q = L.Wgrad()
    q.A, q.m, q.batch, q.rows, q.nsrc, q.n = A.data_ptr(), d, 1, rows, nsrc, nsrc * d
    q.flags = (3 << 8) | (L.F_SILU_B if silu else 0)
    keep = [A]
    for k in range(nsrc):
        S = torch.randn(rows, d, generator=g).to(dev)
        keep.append(S)
        q.src[k].ptr, q.src[k].bstride, q.src[k].width = S.data_ptr(), rows * d, d
        if k == 1:
            idx = torch.randint(0, rows, (rows,), generator=g, dtype=torch.int32).to(dev)
            keep.append(idx)
            q.src[k].idx = idx.data_ptr()
    q.partials, q.nparts = A.data_ptr(), 1
    q.nparts = lib.nlam_wgrad_nparts(C.byref(q))
    part = torch.empty(q.nparts, d, nsrc * d, device=dev)
    keep.append(part)
    q.partials = part.data_ptr()
    return q, keep, part


def timed(fn, reps, rounds):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(20):
        fn(st)
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(st)
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / reps)
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=6561)
    ap.add_argument("--members", type=int, default=5)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    lib = L.load()
    res = {"rows": a.rows, "members": a.members, "d": a.d}
    for name, nsrc, silu in (("dW1_2src", 2, False), ("dW2_silu", 1, True)):
        ms = [member(lib, a.rows, a.d, nsrc, silu, 10 * nsrc + k) for k in range(a.members)]
        arr = (L.Wgrad * a.members)(*[m[0] for m in ms])
        assert lib.nlam_wgrad_dma_group_supported(C.byref(ms[0][0])) == 1

        def singles(st):
            for q, _, _ in ms:
                assert lib.nlam_wgrad(C.byref(q), st) == 0

        def grouped(st):
            assert lib.nlam_wgrad_dma_group(arr, a.members, st) == 0

        singles(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        ref = [m[2].clone() for m in ms]
        for m in ms:
            m[2].fill_(float("nan"))
        grouped(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        same = all(torch.equal(r, m[2]) for r, m in zip(ref, ms))
        res[name] = {"nparts": int(ms[0][0].nparts), "same_bits": same, "one_member": timed(lambda st: lib.nlam_wgrad(C.byref(ms[0][0]), st), a.reps, a.rounds),
                     "members_one_by_one": timed(singles, a.reps, a.rounds), "grouped": timed(grouped, a.reps, a.rounds)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
