"""Wall time of checkpoint.save_checkpoint / load_checkpoint for a captured Trainer at bench.py's cfg2 and cfg5 sizes.

    python tools/checkpoint_bench.py [out.json]

Per config: parameter count, file size, and the median of 5 repetitions of save to a dict (device-to-host copies), save to a
file, load from the dict and load from the file (host-to-device copies; the trainer keeps its captured step)."""
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import bench  # noqa: E402
from neural_lam_amd import checkpoint as ck  # noqa: E402
from neural_lam_amd.trainer import Trainer  # noqa: E402


def timed(fn, reps=5):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    dev = torch.device("cuda:0")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "last.ckpt"
        for name in ("cfg2", "cfg5"):
            cfg = bench.CONFIGS[name]
            _, _, _, _, step, batch = bench.build(cfg, dev)
            tr = Trainer(step, lr=1e-3, use_graph=True)
            for _ in range(2):
                tr.step(*batch)
            ckpt = ck.save_checkpoint(path, tr, epoch=0, global_step=2)
            res[name] = {
                "params": sum(p.numel() for p in tr.fp.params),
                "file_MB": round(path.stat().st_size / 1e6, 2),
                "save_dict_ms": round(timed(lambda: ck.save_checkpoint(None, tr, epoch=0, global_step=2)), 2),
                "save_file_ms": round(timed(lambda: ck.save_checkpoint(path, tr, epoch=0, global_step=2)), 2),
                "load_dict_ms": round(timed(lambda: ck.load_checkpoint(ckpt, tr)), 2),
                "load_file_ms": round(timed(lambda: ck.load_checkpoint(path, tr)), 2),
            }
            tr.step(*batch)   # the captured step still runs after the loads
            torch.cuda.synchronize()
            del tr, step, ckpt
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
