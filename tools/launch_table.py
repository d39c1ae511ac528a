#!/usr/bin/env python3
"""Reduce rocprofv3 kernel traces to the multiset of launches of this library's kernels.

    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python -m pytest tests/test_x.py -m gpu
    tools/launch_table.py DIR/**/NAME_kernel_trace.csv ... > table.csv

One output line per distinct (kernel instantiation, grid, workgroup, dynamic + static LDS bytes) with the number of times it
was launched, sorted: two builds that map every runtime shape to the same instantiation and launch shape give byte-identical
tables (`diff a.csv b.csv`).  The library's kernels are the ones in the anonymous namespace at global scope; everything
else (PyTorch's own kernels) is left out."""
import collections
import csv
import sys


def main():
    table = collections.Counter()
    for path in sys.argv[1:]:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].strip().removeprefix("void ")
                if not name.startswith(("(anonymous namespace)::", "_ZN12_GLOBAL__N_1")):
                    continue
                name = name.removeprefix("(anonymous namespace)::").split("(")[0]
                grid = "x".join(r.get(f"Grid_Size_{a}", "1") or "1" for a in "XYZ")
                wg = "x".join(r.get(f"Workgroup_Size_{a}", "1") or "1" for a in "XYZ")
                table[(name, grid, wg, r.get("LDS_Block_Size", r.get("Group_Segment_Size", "")))] += 1
    w = csv.writer(sys.stdout, lineterminator="\n")
    w.writerow(["kernel", "grid_threads", "workgroup", "lds_bytes", "launches"])
    for key in sorted(table):
        w.writerow([*key, table[key]])


if __name__ == "__main__":
    main()
