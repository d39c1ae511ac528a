#!/usr/bin/env python3
"""Compare two device-assembly listings of csrc/nlam_hip.hip kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC [-DNLAM_TU=k] --cuda-device-only -S nlam_hip.hip -o X.s
    tools/device_asm_diff.py [--rename OLD=NEW]... before.s after.s

A host-side refactor must leave the device code alone: the same set of kernel symbols, and under every symbol the same
text (code, kernel descriptor, resource comments) and the same metadata record.  The order in which the compiler emits the
functions follows the order in which the host code names them and may change, so the listing is cut at the function
boundaries and the pieces are compared by symbol.  Two things are normalised: lines that name `__hip_cuid_` (a hash of
the source text), and the function ordinal in local labels and loop comments (.LBB<n>_<k>, .Lfunc_end<n>; with it the
padding in front of a comment), which is the emission order again.  A kernel that was renamed on purpose is paired with
--rename OLD=NEW (repeatable): the one symbol of before.s that contains OLD is compared with the one symbol of after.s that
contains NEW, each under a placeholder for its own name, instead of being reported as missing on both sides.
Exit status 0 = identical, 1 = not; the kernel count is printed either way."""
import re
import sys

ORDINAL = re.compile(r"\b(L?BB|Lfunc_begin|Lfunc_end|LJTI)\d+")


def pieces(path):
    lines = [l for l in open(path) if "__hip_cuid_" not in l]
    meta = next(i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata")
    # functions: from the .section line in front of `.type SYM,@function` to the next one (the last ends at the gpr_maximums section)
    starts = []
    for i, l in enumerate(lines[:meta]):
        m = re.match(r"\t\.type\t(\S+),@function", l)
        if m:
            j = i
            while not lines[j].startswith("\t.section\t.text"):
                j -= 1
            starts.append((j, m.group(1)))
    tail = next(i for i in range(starts[-1][0], meta) if lines[i].startswith("\t.section\t.AMDGPU.gpr_maximums"))
    while lines[tail - 1].split()[0] in (".text", ".p2alignl", ".fill"):   # the padding behind the last function
        tail -= 1
    out = {"<head>": lines[: starts[0][0]], "<tail>": lines[tail:meta]}
    for (a, sym), (b, _) in zip(starts, starts[1:] + [(tail, None)]):
        assert sym not in out, sym
        out[sym] = [" ".join(ORDINAL.sub(r"\1N", l).split()) for l in lines[a:b]]
    # metadata: one YAML record per kernel
    recs, cur = [], None
    for l in lines[meta:]:
        if l.startswith("  - ."):
            cur = []
            recs.append(cur)
        if cur is None or not l.startswith("  "):
            cur = None
            out.setdefault("<meta>", []).append(l)
        else:
            cur.append(l)
    for r in recs:
        name = next(l.split()[1] for l in r if l.startswith("    .name:"))
        out["meta:" + name] = r
    return out


def rename(d, sub, key, path):
    """Re-key the one kernel of d whose symbol contains sub as `key`, its own name replaced by a placeholder in its text."""
    syms = [k for k in d if sub in k and not k.startswith(("meta:", "<"))]
    if len(syms) != 1:
        sys.exit(f"--rename: {sub!r} matches {len(syms)} symbols of {path}")
    for k in (syms[0], "meta:" + syms[0]):
        d[k.replace(syms[0], key)] = [l.replace(syms[0], "<renamed>") for l in d.pop(k)]


def main():
    renames = []
    while len(sys.argv) > 1 and sys.argv[1] == "--rename":
        renames.append(sys.argv[2].split("=", 1))
        del sys.argv[1:3]
    a, b = pieces(sys.argv[1]), pieces(sys.argv[2])
    for old, new in renames:
        rename(a, old, f"{old}={new}", sys.argv[1])
        rename(b, new, f"{old}={new}", sys.argv[2])
    kernels = lambda d: sorted(k[5:] for k in d if k.startswith("meta:"))
    print(f"{sys.argv[1]}: {len(kernels(a))} kernels, {sys.argv[2]}: {len(kernels(b))} kernels")
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(("only in " + (sys.argv[1] if k in a else sys.argv[2])) + ": " + k)
            bad += 1
        elif a[k] != b[k]:
            print("differs: " + k)
            bad += 1
    print("identical kernel by kernel" if bad == 0 else f"{bad} pieces differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
