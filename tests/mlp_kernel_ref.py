"""Shared machinery of the kernel-level MLP suites (test_mlp_narrow_kernels.py, test_mlp_wide_kernels.py,
test_mlp_gemm_kernels.py): the case record, the problem builder, the float64 math of the contract of include/nlam_hip.h with its
first-order error budget, the two comparison functions, the tiers' problems and the CPU stand-in for a kernel, the
launch-descriptor fillers and the device-buffer helper with NaN fill and NaN guard rows.  A plain module, imported by the three
files; nothing here is collected by pytest."""
import ctypes as C
import math
from dataclasses import dataclass, replace
from types import SimpleNamespace as NS

import numpy as np
import torch

from neural_lam_amd import _lib as L
from neural_lam_amd import graph as G

U = 2.0 ** -24          # fp32 unit roundoff
UB = 2.0 ** -8          # bf16 unit roundoff
GRID_WAVES = 2048       # nlam_grid_waves() of this build (asserted by the cases that depend on it)
GUARD = 4 * 64          # NaN floats behind every output buffer
EPS = float(np.float32(1e-5))
T_SILU = 2.0 ** -19     # the kernels' fp32 SiLU / SiLU' (v_exp_f32, v_rcp_f32) against the float64 ones, as in test_wgrad_kernels.py
# The matrix modes as include/nlam_hip.h states them: one term = bf16 operand rounding (two operands: 2 * 2^-8), two terms
# ~2^-16, three terms 2^-24 class.  Worst case of the split with round-to-nearest terms: two terms leave 2^-16 of each operand and
# drop the 2^-16 cross product (3 units of 2^-16), three terms leave 2^-24 of each operand and drop two 2^-24 cross products
# (4 units of 2^-24): the safety multiple on the split modes is those "few units", 4.
SPLIT_SAFETY = 4.0
MODE_TERM = {0: 0.0, 1: 2.0 * UB, 2: SPLIT_SAFETY * 2.0 ** -16, 3: SPLIT_SAFETY * 2.0 ** -24}

# receiver in-degrees of the edge sets (tiles are whole receivers of <= 32 rows in all)
GRAPHS = {
    # several tiles of fewer than 32 rows; empty receivers at the start, in the middle and at the end
    "mixed": (0, 0, 5, 9, 0, 11, 3, 8, 0, 0, 12, 7, 1, 0, 6, 10, 4, 13, 2, 0),
    # a receiver of in-degree 70 (three pieces) and one of 33 between ordinary and empty ones
    "split": (0, 4, 70, 0, 9, 33, 2, 0, 17, 0),
}
# the same receivers many times over, for the wide kernels' super tiles (several 32-row tiles per workgroup pass, a persistent
# grid that walks several super tiles): odd tile counts
GRAPHS["mixed12"] = GRAPHS["mixed"] * 12 + (3, 30)
GRAPHS["split9"] = GRAPHS["split"] * 9 + (0, 5, 31)
GRAPHS["mixed44"] = GRAPHS["mixed"] * 44 + (7, 0, 30, 30)      # more than 128 tiles, an odd number of 64-row super tiles (the edge kernels)
NUM_SEND = 13


@dataclass(frozen=True)
class Case:
    name: str
    fwd: int                   # nlam_mlp_fwd_plan code the case is meant to hit
    bwd: int                   # nlam_mlp_bwd_plan code
    widths: tuple
    hid: int
    dout: int
    rows: int = 0              # rows per batch item (graph cases: the number of edges)
    batch: int = 1
    mm: int = 0                # requested matrix mode (NLAM_F_MM_* term count)
    ln: bool = True
    add0: bool = False
    add1: bool = False
    mean: bool = False
    no_act: bool = False
    pre: bool = False
    ldw1_extra: int = 0        # NLAM_F_PRE_ADD: columns of W1 behind src0's (and the addends')
    gather: tuple = ()         # sources read through an unsorted index with repeated rows
    perm: tuple = ()           # sources read through a permutation (dmode 1 scatters through it)
    broadcast: tuple = ()      # sources with bstride = 0
    graph: str = ""            # edge geometry over GRAPHS[graph]: sources (edge, sender, receiver) gathered by (perm, send, rec)
    roles: str = "esr"         # ... the role of each source of a graph case
    atomic: bool = False       # receivers above 32 in-edges as NLAM_TILE_SPLIT tiles (else the virtual split + nlam_split_combine)
    want_out: bool = True
    aggregate: bool = False
    out_perm: bool = False     # out_idx = a permutation (graph cases: the CSR permutation)
    dmode: tuple = (1, 1, 1)
    g_out: bool = True
    g_aggr: bool = False
    cat: tuple = ()            # widths of the concatenated pieces of src[0]
    cat_shared: tuple = ()     # pieces with cat_bstride = 0
    sbf: bool = False          # NLAM_F_STORE_BF16: z1 / xhat (forward) and dz1 / dz2 (backward) are rows of bf16
    acc0: bool = False         # NLAM_F_ACC_DSRC0: dsrc[0] is pre-filled and added to
    tune: tuple = ()           # (key, value) pairs for nlam_set_tuning (the wide file's fixture sets and restores them)
    ldw1_pad: int = 0          # floats between rows of W1 beyond the width sum, without NLAM_F_PRE_ADD (the tiled-GEMM family)
    ln_beta: bool = True       # False: LayerNorm without ln_b (ln_b = NULL)
    rowseg: bool = False       # aggregation without a tile list (tiles = NULL): every row is its own segment, through rowptr

    def __str__(self):
        return self.name


# ---------------------------------------------------------------------------------------------------------------------------
# the problem on the host: float64 operands exactly as they are stored (fp32 values), and the geometry
# ---------------------------------------------------------------------------------------------------------------------------
LOW_W = 1.0 + 2.0 ** -9 + 2.0 ** -18   # three non-zero bf16 terms (1, 2^-9, 2^-18), no rounding tie in the split; 19 bits: exact in fp32
LOW_ONES = 16                          # ones per input row of the low-order probe


def _values(gen, shape, ncols, kind, r=4):
    if kind == "int":
        return torch.randint(-r, r + 1, shape, generator=gen).double()
    if kind == "probe":   # 1 + 2^-9 + 0.98 * 2^-17: bf16 terms 1, 2^-9 and a third term that is as large as a third term gets
        return torch.full(shape, 1.0 + 2.0 ** -9 + 0.98 * 2.0 ** -17, dtype=torch.float64).float().double()
    scale = 2.0 ** torch.randint(-3, 4, (ncols,), generator=gen).double()   # a different scale per column
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * scale).float().double()


def _sparse_ones(shape, ones, shift):
    """(nb, nr, w) of zeros with `ones` ones per row (fewer when the row is shorter), at positions that move from row to row, so
    that every K group of the source is hit by some row."""
    nb, nr, w = shape
    n1 = min(ones, w)
    rows = torch.arange(nr)[:, None]
    pos = (rows * 5 + shift + torch.arange(n1)[None, :] * max(1, w // n1)) % w
    S = torch.zeros(shape, dtype=torch.float64)
    S.scatter_(2, pos[None].expand(nb, -1, -1), 1.0)
    return S


def build_problem(case, seed, kind, irange=4):
    """kind: "int" (tier a; irange: the integers are in [-irange, irange]), "rand" (tier b), "probe" (tier c of the narrow file:
    positive operands with a maximal third bf16 term) or "low" (tier c of the wide file, exact at any K: every W1 entry is
    +-LOW_W with one sign per row of W1, an input row holds at most LOW_ONES ones and otherwise zeros, b1 and the addends of a
    factorised layer are small integers -- every partial sum of z1 is k * LOW_W + integer, k <= 16: 20 bits at most)."""
    gen = torch.Generator().manual_seed(seed)
    c = case
    P = NS(case=c, batch=c.batch, hid=c.hid, dout=c.dout, nsrc=len(c.widths), eps=EPS, irange=irange)
    P.tiles = P.rowptr = P.scale = P.seg_of_row = P.comb = P.out_idx = P.rowptr_dev = P.inv_deg_dev = None
    P.nseg = P.nseg_rows = 0
    P.has_split = False
    if c.graph:
        deg = torch.tensor(GRAPHS[c.graph])
        rec = torch.repeat_interleave(torch.arange(len(deg)), deg)
        order = torch.randperm(rec.numel(), generator=gen)
        ei = torch.stack([torch.randint(0, NUM_SEND, (rec.numel(),), generator=gen), rec[order]])
        csr = G.build_edge_csr(ei, num_send=NUM_SEND, num_rec=len(deg))
        tiles, has_split, split = G.build_tile_schedule(csr.rowptr, virtual_split=not c.atomic)
        csr = G.attach_split(csr, split)
        P.rows, P.tiles, P.has_split, P.csr = csr.num_edges, tiles, has_split, csr
        P.nseg = csr.num_rec
        P.rowptr_dev = csr.rowptr_ext if split is not None else csr.rowptr
        P.inv_deg_dev = csr.inv_deg_ext if split is not None else csr.inv_deg
        P.nseg_rows = csr.nseg_ext if split is not None else csr.num_rec
        P.comb = (csr.comb_ptr, csr.comb_src, csr.comb_dst) if split is not None else None
        P.seg_of_row = csr.rec.long()
        P.scale = csr.inv_deg.double() if c.mean else torch.ones(csr.num_rec, dtype=torch.float64)
        P.deg = deg.double()
        assert c.graph.startswith("split") == (split is not None or has_split)
        assert int((tiles[:, 1] < 32).sum()) >= 2   # tiles of fewer than 32 rows made of whole receivers
    else:
        P.rows = c.rows
        if c.rowseg:   # no tile list: tile t is rows 32 t .. 32 t + 31, every row a segment of its own
            P.nseg = P.nseg_rows = c.rows
            P.rowptr_dev, P.inv_deg_dev = torch.arange(c.rows + 1), torch.ones(c.rows)
            P.seg_of_row = torch.arange(c.rows)
            P.scale = P.deg = torch.ones(c.rows, dtype=torch.float64)
    P.ntiles = P.tiles.shape[0] if P.tiles is not None else -(-P.rows // 32)
    rows = P.rows
    P.srcs = []
    for k, w in enumerate(c.widths):
        idx = None
        if c.graph:
            role = c.roles[k]
            nr = {"e": rows, "s": NUM_SEND, "r": P.nseg}[role]
            idx = {"e": P.csr.perm, "s": P.csr.send, "r": P.csr.rec}[role].long()
        elif k in c.gather:
            nr = rows // 2 + 3
            idx = torch.randint(0, nr, (rows,), generator=gen)   # unsorted, with repeated rows
            idx[: min(4, rows)] = nr - 1
        elif k in c.perm:
            nr, idx = rows, torch.randperm(rows, generator=gen)
        else:
            nr = rows
        nb = 1 if k in c.broadcast else c.batch
        vk = "rand" if (kind == "probe" and c.pre and k > 0) else kind   # the probe is about GEMM1's operands
        if kind == "low":
            ngemm = 1 if c.pre else len(c.widths)
            S = _values(gen, (nb, nr, w), w, "int") if (c.pre and k > 0) else _sparse_ones((nb, nr, w), LOW_ONES // ngemm, 3 * k)
        else:
            S = _values(gen, (nb, nr, w), w, vk, irange)
        P.srcs.append(NS(S=S, idx=idx, nr=nr, nb=nb, width=w, bstride=0 if k in c.broadcast else nr * w))
        if c.dmode[k] == 1:
            assert idx is None or idx.unique().numel() == nr == rows, "dmode 1 scatters through a unique index"
        if c.dmode[k] == 3:
            assert (c.graph and c.roles[k] == "r") or (c.rowseg and idx is None)
    if c.cat:   # src[0] = the row-wise concatenation of pieces
        assert sum(c.cat) == c.widths[0] and len(c.widths) == 1
        X = P.srcs[0].S
        P.pieces, off = [], 0
        for q, w in enumerate(c.cat):
            piece = X[:, :, off: off + w]
            if q in c.cat_shared:
                piece = piece[:1]
                X[:, :, off: off + w] = piece   # the same rows for every batch item
            P.pieces.append(piece.contiguous())
            off += w
    kg = c.widths[0] if c.pre else sum(c.widths)   # columns of W1 that go through GEMM1
    P.kg, P.ldw1 = kg, (kg + c.ldw1_extra if c.pre else kg + c.ldw1_pad)
    if kind == "int":
        P.W1 = _values(gen, (c.hid, P.ldw1), 0, "int", irange)
        P.W2 = _values(gen, (c.dout, c.hid), 0, "int", irange)
        P.b1, P.b2 = _values(gen, (c.hid,), 0, "int", irange), _values(gen, (c.dout,), 0, "int", irange)
        P.gamma, P.beta = _values(gen, (c.dout,), 0, "int", irange), _values(gen, (c.dout,), 0, "int", irange)
    else:
        rs = 2.0 ** torch.randint(-3, 4, (c.dout,), generator=gen).double()
        P.W1 = (torch.randn((c.hid, P.ldw1), generator=gen, dtype=torch.float64) / math.sqrt(kg)).float().double()
        if kind == "probe":
            P.W1 = P.W1.abs()
        if kind == "low":
            sign = 1.0 - 2.0 * (torch.arange(c.hid) % 2).double()
            P.W1 = (sign[:, None] * LOW_W).expand(c.hid, P.ldw1).contiguous()
            assert torch.equal(P.W1.float().double(), P.W1)
        P.W2 = (torch.randn((c.dout, c.hid), generator=gen, dtype=torch.float64) / math.sqrt(c.hid) * rs[:, None]).float().double()
        P.b1 = (0.5 * torch.randn((c.hid,), generator=gen, dtype=torch.float64)).float().double()
        if kind == "low":
            P.b1 = _values(gen, (c.hid,), 0, "int")
        P.b2 =(0.5 * torch.randn((c.dout,), generator=gen, dtype=torch.float64) * rs).float().double()
        gs = 2.0 ** torch.randint(-3, 4, (c.dout,), generator=gen).double()
        P.gamma = ((1.0 + 0.3 * torch.randn((c.dout,), generator=gen, dtype=torch.float64)) * gs).float().double()
        P.beta = (torch.randn((c.dout,), generator=gen, dtype=torch.float64) * gs).float().double()
    if not c.ln_beta:
        P.beta = torch.zeros_like(P.beta)
    P.out_rows = rows
    if c.out_perm:
        P.out_idx = P.csr.perm.long() if c.graph else torch.randperm(rows, generator=gen)
    gk = "int" if kind == "int" else "rand"
    P.g_out = _values(gen, (c.batch, P.out_rows, c.dout), c.dout, gk, irange) if c.g_out else None
    P.g_aggr = _values(gen, (c.batch, P.nseg, c.dout), c.dout, gk, irange) if c.g_aggr else None
    P.dsrc0_init = None
    if c.acc0:   # what an earlier step left in dsrc[0]
        assert c.dmode[0] == 1
        P.dsrc0_init = _values(gen, (c.batch, P.srcs[0].nr, c.widths[0]), c.widths[0], gk, irange)
    assert c.g_out or c.g_aggr
    assert not c.g_out or c.want_out
    assert not c.g_aggr or c.aggregate
    return P


# ---------------------------------------------------------------------------------------------------------------------------
# the math of the header's contract, in a chosen precision (float64: the reference; float32: the CPU stand-in "kernel"), with
# the first-order error budget propagated next to it and optional injected defects (the checker's own test)
# ---------------------------------------------------------------------------------------------------------------------------
def _segsum(x, seg, nseg):
    out = torch.zeros((x.shape[0], nseg, x.shape[2]), dtype=x.dtype)
    return out.index_add_(1, seg, x)


def _gathered(P, dt, defect):
    xs = []
    for k, s in enumerate(P.srcs):
        S = s.S.to(dt)
        S = S.expand(P.batch, -1, -1) if S.shape[0] == 1 else S
        idx = s.idx
        if defect == "swap_gather_indices" and idx is not None and k == max(i for i, q in enumerate(P.srcs) if q.idx is not None):
            idx = idx.clone()
            j = int((idx != idx[0]).nonzero()[0])
            idx[0], idx[j] = idx[j].clone(), idx[0].clone()
        xs.append(S[:, idx] if idx is not None else S)
    return xs


def to_bf16(t, truncate=False):
    """The values rounded to bfloat16 (to nearest, ties to even: v_cvt_pk_bf16_f32) in the dtype they came in; truncate: the
    low 16 bits of the fp32 value cut off instead (an injected defect)."""
    if truncate:
        return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)
    return t.float().to(torch.bfloat16).to(t.dtype)


def forward_math(P, dt=torch.float64, ns=0, z1_given=None, defect=None):
    """-> (values, budgets): dicts over z1, xhat, rstd, out, aggr (aggr: the real receivers' rows).  ns: the term count the
    budget is made for; z1_given: continue from this pre-activation (budget of z1 = 0: the stages after GEMM1 on their own).
    With bf16 storage (case.sbf) the reference's z1 / xhat stay unrounded and their budgets take one bf16 rounding of the value
    the kernel holds (UB * (|R| + E)); the stand-in stores rounded copies and goes on with what it holds in fp32, as the kernels
    do; a z1_given is then a stored, rounded z1, UB * |z1| away from what the later stages of the kernel went on with."""
    c = P.case
    f = lambda t: t.to(dt)
    xs = _gathered(P, dt, defect)
    W1g = f(P.W1[:, : P.kg])
    X = xs[0] if c.pre else torch.cat(xs, -1)
    adds = xs[1:] if c.pre else []
    if defect == "drop_input_column":
        X = X.clone()
        X[..., X.shape[-1] // 2] = 0
    if defect == "supertile_last_row_from_neighbour":   # the last row of the first 128-row super tile reads the next tile's first row
        X = X.clone()
        r = 127 if X.shape[1] > 128 else X.shape[1] - 2
        X[:, r] = X[:, r + 1]
    # the tiled-GEMM family's own: operands concatenated on load, row tiles that straddle batch items, ragged column tiles
    if defect == "boundary_column_from_neighbour":   # the first column of source 1 attributed to source 0: read behind source 0's row
        X = X.clone()
        X[..., c.widths[0]] = torch.roll(xs[0][..., 0], -1, 1)
    if defect == "second_item_first_row_from_first_item":   # the first row of the second batch item, with the first item's batch offset
        X = X.clone()
        X[1, 0] = X[0, 0]
    if defect == "drop_third_term":   # x as two bf16 terms
        x1 = X.to(torch.bfloat16).to(dt)
        X = x1 + (X - x1).to(torch.bfloat16).to(dt)
    if defect == "drop_w1_third_term":   # W1 as two bf16 terms (the wide file's exact probe: its x is 0 / 1, one bf16 term)
        w1 = W1g.to(torch.bfloat16).to(dt)
        W1g = w1 + (W1g - w1).to(torch.bfloat16).to(dt)
    z1 = X @ W1g.T + f(P.b1)
    for a in adds:
        z1 = z1 + a
    if defect == "last_column_tile_without_bias":   # the ragged last 128-column tile of z1
        z1 = z1.clone()
        n0 = 128 * ((c.hid - 1) // 128)
        z1[..., n0:] -= f(P.b1)[n0:]
    A1 =X.abs() @ W1g.abs().T + f(P.b1).abs() + sum(a.abs() for a in adds)
    E_z1 = (U * (P.kg + len(adds) + 2) + MODE_TERM[ns]) * A1
    z1_stored, E_z1_stored = z1, E_z1
    if c.sbf:
        E_z1_stored = E_z1 + UB * (z1.abs() + E_z1)
        if dt != torch.float64:
            z1_stored = to_bf16(z1, truncate=defect == "z1_truncated_bf16")
    if z1_given is not None:
        z1 = f(z1_given)
        z1_stored, E_z1 = z1, (UB * z1.abs() if c.sbf else torch.zeros_like(A1))
    if c.no_act:
        h, E_h = z1, E_z1
    else:
        sg = torch.sigmoid(z1)
        h = z1 * sg
        E_h = (sg * (1 + z1 * (1 - sg))).abs() * E_z1 + (T_SILU + 2 * U * z1.abs()) * h.abs()
    W2, b2 = f(P.W2), f(P.b2)
    y = h @ W2.T + b2
    if defect == "drop_dout_block_in_gemm2":   # the second 32-column block of dout never accumulated
        y = y.clone()
        y[..., 32:64] = b2[32:64]
    E_y = E_h @ W2.abs().T + (U * (c.hid + 2) + MODE_TERM[ns]) * (h.abs() @ W2.abs().T + b2.abs())
    val, bud = {"z1": z1_stored}, {"z1": E_z1_stored}
    if c.ln:
        mean = y.mean(-1, keepdim=True)
        d = y - mean
        var = (d * d).mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + (0.0 if defect == "rstd_without_eps" else P.eps))
        xhat = d * rstd
        g, be = f(P.gamma), f(P.beta)
        m = xhat * g + be
        t_ln = U * (c.dout + 8)   # the row statistics: two sums over dout, the approximate rsqrt, eps
        E_d = E_y + E_y.mean(-1, keepdim=True) + U * (c.dout + 4) * (y.abs() + y.abs().mean(-1, keepdim=True))
        E_xhat = rstd * (E_d + xhat.abs() * (xhat.abs() * E_d).mean(-1, keepdim=True)) + t_ln * xhat.abs()
        E_rstd = rstd * rstd * (xhat.abs() * E_d).mean(-1, keepdim=True) + t_ln * rstd
        E_m = g.abs() * E_xhat + 2 * U * ((g * xhat).abs() + be.abs())
        val.update(xhat=to_bf16(xhat) if (c.sbf and dt != torch.float64) else xhat, rstd=rstd[..., 0])
        bud.update(xhat=E_xhat + UB * (xhat.abs() + E_xhat) if c.sbf else E_xhat, rstd=E_rstd[..., 0])
        if dt == torch.float64:
            P.var_min = float(var.min())   # the budget is first order in 1 / (var + eps): the builder of a case checks this
    else:
        m, E_m = y, E_y
    if c.add1 and defect != "omit_residual":
        m = m + xs[1]
        E_m = E_m + U * m.abs()
    if c.aggregate:
        mm_, Em_ = m, m.abs()
        if defect == "tile_last_row_not_aggregated":   # the last row of the second tile
            t = P.tiles[1]
            mm_ = m.clone()
            mm_[:, int(t[0]) + int(t[1]) - 1] = 0
        sc = f(P.scale)[None, :, None]
        val["aggr"] = sc * _segsum(mm_, P.seg_of_row, P.nseg)
        bud["aggr"] = sc * _segsum(E_m, P.seg_of_row, P.nseg) + U * (f(P.deg)[None, :, None] + 4) * sc * _segsum(Em_, P.seg_of_row, P.nseg)
    if c.want_out:
        o, E_o = m, E_m
        if c.add0 and defect != "omit_residual":
            o = m + xs[0]
            E_o = E_m + U * o.abs()
        if P.out_idx is not None:
            out, E_out = torch.empty_like(o), torch.empty_like(E_o)
            out[:, P.out_idx], E_out[:, P.out_idx] = o, E_o
            o, E_o = out, E_out
        val["out"], bud["out"] = o, E_o
    if dt != torch.float64:
        bud = None
    return val, bud


def backward_math(P, saved, dt=torch.float64, ns=0, defect=None, nblk=1):
    """Backward from the saved z1 / xhat / rstd that are handed in -> (values, budgets) over dz1, dz2, dsrc0.., db1, db2, dgamma,
    dbeta (the four vectors summed over rows in this precision).  nblk: the workgroups of the launch (each sums its rows in fp32)."""
    c = P.case
    f = lambda t: t.to(dt)
    xs_shape = [(P.batch, P.rows, w) for w in c.widths]
    z1 = f(saved["z1"])
    zero = torch.zeros((P.batch, P.rows, c.dout), dtype=dt)
    go = zero
    if P.g_out is not None:
        go = f(P.g_out)[:, P.out_idx] if P.out_idx is not None else f(P.g_out)
    dm, E_dm = go, torch.zeros_like(zero)
    if P.g_aggr is not None:
        sc = torch.ones_like(P.scale) if defect == "mean_scale_missing_in_backward" else P.scale
        ga = (f(P.g_aggr) * f(sc)[None, :, None])[:, P.seg_of_row]
        dm = go + ga
        E_dm = (U * ga.abs() if c.mean else 0) + (U * dm.abs() if P.g_out is not None else 0) + E_dm
    val, bud = {}, {}
    rows_blk = 32 * -(-P.ntiles * P.batch // nblk) + 8   # rows one workgroup sums in fp32 before its partial is written
    vsum = lambda t: t.sum((0, 1))
    if c.ln:
        xhat, rstd, g = f(saved["xhat"]), f(saved["rstd"])[..., None], f(P.gamma)
        dxh = dm * g
        c1, c2 = dxh.mean(-1, keepdim=True), (dxh * xhat).mean(-1, keepdim=True)
        dz2 = rstd * (dxh - c1 - xhat * c2)
        E_dxh = g.abs() * E_dm + U * dxh.abs()
        mag = dxh.abs() + dxh.abs().mean(-1, keepdim=True) + xhat.abs() * (dxh * xhat).abs().mean(-1, keepdim=True)
        E_dz2 = rstd * (E_dxh + E_dxh.mean(-1, keepdim=True) + xhat.abs() * (xhat.abs() * E_dxh).mean(-1, keepdim=True)) + U * (c.dout + 8) * rstd * mag
        val.update(dgamma=vsum(dm * xhat), dbeta=vsum(dm))
        bud.update(dgamma=vsum(E_dm * xhat.abs()) + U * rows_blk * vsum((dm * xhat).abs()), dbeta=vsum(E_dm) + U * rows_blk * vsum(dm.abs()))
    else:
        dz2, E_dz2 = dm, E_dm
    W2 = f(P.W2)
    dh = dz2 @ W2
    if defect == "w2_untransposed_in_dz1":   # the (dout, hid) rows of W2 read as (hid, dout) rows
        dh = dz2 @ W2.reshape(c.hid, c.dout).T
    E_dh = E_dz2 @ W2.abs() + (U * (c.dout + 2) + MODE_TERM[ns]) * (dz2.abs() @ W2.abs())
    if c.no_act:
        dz1, E_dz1 = dh, E_dh
    else:
        sg = torch.sigmoid(z1)
        sp = sg if defect == "sigmoid_for_silu_derivative" else sg * (1 + z1 * (1 - sg))
        dz1 = dh * sp
        E_dz1 = sp.abs() * E_dh + (T_SILU + 2 * U * z1.abs()) * dh.abs() * (sg + z1.abs() * sg * (1 - sg)) + U * dz1.abs()
    st = (lambda t: to_bf16(t)) if (c.sbf and dt != torch.float64) else (lambda t: t)   # dz1 / dz2 leave as bf16 rows; the sums and
    sb = (lambda t, e: e + UB * (t.abs() + e)) if c.sbf else (lambda t, e: e)              # the data gradients use what the kernel holds
    val.update(dz1=st(dz1), dz2=st(dz2), db1=vsum(dz1), db2=vsum(dz2))
    bud.update(dz1=sb(dz1, E_dz1), dz2=sb(dz2, E_dz2), db1=vsum(E_dz1) + U * rows_blk * vsum(dz1.abs()), db2=vsum(E_dz2) + U * rows_blk * vsum(dz2.abs()))
    W1g = f(P.W1[:, : P.kg])
    dX = dz1 @ W1g
    E_dX = E_dz1 @ W1g.abs() + (U * (c.hid + 2) + MODE_TERM[ns]) * (dz1.abs() @ W1g.abs())
    off = 0
    for k, w in enumerate(c.widths):
        if c.pre and k > 0:
            dx, E_dx = dz1, E_dz1
        else:
            dx, E_dx = dX[..., off: off + w], E_dX[..., off: off + w]
            off += w
        if k == 0 and c.add0 and P.g_out is not None and defect != "omit_residual":
            dx = dx + go
            E_dx = E_dx + U * dx.abs()
        if k == 1 and c.add1 and defect != "omit_residual":
            dx = dx + dm
            E_dx = E_dx + E_dm + U * dx.abs()
        assert dx.shape == xs_shape[k]
        mode, idx = c.dmode[k], P.srcs[k].idx
        if mode == 0:
            continue
        if mode == 1 and idx is not None:
            if defect == "dmode1_scatter_through_wrong_index":   # another source's index (identity where that source has none)
                other = P.srcs[(k + 1) % P.nsrc].idx
                idx = other if (other is not None and other.unique().numel() == P.rows) else torch.arange(P.rows)
            o, E_o = torch.empty_like(dx), torch.empty_like(E_dx)
            o[:, idx], E_o[:, idx] = dx, E_dx
            dx, E_dx = o, E_o
        if k == 0 and c.acc0:   # NLAM_F_ACC_DSRC0: added to what dsrc[0] holds
            if defect != "dsrc0_overwritten":
                dx = dx + f(P.dsrc0_init)
            E_dx = E_dx + U * dx.abs()
        if mode == 3:
            E_dx = _segsum(E_dx, P.seg_of_row, P.nseg) + U * (f(P.deg)[None, :, None] + 4) * _segsum(dx.abs(), P.seg_of_row, P.nseg)
            dx = _segsum(dx, P.seg_of_row, P.nseg)
        val[f"dsrc{k}"], bud[f"dsrc{k}"] = dx, E_dx
    if dt != torch.float64:
        bud = None
    return val, bud


def block_vectors(P, val_rows, nblk, skip=None):
    """The stand-in's vec_partials: rows dealt to nblk workgroups, each summing its share (float32); `skip`: a block left out."""
    out = {}
    for name, t in val_rows.items():
        flat = t.reshape(-1, t.shape[-1])
        parts = [ch.sum(0) for ch in torch.chunk(flat, nblk, 0)]
        out[name] = torch.stack([q for i, q in enumerate(parts) if i != skip]).double().sum(0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison functions (tier a, tier b): they return the names of the quantities that fail
# ---------------------------------------------------------------------------------------------------------------------------
def exact_quantities(case, forward):
    """Tier (a): what must be bit-equal to the float64 result."""
    chain = case.no_act and not case.ln and not case.mean
    if forward:
        return ["z1"] + (["out", "aggr"] if chain else [])
    if chain:
        return ["dz2", "dz1", "dsrc0", "dsrc1", "dsrc2", "db1", "db2"]
    if not case.ln and not case.mean:   # dz2 is a gather and add of integer gradients
        return ["dz2", "db2"]
    return []


def compare_exact(got, ref, names):
    bad = []
    for n in names:
        if n in ref and not (n in got and got[n].shape == ref[n].shape and torch.equal(got[n].double(), ref[n])):
            bad.append(n)
    return bad


def compare_bounded(got, ref, bud, names=None, note=None):
    """Tier (b): |got - R| <= bound element by element; a NaN (an unwritten element) fails.  note(name, ratio) records the
    largest |got - R| / bound."""
    bad = []
    for n in (names if names is not None else ref.keys()):
        if n not in ref:
            continue
        if n not in got or got[n].shape != ref[n].shape:
            bad.append(n)
            continue
        err = (got[n].double() - ref[n]).abs()
        bound = bud[n] + 2.0 ** -50 * ref[n].abs() + 1e-300   # + the float64 evaluation of the reference itself
        if not bool((err <= bound).all()):
            bad.append(n)
        if note is not None:
            r = (err / bound)
            note(n, float(r[torch.isfinite(r)].max()) if torch.isfinite(r).any() else float("inf"))
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# the launch descriptors (shared by the plan-table test, which fills them with placeholder addresses, and the GPU launches)
# ---------------------------------------------------------------------------------------------------------------------------
def case_flags(c, backward=False):
    return ((c.mm << 8) | (L.F_STORE_BF16 if c.sbf else 0) | (L.F_ACC_DSRC0 if (c.acc0 and backward) else 0) | (L.F_ADD_SRC0 if c.add0 else 0) | (L.F_ADD_SRC1 if c.add1 else 0) | (L.F_MEAN if c.mean else 0)
            | (L.F_NO_ACT if c.no_act else 0) | (L.F_PRE_ADD if c.pre else 0))


def describe_fwd(P, a):
    """nlam_mlp_fwd_t of the problem; a: name -> device address (or None)."""
    c = P.case
    p = L.MlpFwd()
    for k, s in enumerate(P.srcs):
        p.src[k].ptr, p.src[k].idx, p.src[k].bstride, p.src[k].width = a(f"src{k}"), a(f"idx{k}"), s.bstride, s.width
    p.nsrc, p.batch, p.rows, p.ntiles, p.tiles = P.nsrc, P.batch, P.rows, P.ntiles, a("tiles")
    p.W1, p.b1, p.W2, p.b2 = a("W1"), a("b1"), a("W2"), a("b2")
    p.ln_w, p.ln_b = (a("gamma"), a("beta") if c.ln_beta else None) if c.ln else (None, None)
    p.eps, p.hid, p.dout, p.flags = 1e-5, c.hid, c.dout, case_flags(c)
    p.ldw1 = P.ldw1 if (c.pre or c.ldw1_pad) else 0
    if c.want_out:
        p.out, p.out_idx, p.out_bstride = a("out"), a("out_idx"), P.out_rows * c.dout
    if c.aggregate:
        p.aggr, p.rowptr, p.inv_deg, p.nseg_total = a("aggr"), a("rowptr"), a("inv_deg"), P.nseg_rows
    p.z1 = a("z1")
    if c.ln:
        p.xhat, p.rstd = a("xhat"), a("rstd")
    if c.cat:
        p.src[0].ptr, p.src[0].bstride = None, P.rows * c.widths[0]
        p.ncat = len(c.cat)
        for q, w in enumerate(c.cat):
            p.cat_ptr[q], p.cat_width[q] = a(f"piece{q}"), w
            p.cat_bstride[q] = 0 if q in c.cat_shared else P.rows * w
        p.cat_out = a("cat_out")
    return p


def describe_bwd(P, a, lib):
    """nlam_mlp_bwd_t of the problem, dz2_ld from nlam_mlp_bwd_dz2_ld."""
    c = P.case
    p = L.MlpBwd()
    for k, s in enumerate(P.srcs):
        p.src[k].ptr, p.src[k].idx, p.src[k].bstride, p.src[k].width = a(f"src{k}"), a(f"idx{k}"), s.bstride, s.width
    if c.cat:   # the backward reads the concatenated rows the forward wrote
        p.src[0].ptr, p.src[0].bstride = a("cat_out"), P.rows * c.widths[0]
    p.nsrc, p.batch, p.rows, p.ntiles, p.tiles = P.nsrc, P.batch, P.rows, P.ntiles, a("tiles")
    p.W1, p.W2, p.ln_w = a("W1"), a("W2"), a("gamma") if c.ln else None
    p.hid, p.dout, p.flags, p.nseg_total = c.hid, c.dout, case_flags(c, backward=True), P.nseg
    p.ldw1 = P.ldw1 if (c.pre or c.ldw1_pad) else 0
    if c.g_out:
        p.g_out, p.out_idx, p.out_bstride = a("g_out"), a("out_idx"), P.out_rows * c.dout
    if c.g_aggr:
        p.g_aggr, p.seg_of_row = a("g_aggr"), a("seg_of_row")
    if c.graph or c.rowseg:
        p.rowptr, p.inv_deg = a("rowptr"), a("inv_deg")
    p.z1 = a("z1")
    if c.ln:
        p.xhat, p.rstd = a("xhat"), a("rstd")
    p.dz1, p.dz2 = a("dz1"), a("dz2")
    for k in range(P.nsrc):
        p.dmode[k] = c.dmode[k]
        if c.dmode[k] != 0:
            p.dsrc[k], p.dsrc_bstride[k] = a(f"dsrc{k}"), dsrc_rows(P, k) * c.widths[k]
    p.dz2_ld = lib.nlam_mlp_bwd_dz2_ld(C.byref(p))
    return p


def dsrc_rows(P, k):
    mode = P.case.dmode[k]
    return {1: P.srcs[k].nr, 2: P.rows, 3: P.nseg_rows}[mode]


# ---------------------------------------------------------------------------------------------------------------------------
# GPU side: device copies, NaN-filled guarded outputs, the launches
# ---------------------------------------------------------------------------------------------------------------------------
class Dev:
    """Device copies of a problem's operands; every output is a NaN-filled torch.empty buffer with GUARD NaN floats behind it."""

    def __init__(self, P):
        self.P, self.t, self.outs = P, {}, {}
        c = P.case
        f32 = lambda x: x.to(torch.float32).contiguous().cuda()
        i32 = lambda x: x.to(torch.int32).contiguous().cuda()
        for k, s in enumerate(P.srcs):
            self.t[f"src{k}"] = f32(s.S.reshape(-1))
            if s.idx is not None:
                self.t[f"idx{k}"] = i32(s.idx)
        for n in ("W1", "b1", "W2", "b2", "gamma", "beta", "g_out", "g_aggr"):
            if getattr(P, n) is not None:
                self.t[n] = f32(getattr(P, n))
        if P.tiles is not None:
            self.t["tiles"] = i32(P.tiles)
        if P.rowptr_dev is not None:
            self.t["rowptr"], self.t["inv_deg"], self.t["seg_of_row"] = i32(P.rowptr_dev), f32(P.inv_deg_dev), i32(P.seg_of_row)
            if P.comb is not None:
                self.comb = [i32(x) for x in P.comb]
        if P.out_idx is not None:
            self.t["out_idx"] = i32(P.out_idx)
        for q, piece in enumerate(getattr(P, "pieces", [])):
            self.t[f"piece{q}"] = f32(piece.reshape(-1))
        assert c.batch == P.batch

    def out(self, name, shape, zero=False, dtype=torch.float32):
        n = int(np.prod(shape))
        buf = torch.empty(n + GUARD, device="cuda", dtype=dtype)
        buf.fill_(float("nan"))
        if zero:   # the atomic adds of NLAM_TILE_SPLIT tiles meet in a zeroed buffer
            buf[:n] = 0
        self.outs[name] = (buf, n, tuple(shape))
        self.t[name] = buf[:n].view(shape)
        return self.t[name]

    def addr(self, name):
        t = self.t.get(name)
        return None if t is None else t.data_ptr()

    def guards_intact(self):
        return [n for n, (buf, k, _) in self.outs.items() if not bool(torch.isnan(buf[k:]).all())]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _combine(lib, dev, buf, width):
    ptr, src, dst = dev.comb
    P = dev.P
    assert lib.nlam_split_combine(buf.data_ptr(), P.nseg_rows * width, ptr.data_ptr(), src.data_ptr(), dst.data_ptr(), int(dst.numel()),
                                  width, P.batch, _stream()) == 0


def _written(res, what):
    bad = [n for n, t in res.items() if torch.is_tensor(t) and not bool(torch.isfinite(t).all())]
    assert bad == [], f"{what}: unwritten (NaN) elements in {bad}"


def _same(a, b):
    return [n for n in a if torch.is_tensor(a[n]) and not torch.equal(a[n], b[n])]


def _saved_dev(res):
    return {n: res[n].cuda() for n in ("z1", "xhat", "rstd") if n in res}


# ---------------------------------------------------------------------------------------------------------------------------
# the tiers' problems and references, and the CPU stand-in for a kernel (shared by the wide and the tiled-GEMM files)
# ---------------------------------------------------------------------------------------------------------------------------
def int_problem(case, seed):
    """Tier (a): the largest integer range of 4, 2, 1 for which every sum of absolute values of the quantities compared exactly
    stays below 2^24 (exact_headroom, float64): every partial sum, in any order, is then an exact fp32 value."""
    for r in (4, 2, 1):
        P = build_problem(case, seed, "int", irange=r)
        if exact_headroom(P) < 2.0 ** 24:
            return P
    raise AssertionError(f"{case}: no integer range keeps the sums below 2^24")


def exact_headroom(P):
    c = P.case
    xs = _gathered(P, torch.float64, None)
    X = xs[0] if c.pre else torch.cat(xs, -1)
    W1 = P.W1[:, : P.kg].abs()
    A = X.abs() @ W1.T + P.b1.abs() + sum(a.abs() for a in (xs[1:] if c.pre else []))
    top = float(A.max())
    chain = c.no_act and not c.ln and not c.mean
    if c.ln or c.mean:
        return top
    go = P.g_out.abs() if P.g_out is not None else 0
    if P.g_out is not None and P.out_idx is not None:
        go = go[:, P.out_idx]
    dm = go + (P.g_aggr.abs()[:, P.seg_of_row] if P.g_aggr is not None else 0)
    top = max(top, float(dm.sum((0, 1)).max()))   # db2
    if not chain:
        return top
    Y = A @ P.W2.abs().T + P.b2.abs() + (xs[1].abs() if c.add1 else 0)
    top = max(top, float(Y.max()) + (float(xs[0].abs().max()) if c.add0 else 0))
    if c.aggregate:
        top = max(top, float(_segsum(Y, P.seg_of_row, P.nseg).max()))
    dh = dm @ P.W2.abs()
    dX = dh @ W1 + float(dm.max())
    top = max(top, float(dh.sum((0, 1)).max()), float(dX.max()))
    if 3 in c.dmode:
        top = max(top, float(_segsum(dX, P.seg_of_row, P.nseg).max()))
    return top


def rand_problem(case, seed):
    """Tier (b): the budget is first order in 1 / (var + eps), so the pre-LayerNorm row variance must be well above eps."""
    P = build_problem(case, seed, "rand")
    if case.ln:
        forward_math(P)
        assert P.var_min > 1e3 * P.eps, f"{case}: a row variance of {P.var_min:.3g} is too close to eps for a first-order bound"
    return P


def exact_reference(case, ref, forward):
    """Tier (a): the float64 values as the kernel must store them -- with bf16 storage, rounded once to nearest even."""
    if forward and case.sbf:
        ref = {**ref, "z1": to_bf16(ref["z1"])}
    return ref


def low_reference(P, ns):
    """Tier (c): z1 of the probe.  Three terms and fp32 keep every term of W1: the float64 value; one term keeps the leading
    one: +-count + integers."""
    ref, _ = forward_math(P)
    z1 = ref["z1"]
    if ns == 1:
        P1 = replace_weights(P, torch.sign(P.W1))
        z1 = forward_math(P1)[0]["z1"]
    assert float(z1.abs().max()) < (LOW_ONES + 16) * LOW_W and torch.equal(z1.float().double(), z1), "the probe's z1 must be an exact fp32 value"
    return to_bf16(z1) if P.case.sbf else z1


def replace_weights(P, W1):
    Q = type(P)(**vars(P))
    Q.W1 = W1
    return Q


def replace_case(P, **kw):
    Q = type(P)(**vars(P))
    Q.case = replace(P.case, **kw)
    return Q


STANDIN_NBLK = 16


def standin_run(case, kind, defect=None, ns_claimed=0, nblk=STANDIN_NBLK):
    """The MLP in torch fp32 on the CPU (bf16 rounding where the case stores bf16) with an optional defect, compared like a kernel ->
    names of the failing quantities, forward first.  nblk: the workgroups the stand-in deals the rows of the four vectors to."""
    P = int_problem(case, 7) if kind == "int" else rand_problem(case, 7) if kind == "rand" else build_problem(case, 7, kind)
    ref_f, bud_f = forward_math(P, ns=ns_claimed)
    got_f, _ = forward_math(P, torch.float32, defect=defect)
    if kind == "low":
        return [] if torch.equal(got_f["z1"].double(), low_reference(P, ns_claimed)) else ["z1"]
    saved = {k: got_f[k] for k in ("z1", "xhat", "rstd") if k in got_f}
    ref_b, bud_b = backward_math(P, {k: v.double() for k, v in saved.items()}, ns=ns_claimed, nblk=nblk)
    got_b, _ = backward_math(P, saved, torch.float32, defect=defect)
    c = case
    dm = 0   # a case may have g_out only, g_aggr only, or both
    if P.g_out is not None:
        dm = P.g_out[:, P.out_idx] if P.out_idx is not None else P.g_out
    if P.g_aggr is not None:
        dm = dm + (P.g_aggr * P.scale[None, :, None])[:, P.seg_of_row]
    dm = dm.float()
    # the four vectors as a kernel leaves them: per-workgroup partial sums of what it holds in fp32, summed in float64
    unrounded = got_b if not c.sbf else backward_math(replace_case(P, sbf=False), saved, torch.float32, defect=defect)[0]
    rows = {"db1": unrounded["dz1"], "db2": unrounded["dz2"]}
    if c.ln:
        rows.update(dgamma=dm * saved["xhat"], dbeta=dm)
    got_b.update(block_vectors(P, rows, nblk, skip=1 if defect == "skip_vec_partials_block" else None))
    if kind == "int":
        return (compare_exact(got_f, exact_reference(c, ref_f, True), exact_quantities(c, True))
                + compare_exact(got_b, ref_b, exact_quantities(c, False)))
    return compare_bounded(got_f, ref_f, bud_f) + compare_bounded(got_b, ref_b, bud_b)
