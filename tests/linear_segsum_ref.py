"""Shared machinery of test_linear_kernels.py and test_segment_sum_kernels.py: the case records, the problem builders, the float64
math of the contracts of include/nlam_hip.h (nlam_linear, nlam_segment_sum*, nlam_split_combine) with their first-order error
budgets, the CPU stand-ins for a kernel (torch fp32, split into bf16 terms where a matrix mode asks for it) with injected defects,
and the guarded device buffers.  The constants, the comparison functions and the NaN-filled guarded buffers are those of
mlp_kernel_ref.py; no constant is refitted here.  A plain module; nothing here is collected by pytest."""
from dataclasses import dataclass
from types import SimpleNamespace as NS

import torch

from neural_lam_amd import _lib as L

from mlp_kernel_ref import GUARD, LOW_W, MODE_TERM, SPLIT_SAFETY, U, UB, Dev, compare_bounded, compare_exact, to_bf16  # noqa: F401

CROSS_W = 1.0 + 2.0 ** -9          # two bf16 terms (1, 2^-9): its square 1 + 2^-8 + 2^-18 needs the product of the two second terms
PROBE_ONES = 16                    # non-zero entries per row of x in the low-order probes
PAD_ROWS = 3                       # rows of `out` behind `rows`: NaN before and after every launch


# ---------------------------------------------------------------------------------------------------------------------------
# nlam_linear
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LinCase:
    name: str
    kernel: tuple              # ("bf",) | ("bfw", resident) | ("gemm", WN, SK of the one-term instantiation)
    k: int
    n: int
    rows: int
    modes: tuple = (1, 2, 3)   # requested NLAM_F_MM_BF16X<ns>
    layout: str = "f"          # f: ldk = 1, ldn = k + 32 (a column block of a wider W1); t: ldn = 1, ldk = n + 32 (the data gradient);
    #                            f2: ldk = 2, ldn = 2 k + 4
    woff: int = 32             # floats between the 16-byte aligned start of the weight buffer and W
    dual: bool = False
    tune: tuple = ()           # (key, value) pairs for nlam_set_tuning, in this order

    def __str__(self):
        return self.name

    def strides(self):
        """-> (ldn, ldk, floats of a weight buffer)"""
        ldn, ldk = {"f": (self.k + 32, 1), "t": (1, self.n + 32), "f2": (2 * self.k + 4, 2)}[self.layout]
        return ldn, ldk, self.woff + (self.n - 1) * ldn + (self.k - 1) * ldk + 1

    def code(self, ns):
        """The nlam_linear_plan code the case is built for."""
        if self.kernel[0] == "bf":
            return L.linp_bf(ns, self.k // 32, self.n // 32)
        if self.kernel[0] == "bfw":
            return L.linp_bfw(ns, self.kernel[1], self.dual)
        wn, sk1 = self.kernel[1:]
        return L.linp_gemm(ns, wn, sk1 if (ns == 1 and wn == 1) else 2, self.layout == "t", self.dual)


def lin_matrix(c, Wbuf, swap=False):
    """A[h][c] = W[h * ldn + c * ldk] out of the flat buffer, addressed through the strides (swap: ldn and ldk exchanged, an
    injected defect; indices wrap inside the buffer)."""
    ldn, ldk, size = c.strides()
    if swap:
        ldn, ldk = ldk, ldn
    idx = c.woff + torch.arange(c.n)[:, None] * ldn + torch.arange(c.k)[None, :] * ldk
    return Wbuf[idx % size]


def lin_headroom(c):
    """Tier (a): the largest r <= 127 with k r^2 + r < 2^24 (accumulated twice: 2 k r^2 + r): every partial sum, in any order, is
    an exact fp32 value, and every operand a single bf16 term."""
    r = 127
    while 2 * c.k * r * r + r >= 2 ** 24:
        r -= 1
    return r


def lin_problem(c, seed, kind):
    """kind: "int" (tier a), "rand" (tier b), "low_w" / "low_x" / "cross" (tier c, exact at any K: at most PROBE_ONES non-zero
    entries per row of x, every weight the same magnitude with one sign per output feature)."""
    gen = torch.Generator().manual_seed(seed)
    ldn, ldk, size = c.strides()
    P = NS(case=c, kind=kind)
    shape_x, shape_o = (c.rows, c.k), (c.rows, c.n)
    if kind == "int":
        r = P.r = lin_headroom(c)
        ri = lambda shape: torch.randint(-r, r + 1, shape, generator=gen).double()
        P.x, P.W, P.W2, P.prev, P.prev2 = ri(shape_x), ri((size,)), ri((size,)), ri(shape_o), ri(shape_o)
    elif kind == "rand":
        cs = 2.0 ** torch.randint(-3, 4, (c.k,), generator=gen).double()   # a scale per column of x
        rn = lambda shape: torch.randn(shape, generator=gen, dtype=torch.float64)
        P.x = (rn(shape_x) * cs).float().double()
        P.W, P.W2 = ((rn((size,)) / c.k ** 0.5).float().double() for _ in range(2))
        P.prev, P.prev2 = (rn(shape_o).float().double() for _ in range(2))
    else:
        wv, xv = {"low_w": (LOW_W, 1.0), "low_x": (1.0, LOW_W), "cross": (CROSS_W, CROSS_W)}[kind]
        n1 = min(PROBE_ONES, c.k)
        pos = (torch.arange(c.rows)[:, None] * 5 + 3 + torch.arange(n1)[None, :] * max(1, c.k // n1)) % c.k   # every K group is hit by some row
        P.x = torch.zeros(shape_x, dtype=torch.float64).scatter_(1, pos, xv)
        # one sign per output feature: the buffer is filled through the case's own addressing
        sign = 1.0 - 2.0 * (torch.arange(c.n) % 2).double()
        idx = c.woff + torch.arange(c.n)[:, None] * ldn + torch.arange(c.k)[None, :] * ldk
        P.W = torch.full((size,), wv, dtype=torch.float64)
        P.W[idx] = (sign[:, None] * wv).expand(c.n, c.k)
        P.W2 = -P.W
        P.prev = P.prev2 = None
        P.count, P.sign = n1, sign
    for t in (P.x, P.W, P.W2):
        assert torch.equal(t.float().double(), t)
    return P


def split_terms(t, ns):
    """t (fp32) as ns bf16 terms, each the remainder rounded to nearest even (split_pair)."""
    out, rest = [], t.float()
    for _ in range(ns):
        q = to_bf16(rest)
        out.append(q)
        rest = rest - q
    return out


def split_matmul(x, A, ns, drop_cross=False):
    """sum over p + q < ns of x_p @ A_q^T in fp32 (mma_split_lds); drop_cross: without the product of the two second terms."""
    xs, As = split_terms(x, ns), split_terms(A, ns)
    acc = torch.zeros((x.shape[0], A.shape[0]), dtype=torch.float32)
    for o in range(ns):
        for p in range(o + 1):
            if drop_cross and ns == 3 and p == 1 and o - p == 1:
                continue
            acc = acc + xs[p] @ As[o - p].T
    return acc


LIN_DEFECTS = ("ragged_last_row_from_neighbour", "out2_from_first_weights", "accumulate_overwrites", "skip_last_k_chunk",
               "swap_ldn_ldk", "drop_third_term", "drop_second_terms_product", "skip_padding_group_row_tile")


def linear_math(P, dt=torch.float64, ns=3, defect=None, accumulate=False):
    """-> (values, budgets) over out (and out2 of a dual case): R = x @ A^T (+ prev), A addressed through the strides.  float64:
    the reference, with the budget (U (k + 2) + MODE_TERM[ns]) (|x| @ |A|^T) (+ U |R| when accumulating) -- the z1 budget of
    mlp_kernel_ref.forward_math without bias and addends.  float32: the stand-in for a kernel that executes ns terms."""
    c = P.case
    val, bud = {}, {}
    x = P.x
    if defect == "ragged_last_row_from_neighbour" and c.rows >= 2:   # the clamped read's value kept for the last row
        x = x.clone()
        x[-1] = x[-2]
    if defect == "skip_last_k_chunk":
        x = x.clone()
        x[:, c.k - 32:] = 0
    for name, Wbuf, prev in (("out", P.W, P.prev), ("out2", P.W2, P.prev2)):
        if name == "out2" and not c.dual:
            continue
        if name == "out2" and defect == "out2_from_first_weights":
            Wbuf = P.W
        A = lin_matrix(c, Wbuf, swap=defect == "swap_ldn_ldk")
        if dt == torch.float64:
            if defect is None:   # the two float64 products once per problem, whatever mode and accumulation they are asked for
                cache = P.__dict__.setdefault("_products", {})
                if name not in cache:
                    cache[name] = (x @ A.T, x.abs() @ A.abs().T)
                R, mag = cache[name]
            else:
                R, mag = x @ A.T, x.abs() @ A.abs().T
            bound = (U * (c.k + 2) + MODE_TERM[ns]) * mag
            if accumulate:
                R = R + prev
                bound = bound + U * R.abs()
            val[name], bud[name] = R, bound
            continue
        ex = 2 if (defect == "drop_third_term" and ns == 3) else ns
        R = split_matmul(x, A, ex, drop_cross=defect == "drop_second_terms_product")
        if accumulate and defect != "accumulate_overwrites":
            R = R + prev.float()
        if defect == "skip_padding_group_row_tile":   # the last 64-row tile is one of the group of eight that is padded: left unwritten
            R = R.clone()
            R[64 * ((c.rows - 1) // 64):] = prev.float()[64 * ((c.rows - 1) // 64):] if accumulate else float("nan")
        val[name] = R
    return val, (bud if dt == torch.float64 else None)


def probe_value(kind, ns):
    """What one contributing (x entry, weight) pair of a tier-(c) probe adds on ns executed terms, derived in float64 from the
    terms: the products x_p * w_q with p + q < ns."""
    wv, xv = {"low_w": (LOW_W, 1.0), "low_x": (1.0, LOW_W), "cross": (CROSS_W, CROSS_W)}[kind]
    tw = [t.double() for t in split_terms(torch.tensor([wv]), 3)]
    tx = [t.double() for t in split_terms(torch.tensor([xv]), 3)]
    assert float(sum(tw)) == wv and float(sum(tx)) == xv, "three bf16 terms hold the probe values exactly"
    return float(sum(tx[p] * tw[q] for p in range(ns) for q in range(ns) if p + q < ns))


def probe_reference(P, ns):
    """Tier (c): every output of row r, feature h is sign[h] * count * probe_value (out2: the opposite sign); exact in fp32."""
    c = P.case
    v = probe_value(P.kind, ns)
    R = (P.sign * (P.count * v))[None, :].expand(c.rows, c.n).contiguous()
    assert torch.equal(R.float().double(), R), "the probe's expectation must be an exact fp32 value"
    for m in range(1, P.count + 1):   # and so is every partial sum, whatever the order
        assert float(torch.tensor(m * v).float()) == m * v
    return {"out": R, "out2": -R} if c.dual else {"out": R}


def lin_standin(c, kind, ns, defect=None, accumulate=False):
    """The stand-in compared like a kernel -> names of the failing outputs."""
    P = lin_problem(c, 11, kind)
    got, _ = linear_math(P, torch.float32, ns, defect, accumulate)
    if kind in ("low_w", "low_x", "cross"):
        return compare_exact(got, probe_reference(P, ns), ["out", "out2"])
    ref, bud = linear_math(P, ns=ns, accumulate=accumulate)
    if kind == "int":
        return compare_exact(got, ref, ["out", "out2"])
    return compare_bounded(got, ref, bud)


def describe_linear(c, ns, addr, accumulate=False, dual=None):
    """nlam_linear_t of the case; addr: name -> address of x, W, W2 (the aligned buffer starts), out, out2."""
    ldn, ldk, _ = c.strides()
    p = L.Linear()
    p.x, p.W, p.out = addr("x"), addr("W") + 4 * c.woff, addr("out")
    p.rows, p.ldn, p.ldk, p.k, p.n = c.rows, ldn, ldk, c.k, c.n
    p.accumulate, p.flags = int(accumulate), ns << 8
    if c.dual if dual is None else dual:
        p.W2, p.out2 = addr("W2") + 4 * c.woff, addr("out2")
    return p


class Bufs(Dev):
    """Device buffers by name: inputs copied as they are, outputs NaN-filled with GUARD NaN floats behind them (Dev.out)."""

    def __init__(self):
        self.t, self.outs = {}, {}

    def put(self, name, t, dtype=torch.float32):
        self.t[name] = t.to(dtype).contiguous().cuda()
        return self.t[name]


# ---------------------------------------------------------------------------------------------------------------------------
# nlam_segment_sum, _acc, _add, _bf16 and nlam_split_combine
# ---------------------------------------------------------------------------------------------------------------------------
PLAIN_CYCLE = (0, 1, 7, 8, 9, 15, 16, 17, 0)     # the 8-row batches of segment_sum_kernel / segment_sum_bf16_kernel and their tails


def split_cycle(S):
    """The 8-row batches of segment_sum_split_kernel<S>: a lane group's rows are S apart."""
    return (0, 8 * S - 3, 8 * S - 1, 8 * S, 8 * S + 1, 8 * S + S - 1, 8 * S + S, 16 * S + 1, 1)


@dataclass(frozen=True)
class SegCase:
    name: str
    groups: int                # nlam_segment_sum_groups the case is built for (1, 2, 4); 0: the bf16 kernel
    width: int
    lens: tuple
    entry: str = "sum"         # sum | acc | add | bf16
    batch: int = 2
    shared: bool = False       # in_bstride = 0: one input for every batch item
    pad: int = 8               # floats between batch items of the input beyond rows * width
    order: str = "perm"        # perm | none (order = NULL) | repeat (row ids drawn with repetition)
    scale: bool = True         # False: scale = NULL
    tiers: str = "ab"

    def __str__(self):
        return self.name


def seg_problem(c, seed, kind):
    """kind "int": inputs, extra and prev integers in [-4, 4], scales in {0.25, 0.5, 1, 2}; "rand": random data, scale = 1 / len."""
    gen = torch.Generator().manual_seed(seed)
    lens = torch.tensor(c.lens)
    nseg, total = len(c.lens), int(lens.sum())
    P = NS(case=c, kind=kind, nseg=nseg, total=total, lens=lens)
    P.ptr = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    P.seg_of_q = torch.repeat_interleave(torch.arange(nseg), lens)
    P.rows = max(total, 1)     # rows of the input; "repeat" draws its ids among them with repetition
    P.order = {"perm": lambda: torch.randperm(total, generator=gen), "none": lambda: None,
               "repeat": lambda: torch.randint(0, P.rows, (total,), generator=gen)}[c.order]()
    nb = 1 if c.shared else c.batch
    P.in_bstride = 0 if c.shared else P.rows * c.width + c.pad
    shape_in, shape_out = (nb, P.rows, c.width), (c.batch, nseg, c.width)
    if kind == "int":
        ri = lambda shape: torch.randint(-4, 5, shape, generator=gen).double()
        P.inp, P.extra, P.prev = ri(shape_in), ri(shape_out), ri(shape_out)
        P.scale = 2.0 ** torch.randint(-2, 2, (nseg,), generator=gen).double()
    else:
        cs = 2.0 ** torch.randint(-3, 4, (c.width,), generator=gen).double()
        rn = lambda shape: (torch.randn(shape, generator=gen, dtype=torch.float64) * cs).float().double()
        P.inp, P.extra, P.prev = rn(shape_in), rn(shape_out), rn(shape_out)
        if c.entry == "bf16":
            P.inp = to_bf16(P.inp)   # the input values are bf16 by construction
        P.scale = (1.0 / lens.clamp(min=1).float()).double()   # the mean, as the fp32 values the kernel reads
    if not c.scale:
        P.scale = None
    return P


SEG_DEFECTS = ("tail_row_past_the_end_added", "lane_group_partial_left_out", "scale_applied_to_extra", "acc_overwrites",
               "order_ignored", "empty_segment_unwritten")


def segsum_math(P, dt=torch.float64, defect=None):
    """-> ({"out": R}, {"out": bound}): R = scale[s] * sum_q in[b, order[q]] (+ extra) (+ prev); bound = U (len_s + 4) |scale_s|
    sum |in| + U (|extra| + |prev| + |R|).  float32: the stand-in."""
    c = P.case
    f = lambda t: t.to(dt)
    order = P.order if (P.order is not None and defect != "order_ignored") else torch.arange(P.total)
    seg = P.seg_of_q
    if defect == "tail_row_past_the_end_added":   # the clamped duplicate of a tail's last row, for segments that end in a partial batch
        last = P.ptr[1:] - 1
        dup = (P.lens % 8 != 0).nonzero()[:, 0]
        order, seg = torch.cat([order, order[last[dup]]]), torch.cat([seg, dup])
    if defect == "lane_group_partial_left_out":   # lane group 1 of max(groups, 2): rows lo + 1, lo + 1 + S, ...
        S = max(c.groups, 2)
        keep = (torch.arange(P.total) - P.ptr[:-1][P.seg_of_q]) % S != 1
        order, seg = order[keep], seg[keep]
    X = f(P.inp).expand(c.batch, -1, -1)[:, order]
    zeros = lambda: torch.zeros((c.batch, P.nseg, c.width), dtype=dt)
    S_ = zeros().index_add_(1, seg, X)
    sc = f(P.scale)[None, :, None] if P.scale is not None else torch.ones((1, 1, 1), dtype=dt)
    R = S_ * sc
    terms = []
    if c.entry == "add":
        R = (S_ + f(P.extra)) * sc if defect == "scale_applied_to_extra" else R + f(P.extra)
        terms.append(P.extra.abs())
    if c.entry in ("acc", "add"):
        if defect != "acc_overwrites":
            R = R + f(P.prev)
        terms.append(P.prev.abs())
    if defect == "empty_segment_unwritten":
        R = R.clone()
        R[:, P.lens == 0] = f(P.prev)[:, P.lens == 0] if c.entry in ("acc", "add") else float("nan")
    if dt != torch.float64:
        return {"out": R}, None
    bound = U * (P.lens.double()[None, :, None] + 4) * sc.abs() * zeros().index_add_(1, seg, X.abs()) + U * (sum(terms) + R.abs())
    return {"out": R}, {"out": bound}


def seg_standin(c, kind, defect=None):
    P = seg_problem(c, 13, kind)
    ref, bud = segsum_math(P)
    got, _ = segsum_math(P, torch.float32, defect)
    return compare_exact(got, ref, ["out"]) if kind == "int" else compare_bounded(got, ref, bud)


def bf16_bits(t):
    """float64 values that are bf16 values -> the uint16 rows (as int16 storage), with the round trip asserted."""
    bits = (t.float().contiguous().view(torch.int32) >> 16).to(torch.int16)
    back = (bits.to(torch.int32) << 16).view(torch.float32).double()
    assert torch.equal(back, t), "the values must be exact bf16 values"
    return bits


@dataclass(frozen=True)
class CombCase:
    name: str
    width: int
    pieces: tuple              # pieces per destination row
    batch: int = 2
    in_place: bool = False     # every dst row is also its first src piece

    def __str__(self):
        return self.name


def comb_problem(c, seed, kind):
    gen = torch.Generator().manual_seed(seed)
    n, npieces = len(c.pieces), sum(c.pieces)
    nrows = n + npieces + 2
    P = NS(case=c, n=n, nrows=nrows, bstride=nrows * c.width + 8)
    P.ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(c.pieces).cumsum(0)])
    P.src = n + torch.randperm(npieces + 2, generator=gen)[:npieces]      # the pieces: rows behind the real ones, in no order
    P.dst = torch.randperm(n, generator=gen)
    if c.in_place:
        P.dst = P.src[P.ptr[:-1]].clone()
    shape = (c.batch, nrows, c.width)
    if kind == "int":
        P.buf = torch.randint(-4, 5, shape, generator=gen).double()
    else:
        cs = 2.0 ** torch.randint(-3, 4, (c.width,), generator=gen).double()
        P.buf = (torch.randn(shape, generator=gen, dtype=torch.float64) * cs).float().double()
    return P


def combine_math(P, dt=torch.float64, defect=None):
    """nlam_split_combine: buf[b, dst[s]] = sum of buf[b, src[q]], q in [ptr[s], ptr[s + 1]), pieces in list order; every other
    row unchanged.  bound = U (pieces + 1) sum |piece| on the dst rows, 0 elsewhere."""
    buf = P.buf.to(dt)
    out, bound = buf.clone(), torch.zeros_like(buf)
    for s in range(P.n):
        q = P.src[int(P.ptr[s]): int(P.ptr[s + 1])]
        if defect == "last_piece_left_out":
            q = q[:-1]
        acc = torch.zeros_like(buf[:, 0])
        for r in q:
            acc = acc + buf[:, r]
        out[:, P.dst[s]] = acc
        bound[:, P.dst[s]] = U * (len(q) + 1) * buf[:, q].abs().sum(1)
    return {"buf": out}, ({"buf": bound} if dt == torch.float64 else None)
