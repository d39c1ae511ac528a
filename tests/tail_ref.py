"""Shared machinery of test_tail_sweep_kernels.py: the float64 restatement of the loss, step-tail, extended step-tail and
evaluation passes (include/nlam_hip.h) with a first-order error budget carried beside every value, the launch geometry of the
kernels (which block, thread and sweep an element falls into), the reduction budgets, fp32 stand-ins with injected defects,
and NaN-guarded device buffers.  U, GUARD are those of mlp_kernel_ref.py; EPS32, NORMAL_ULPS and SLACK those of
test_efm_training.py.  A plain module; nothing here is collected by pytest.

The budget.  ``V`` holds a value and a bound on the absolute error the fp32 evaluation of the same expression can have.  Every
fp32 operation that rounds adds one u = 2^-24 of its result; errors of the operands travel through the derivative of the
operation.  Exact operations (negation, |x|, a product with a power of two, a selection) add nothing.  A fused multiply-add
rounds once where the budget counts twice: contraction never leaves the budget.  The library functions take the accuracy the
project already relies on for logf (test_ensemble_forecast.NORMAL_ULPS: the ULP table of the OpenCL C specification, which the
ROCm device library is built to): log 3 ulp, exp 3, expm1 3, log1p 2, erf 16, an ulp at most EPS32 of the value; division is
correctly rounded (hipcc's default).  The constants the kernels hold in fp32 (pi^-1/2, ...) are one rounding away from the
float64 ones.  Second-order terms: SLACK."""
import ctypes as C
import math

import numpy as np
import torch

from mlp_kernel_ref import GUARD, U
from test_efm_training import EPS32, NORMAL_ULPS, SLACK

from neural_lam_amd import _lib as L

KINDS = ["mse", "mae", "wmse", "wmae", "nll", "crps_gauss"]
TERMS = ["inv_var"] + KINDS
LOG_ULPS = 2.0 * (NORMAL_ULPS - 0.5 - 4.0 - 0.5)   # the logf term of NORMAL_ULPS (3 / 2 behind the square root): 3 ulp
EXP_ULPS, EXPM1_ULPS, LOG1P_ULPS, ERF_ULPS = 3.0, 3.0, 2.0, 16.0   # the same table
assert LOG_ULPS == 3.0

# the clamps of the extended tail as the kernels (and torch on fp32 tensors) hold them
SIG_LOW, SIG_HIGH = float(np.float32(1e-6)), float(np.float32(1.0 - 1e-6))
ISP_LOW = float(torch.log(torch.tensor(1e-6 + 1)))   # log(float32(1 + 1e-6)) evaluated in fp32
SP_THRESHOLD = 20.0


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------------
# values with an error budget
# ---------------------------------------------------------------------------------------------------------------------------
def _a(x):
    return x.double().abs()


class V:
    """v: the value in the working dtype (float64: the reference; float32: the stand-in, every operation rounded by torch);
    e: float64 bound on |fp32 evaluation - exact| of v (meaningful beside a float64 v)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros(v.shape, dtype=torch.float64) if e is None else e

    def _rounded(self):
        return V(self.v, self.e + U * _a(self.v))

    def __add__(self, o):
        return V(self.v + o.v, self.e + o.e)._rounded()

    def __sub__(self, o):
        return V(self.v - o.v, self.e + o.e)._rounded()

    def __mul__(self, o):
        return V(self.v * o.v, _a(self.v) * o.e + _a(o.v) * self.e)._rounded()

    def __truediv__(self, o):
        q = self.v / o.v
        return V(q, (self.e + _a(q) * o.e) / _a(o.v))._rounded()

    def __neg__(self):
        return V(-self.v, self.e)

    def abs(self):
        return V(self.v.abs(), self.e)

    def pow2(self, k):
        """the product with a power of two: exact"""
        return V(self.v * k, self.e * abs(k))

    def fn(self, f, df, ulps):
        v = f(self.v)
        return V(v, _a(df(self.v.double())) * self.e + ulps * EPS32 * _a(v))

    def log(self):
        return self.fn(torch.log, lambda x: 1.0 / x, LOG_ULPS)

    def exp(self):
        return self.fn(torch.exp, torch.exp, EXP_ULPS)

    def expm1(self):
        return self.fn(torch.expm1, torch.exp, EXPM1_ULPS)

    def log1p(self):
        return self.fn(torch.log1p, lambda x: 1.0 / (1.0 + x), LOG1P_ULPS)

    def erf(self):
        return self.fn(torch.erf, lambda x: 2.0 / math.sqrt(math.pi) * torch.exp(-x * x), ERF_ULPS)

    def __getitem__(self, idx):
        return V(self.v[idx], self.e.expand(self.v.shape)[idx])


def exact(c, dt):
    """a constant both precisions hold exactly"""
    return V(torch.tensor(c, dtype=dt))


def const(c, dt):
    """a constant the kernel holds rounded to fp32"""
    return V(torch.tensor(c, dtype=dt), torch.tensor(U * abs(c), dtype=torch.float64))


def where(cond, a, b):
    shape = torch.broadcast_shapes(cond.shape, a.v.shape, b.v.shape)
    return V(torch.where(cond, a.v, b.v), torch.where(cond, a.e.expand(a.v.shape).expand(shape), b.e.expand(b.v.shape).expand(shape)))


def stack(cols):
    shape = cols[0].v.shape
    return V(torch.stack([c.v for c in cols], dim=-1), torch.stack([c.e.expand(shape) for c in cols], dim=-1))


class Branches:
    """The branch points an evaluation passed, each with its distance from the point and the error budget of the compared value:
    fp32 and float64 take the same side where the distance exceeds the budget."""

    def __init__(self):
        self.items = []

    def add(self, name, value, point):
        self.items.append((name, _a(value.v - point), value.e.expand(value.v.shape)))

    def assert_margins(self, what="", factor=4.0, allow_zero=()):
        for name, dist, err in self.items:
            ok = dist > factor * err + 1e-300
            if name in allow_zero:   # exact ties: a zero that both precisions compute exactly
                ok = ok | (dist == 0)
            assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements within {factor} budgets of the branch point {name}"


# ---------------------------------------------------------------------------------------------------------------------------
# the loss kinds (csrc/nlam_hip.hip: loss_consts, loss_entry, loss_dpred, loss_dstd, in their order of operations)
# ---------------------------------------------------------------------------------------------------------------------------
def _cdf(z):
    dt = z.v.dtype
    return (exact(1.0, dt) + (z * const(math.sqrt(0.5), dt)).erf()).pow2(0.5)


def _two_pdf_minus(z):
    """2 phi(z) - pi^-1/2"""
    dt = z.v.dtype
    return const(1.0 / math.sqrt(2.0 * math.pi), dt).pow2(2.0) * (z.pow2(-0.5) * z).exp() - const(1.0 / math.sqrt(math.pi), dt)


def loss_consts(kind, s):
    dt = s.v.dtype
    one = exact(1.0, dt)
    c0 = c1 = exact(0.0, dt)
    if kind in ("wmse", "nll"):
        c0 = one / (s * s)
    if kind in ("wmae", "crps_gauss"):
        c0 = one / s
    if kind == "nll":
        c1 = s.log() + const(0.5 * math.log(2.0 * math.pi), dt)
    if kind == "crps_gauss":
        c1 = s
    return c0, c1


def loss_entry(kind, d, c0, c1):
    if kind == "mse":
        return d * d
    if kind == "mae":
        return d.abs()
    if kind == "wmse":
        return d * d * c0
    if kind == "wmae":
        return d.abs() * c0
    if kind == "nll":
        return d.pow2(0.5) * d * c0 + c1
    z = (-d) * c0
    one = exact(1.0, d.v.dtype)
    return c1 * (z * (_cdf(z).pow2(2.0) - one) + _two_pdf_minus(z))


def _sign0(d):
    return V(torch.sign(d.v))


def loss_dpred(kind, d, c0, br=None):
    if kind in ("mae", "wmae") and br is not None:
        br.add("|d| = 0", d, 0.0)
    if kind == "mse":
        return d.pow2(2.0)
    if kind == "mae":
        return _sign0(d)
    if kind == "wmse":
        return d.pow2(2.0) * c0
    if kind == "wmae":
        return _sign0(d) * c0
    if kind == "nll":
        return d * c0
    return exact(1.0, d.v.dtype) - _cdf((-d) * c0).pow2(2.0)


def loss_dstd(kind, d, s):
    dt = d.v.dtype
    r = exact(1.0, dt) / s
    if kind == "wmse":
        return d.pow2(-2.0) * d * r * r * r
    if kind == "wmae":
        return (-d.abs()) * r * r
    if kind == "nll":
        return r - d * d * r * r * r
    if kind == "crps_gauss":
        return _two_pdf_minus((-d) * r)
    return exact(0.0, dt) * d


def entry64(kind, d, s):
    """the entry of include/nlam_hip.h as plain float64 torch (autograd reference)"""
    if kind == "mse":
        return d**2
    if kind == "mae":
        return d.abs()
    if kind in ("wmse", "inv_var"):
        return d**2 / s**2
    if kind == "wmae":
        return d.abs() / s
    if kind == "nll":
        return 0.5 * d**2 / s**2 + torch.log(s) + 0.5 * math.log(2.0 * math.pi)
    z = -d / s
    cdf = 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return s * (z * (2.0 * cdf - 1.0) + 2.0 * pdf - 1.0 / math.sqrt(math.pi))


# ---------------------------------------------------------------------------------------------------------------------------
# nlam_loss_fwd / _bwd
# ---------------------------------------------------------------------------------------------------------------------------
def loss_math(d, kind, per_entry, scale, gscalar, dt=torch.float64, idx=None, br=None):
    """-> {"terms": w * entry per element (0 on rows of weight 0), "dpred", "dstd" (per-entry std)} as V.  idx = (f, n) index
    tensors per element (the stand-in's defects move them); default: the true ones."""
    B, N, F = d["pred"].shape
    f_i, n_i = idx if idx is not None else true_index(B, N, F)
    pv, tg = V(d["pred"].to(dt)), V(d["target"].to(dt))
    w = V(d["row_weight"].to(dt)[n_i])
    s = V(d["std"].to(dt)) if per_entry else V(d["var_std"].to(dt)[f_i])
    c0, c1 = loss_consts(kind, s)
    dd = pv - tg
    zero = exact(0.0, dt)
    on = w.v != 0
    out = {"terms": where(on, w * loss_entry(kind, dd, c0, c1), zero)}
    g = exact(f32(scale), dt) * exact(f32(gscalar), dt)
    out["dpred"] = where(on, g * w * loss_dpred(kind, dd, c0, br), zero)
    if per_entry:
        out["dstd"] = where(on, g * w * loss_dstd(kind, dd, s), zero)
    return out


def loss_autograd(d, kind, per_entry, scale, gscalar):
    t = {k: v.double() for k, v in d.items() if isinstance(v, torch.Tensor)}
    pred = t["pred"].clone().requires_grad_()
    std = t["std"].clone().requires_grad_() if per_entry else None
    s = std if per_entry else t["var_std"]
    terms = t["row_weight"][:, None] * entry64(kind, pred - t["target"], s)
    total = f32(gscalar) * f32(scale) * terms.sum()
    grads = torch.autograd.grad(total, (pred, std) if per_entry and kind not in ("mse", "mae") else (pred,))
    out = {"terms": terms.detach(), "dpred": grads[0]}
    if per_entry:
        out["dstd"] = grads[1] if len(grads) > 1 else torch.zeros_like(pred)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# nlam_step_tail_fwd / _bwd (term "inv_var") and nlam_step_tail_loss_fwd / _bwd (the six kinds)
# ---------------------------------------------------------------------------------------------------------------------------
def true_index(B, N, F):
    e = torch.arange(B * N * F)
    return (e % F).view(B, N, F), ((e // F) % N).view(B, N, F)


def tail_math(d, term, affine, with_gpred, scale, gloss, dt=torch.float64, idx=None, br=None):
    """The plain step tail: {"pred", "terms", "d_delta", "d_prev"} as V.  d holds fp32 inputs: delta, prev, truth, target,
    g_pred (B, N, F); bmask, row_weight (N); dstd, dmean, var_std, inv_var (F)."""
    B, N, F = d["delta"].shape
    f_i, n_i = idx if idx is not None else true_index(B, N, F)
    t = {k: v.to(dt) for k, v in d.items() if isinstance(v, torch.Tensor)}
    var = lambda k: V(t[k][f_i])  # noqa: E731
    bm, w = t["bmask"][n_i], V(t["row_weight"][n_i])
    assert bool(((bm == 0) | (bm == 1)).all())
    zero = exact(0.0, dt)
    nw = V(t["prev"]) + (V(t["delta"]) * var("dstd") if affine else V(t["delta"]))
    if affine:
        nw = nw + var("dmean")
    pred = where(bm == 1, V(t["truth"]), nw)   # bmask is 0 or 1: both products and the sum are exact
    dd = pred - V(t["target"])
    on = w.v != 0
    if term == "inv_var":
        iv = var("inv_var")
        terms = w * iv * dd * dd
        g = exact(2.0 * f32(scale), dt) * exact(f32(gloss), dt)
        gp = g * w * iv * dd
    else:
        reads = term not in ("mse", "mae")
        c0, c1 = loss_consts(term, var("var_std")) if reads else (zero, zero)
        terms = w * loss_entry(term, dd, c0, c1)
        g = exact(f32(scale), dt) * exact(f32(gloss), dt)
        gp = g * w * loss_dpred(term, dd, c0, br)
    gin = V(t["g_pred"]) if with_gpred else zero
    G = where(on, (gin + gp) if with_gpred else gp, gin)
    G = where(bm == 1, zero, G)   # times (1 - bmask): exact
    return {"pred": pred, "terms": where(on, terms, zero), "d_prev": G, "d_delta": G * var("dstd") if affine else G}


def tail_autograd(d, term, affine, with_gpred, scale, gloss):
    t = {k: v.double() for k, v in d.items() if isinstance(v, torch.Tensor)}
    delta, prev = t["delta"].clone().requires_grad_(), t["prev"].clone().requires_grad_()
    new = prev + (delta * t["dstd"] + t["dmean"] if affine else delta)
    bm = t["bmask"][:, None]
    pred = bm * t["truth"] + (1 - bm) * new
    if term == "inv_var":
        ent = t["inv_var"] * (pred - t["target"]) ** 2
    else:
        ent = entry64(term, pred - t["target"], t["var_std"])
    terms = t["row_weight"][:, None] * ent
    total = f32(gloss) * f32(scale) * terms.sum() + ((pred * t["g_pred"]).sum() if with_gpred else 0.0)
    d_delta, d_prev = torch.autograd.grad(total, (delta, prev))
    return {"pred": pred.detach(), "terms": terms.detach(), "d_delta": d_delta, "d_prev": d_prev}


# ---------------------------------------------------------------------------------------------------------------------------
# nlam_step_tail_ext_fwd / _bwd
# ---------------------------------------------------------------------------------------------------------------------------
def _softplus(q, br, name):
    br.add(name, q, SP_THRESHOLD)
    above = q.v > SP_THRESHOLD
    dt = q.v.dtype
    one = exact(1.0, dt)
    qs = V(torch.clamp(q.v, max=SP_THRESHOLD + 1.0), q.e)   # the branch not taken stays finite in fp32
    return where(above, q, qs.exp().log1p()), where(above, one, one / (one + (-qs).exp()))


def _clamped_new(mode, pv, r, lo, hi, br):
    """clamped_new of one variable's column -> (new, d new / d r, d new / d prev)"""
    dt = pv.v.dtype
    one, zero = exact(1.0, dt), exact(0.0, dt)
    if mode == L.CLAMP_NONE:
        return pv + r, one, one
    if mode == L.CLAMP_BOTH:
        span = hi - lo
        x = (pv - lo) / span
        br.add("sigmoid clamp low", x, SIG_LOW)
        br.add("sigmoid clamp high", x, SIG_HIGH)
        inside = (x.v >= SIG_LOW) & (x.v <= SIG_HIGH)
        u = where(x.v < SIG_LOW, exact(SIG_LOW, dt), where(x.v > SIG_HIGH, exact(SIG_HIGH, dt), x))
        omu = one - u
        s = one / (one + (-((u / omu).log() + r)).exp())
        k = s * (one - s)
        return lo + span * s, span * k, where(inside, k / (u * omu), zero)
    lower = mode == L.CLAMP_LOWER
    y = pv - lo if lower else hi - pv
    br.add("inverse_softplus clamp", y, ISP_LOW)
    br.add("inverse_softplus threshold", y, SP_THRESHOLD)
    above, inrange = y.v > SP_THRESHOLD, y.v >= ISP_LOW
    yc = where(y.v < ISP_LOW, exact(ISP_LOW, dt), where(above, exact(SP_THRESHOLD, dt), y))
    em = yc.expm1()
    dy = where(above, one, where(inrange, (em + one) / em, zero))
    inv = where(above, y, em.log())
    q = inv + r if lower else inv - r
    sp, dr = _softplus(q, br, "softplus threshold (state)")
    return (lo + sp if lower else hi - sp), dr, dr * dy


def ext_math(d, kind, has_std, with_g, with_loss, scale, gloss, dt=torch.float64, br=None):
    """The extended tail: {"pred", "pred_std", "terms", "d_delta_mean", "d_delta_std", "d_prev"} as V.  d: prev, truth, target,
    g_pred, g_std (B, N, F), delta2 (B, N, 2 F: the mean half is the delta without a std head), dstd, dmean, var_std, lo, hi (F),
    bmask, row_weight (N), modes (list)."""
    br = br if br is not None else Branches()
    B, N, F = d["prev"].shape
    t = {k: v.to(dt) for k, v in d.items() if isinstance(v, torch.Tensor)}
    bm = t["bmask"][None, :].expand(B, N)
    w = V(t["row_weight"][:, None].expand(N, F).contiguous())
    zero = exact(0.0, dt)
    news, drs, dps = [], [], []
    for f, m in enumerate(d["modes"]):
        col = lambda k: V(t[k][f])  # noqa: E731
        r = V(t["delta2"][..., f]) * col("dstd") + col("dmean")
        nw, dr, dp = _clamped_new(m, V(t["prev"][..., f]), r, col("lo"), col("hi"), br)
        shape = (B, N)
        news.append(nw)
        drs.append(V(dr.v.expand(shape), dr.e.expand(shape)))
        dps.append(V(dp.v.expand(shape), dp.e.expand(shape)))
    new, dr, dp = stack(news), stack(drs), stack(dps)
    pred = where((bm == 1)[..., None], V(t["truth"]), new)
    out = {"pred": pred}
    sd = gsd = None
    if has_std:
        raw = V(t["delta2"][..., F:])
        sd, gsd = _softplus(raw, br, "softplus threshold (std)")
        out["pred_std"] = sd
    G = V(t["g_pred"]) if with_g else zero
    gs = V(t["g_std"]) if (with_g and has_std) else zero
    if with_loss:
        dd = pred - V(t["target"])
        on = w.v != 0
        reads = kind not in ("mse", "mae")
        s = sd if has_std else V(t["var_std"])
        c0, c1 = loss_consts(kind, s) if (reads or has_std) else (zero, zero)
        out["terms"] = where(on, w * loss_entry(kind, dd, c0, c1), zero)
        g = exact(f32(scale), dt) * exact(f32(gloss), dt)
        gp = g * w * loss_dpred(kind, dd, c0, br)
        G = where(on, (G + gp) if with_g else gp, G)
        if has_std:
            gq = g * w * loss_dstd(kind, dd, sd)
            gs = where(on, (gs + gq) if with_g else gq, gs)
    G = where((bm == 1)[..., None], zero, G)   # times (1 - bmask): exact
    out["d_prev"] = G * dp
    out["d_delta_mean"] = G * dr * V(t["dstd"])
    if has_std:
        out["d_delta_std"] = gs * gsd
    return out


def _isp64(y):
    yc = torch.clamp(y, min=ISP_LOW, max=SP_THRESHOLD)
    return torch.where(y <= SP_THRESHOLD, torch.log(torch.expm1(yc)), y)


def ext_autograd(d, kind, has_std, with_g, with_loss, scale, gloss):
    """The reference's formulation (get_clamped_new_state, softplus, the boundary overwrite, the entry on the interior weights)
    with torch ops in float64; the clamps at the fp32 values torch applies to fp32 tensors; gradients by autograd."""
    sp = torch.nn.functional.softplus
    t = {k: v.double() for k, v in d.items() if isinstance(v, torch.Tensor)}
    F = t["prev"].shape[-1]
    delta = t["delta2"].clone().requires_grad_()
    prev = t["prev"].clone().requires_grad_()
    r = delta[..., :F] * t["dstd"] + t["dmean"]
    cols = []
    for f, m in enumerate(d["modes"]):
        p, rf, lo, hi = prev[..., f], r[..., f], t["lo"][f], t["hi"][f]
        if m == L.CLAMP_NONE:
            cols.append(p + rf)
        elif m == L.CLAMP_BOTH:
            u = torch.clamp((p - lo) / (hi - lo), min=SIG_LOW, max=SIG_HIGH)
            cols.append(lo + (hi - lo) * torch.sigmoid(torch.log(u / (1 - u)) + rf))
        elif m == L.CLAMP_LOWER:
            cols.append(lo + sp(_isp64(p - lo) + rf))
        else:
            cols.append(hi - sp(_isp64(hi - p) - rf))
    new = torch.stack(cols, dim=-1)
    bm = t["bmask"][:, None]
    pred = bm * t["truth"] + (1 - bm) * new
    std = sp(delta[..., F:]) if has_std else None
    total = torch.zeros((), dtype=torch.float64)
    out = {"pred": pred.detach()}
    if with_loss:
        terms = t["row_weight"][:, None] * entry64(kind, pred - t["target"], std if has_std else t["var_std"])
        out["terms"] = terms.detach()
        total = total + f32(gloss) * f32(scale) * terms.sum()
    if with_g:
        total = total + (pred * t["g_pred"]).sum() + ((std * t["g_std"]).sum() if has_std else 0.0)
    d_delta, d_prev = torch.autograd.grad(total, (delta, prev), allow_unused=True)
    d_delta = torch.zeros_like(delta) if d_delta is None else d_delta
    out.update(d_delta_mean=d_delta[..., :F], d_prev=torch.zeros_like(prev) if d_prev is None else d_prev)
    if has_std:
        out.update(pred_std=std.detach(), d_delta_std=d_delta[..., F:])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# launch geometry and reduction budgets
# ---------------------------------------------------------------------------------------------------------------------------
def elementwise_blocks(total, cap):
    return min(cap, (total + 255) // 256)


class Sweep:
    """Where the elements of a grid-stride pass of `nblocks` workgroups of 256 threads fall: `vec` = the 16-byte loop (a
    thread takes quads), else the scalar loop."""

    def __init__(self, total, nblocks, vec):
        assert not vec or total % 4 == 0
        self.total, self.nblocks, self.vec = total, nblocks, vec
        e = torch.arange(total)
        unit = e // 4 if vec else e
        nthr = nblocks * 256
        self.nunits = (total // 4) if vec else total
        self.sweep = unit // nthr                       # the trip of the loop that reaches the element
        self.block = (unit % nthr) // 256
        self.nsweeps = -(-self.nunits // nthr)
        # additions on one output's path: a thread's own elements, the xor tree of a wave, the four waves
        self.per_thread = self.nsweeps * (4 if vec else 1)
        self.depth = self.per_thread + 6 + 2

    def block_units(self):
        return torch.bincount((torch.arange(self.nunits) % (self.nblocks * 256)) // 256, minlength=self.nblocks)


def partials_ref(terms, sw, scale):
    """partials[b] = scale * sum of the block's terms: (R, bound) from the per-element terms (a V, float64)."""
    v, e = terms.v.reshape(-1).double(), terms.e.expand(terms.v.shape).reshape(-1)
    z = torch.zeros(sw.nblocks, dtype=torch.float64)
    s, sa, se = z.clone().index_add_(0, sw.block, v), z.clone().index_add_(0, sw.block, v.abs()), z.clone().index_add_(0, sw.block, e)
    sc = f32(scale)
    return sc * s, abs(sc) * (se + U * (sw.depth + 1) * sa)


def loss_ref(terms, sw, scale):
    """the loss behind nlam_reduce_partials: its waves add (nparts + 3) / 4 partials each, then (0 + 1) + (2 + 3)"""
    v, e = terms.v.reshape(-1).double(), terms.e.expand(terms.v.shape).reshape(-1)
    depth = sw.depth + 1 + (sw.nblocks + 3) // 4 + 2
    sc = f32(scale)
    return sc * v.sum(), abs(sc) * (e.sum() + U * depth * v.abs().sum())


def compare(got, ref, note=None):
    """|got - R| <= SLACK * bound element by element over EVERY element; a NaN (an element no sweep reached) fails.
    ref: name -> (R, bound).  -> the names that fail."""
    bad = []
    for name, (R, bound) in ref.items():
        if name not in got or tuple(got[name].shape) != tuple(R.shape):
            bad.append(name)
            continue
        err = (got[name].double() - R).abs()
        lim = SLACK * bound.expand(R.shape) + 2.0 ** -50 * R.abs() + 1e-300
        if not bool((err <= lim).all()):
            bad.append(name)
        if note is not None:
            r = err / lim
            note(name, float(r[torch.isfinite(r)].max()) if bool(torch.isfinite(r).any()) else float("inf"))
    return bad


def vref(x):
    return x.v.double(), x.e.expand(x.v.shape)


def max_norm_passes(got, R, tol=1e-5):
    """the check the older tests apply: max|a - b| / max|b| <= tol"""
    return float((got.double() - R).abs().max() / R.abs().max()) <= tol


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def boundary_mask(N, g, share=0.3):
    bmask = torch.zeros(N)
    bmask[torch.randperm(N, generator=g)[: max(1, round(share * N))]] = 1.0
    return bmask


def tail_inputs(shape, seed):
    """Seeded fp32 inputs of the plain tail and the loss pass; ~30 % boundary nodes (bmask = 1, row_weight = 0)."""
    B, N, F = shape
    g = torch.Generator().manual_seed(seed)
    d = {k: torch.randn(B, N, F, generator=g) for k in ("delta", "prev", "truth", "target", "g_pred")}
    bmask = boundary_mask(N, g)
    d["bmask"], d["row_weight"] = bmask, (1 - bmask) / (1 - bmask).sum()
    d["dstd"], d["dmean"] = torch.rand(F, generator=g) + 0.5, torch.randn(F, generator=g)
    d["var_std"] = torch.rand(F, generator=g) + 0.5
    d["inv_var"] = 1.0 / d["var_std"] ** 2
    d["pred"] = torch.randn(B, N, F, generator=g)            # the loss pass's own prediction
    d["std"] = torch.rand(B, N, F, generator=g) + 0.5        # and per-entry std
    return d


def ext_inputs(shape, seed):
    """fp32 inputs of the extended tail, built as test_clamped_tail._tail_case builds them (any F, F = 1 included): the clamp
    modes both, lower, upper, none in rotation over the variables; clamped columns inside their limits with a margin, about 1 %
    of the rows outside a limit by >= 0.2, a few rows above the softplus threshold, raw std ~ N(0, 1) with one element at 25,
    ~30 % boundary nodes of weight 0.  The margins are asserted where the reference passes the branch points (Branches)."""
    B, N, F = shape
    g = torch.Generator().manual_seed(seed)
    rows_n = B * N
    modes = [(L.CLAMP_BOTH, L.CLAMP_LOWER, L.CLAMP_UPPER, L.CLAMP_NONE)[f % 4] for f in range(F)]
    lo = torch.tensor([-1.0 + 0.1 * (f % 10) for f in range(F)])
    hi = lo + 3.0
    prev = torch.randn(rows_n, F, generator=g)
    rows = torch.arange(rows_n)
    outside, above = rows % 97 == 3, rows % 89 == 5
    for f, m in enumerate(modes):
        u, a = torch.rand(rows_n, generator=g), torch.randn(rows_n, generator=g).abs()
        if m == L.CLAMP_BOTH:
            col = lo[f] + 0.03 + u * (3.0 - 0.06)
            col[outside] = torch.where(u[outside] < 0.5, lo[f] - 0.2 - u[outside], hi[f] + 0.2 + u[outside])
        elif m == L.CLAMP_LOWER:
            col = lo[f] + 0.03 + 1.5 * a
            col[outside] = lo[f] - 0.2 - u[outside]
            col[above] = lo[f] + 23.0 + u[above]
        elif m == L.CLAMP_UPPER:
            col = hi[f] - 0.03 - 1.5 * a
            col[outside] = hi[f] + 0.2 + u[outside]
            col[above] = hi[f] - 23.0 - u[above]
        else:
            continue
        prev[:, f] = col
    bmask = boundary_mask(N, g)
    bmask[0], bmask[-1] = 0.0, 1.0
    interior = 1.0 - bmask
    d = {"prev": prev.view(B, N, F), "delta2": torch.randn(B, N, 2 * F, generator=g), "truth": torch.randn(B, N, F, generator=g),
         "target": torch.randn(B, N, F, generator=g), "g_pred": torch.randn(B, N, F, generator=g),
         "g_std": torch.randn(B, N, F, generator=g), "dstd": torch.rand(F, generator=g) + 0.5, "dmean": 0.1 * torch.randn(F, generator=g),
         "var_std": torch.rand(F, generator=g) + 0.5, "bmask": bmask, "row_weight": interior / interior.sum(), "lo": lo, "hi": hi}
    d["delta2"][0, 0, 2 * F - 1] = 25.0   # the raw std of one interior element on softplus' linear branch
    d["modes"] = modes
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# nlam_eval_metrics
# ---------------------------------------------------------------------------------------------------------------------------
EVAL_CHUNK_ELEMS = 8192


def eval_chunk_nodes(F):
    return ((EVAL_CHUNK_ELEMS // F + 3) // 4) * 4


def eval_lanes(F):
    return (256 // F) * F


def eval_nchunks(N, F):
    return -(-N // eval_chunk_nodes(F))


def eval_inputs(shape, seed, last_chunk_boundary=False):
    B, T, N, F = shape
    g = torch.Generator().manual_seed(seed)
    # errors of different size per variable, 10^-1.5 .. 10^0.5: a max-norm over the variables sees only the large ones
    mag = 10.0 ** (-1.5 + 2.0 * torch.arange(F) / max(1, F - 1))
    pred = torch.randn(B, T, N, F, generator=g)
    d = {"pred": pred, "target": pred + mag * torch.randn(B, T, N, F, generator=g),
         "std": torch.rand(B, T, N, F, generator=g) + 0.5, "var_std": torch.rand(F, generator=g) + 0.5}
    bmask = boundary_mask(N, g)
    if last_chunk_boundary:
        bmask[(eval_nchunks(N, F) - 1) * eval_chunk_nodes(F):] = 1.0
    d["row_weight"] = (1 - bmask) / (1 - bmask).sum()
    return d


def eval_math(d, kind, per_entry, map_steps, dt=torch.float64, defect=None):
    """step_loss (B, T), sq / ab / std_mean (B, T, F) and maps (B, S, N) of nlam_eval_metrics as name -> (R, bound) in float64,
    or with dt = float32 the stand-in's values (name -> tensor; per-chunk partial sums, then the chunks).
    The additions on one output's path: a lane's strides (x 4 elements for the loss), the wave tree and the four waves (loss) or
    the W / F slots of a variable (sq, ab, std), then ceil(chunks / 4) chunks per wave and (0 + 1) + (2 + 3)."""
    B, T, N, F = d["pred"].shape
    pv, tg = V(d["pred"].to(dt)), V(d["target"].to(dt))
    w = V(d["row_weight"].to(dt)[:, None].expand(N, F).contiguous())
    s = V(d["std"].to(dt)) if per_entry else V(d["var_std"].to(dt))
    c0, c1 = loss_consts(kind, s) if (kind not in ("mse", "mae") or per_entry) else (exact(0.0, dt), exact(0.0, dt))
    dd = pv - tg
    ent = loss_entry(kind, dd, c0, c1)
    on = (w.v != 0).expand(B, T, N, F)
    zero = exact(0.0, dt)
    q = {"loss": where(on, w * ent, zero), "sq": where(on, w * (dd * dd), zero), "ab": where(on, w * dd.abs(), zero)}
    if per_entry:
        q["std_mean"] = where(on, w * s, zero)
    cn, nch = eval_chunk_nodes(F), eval_nchunks(N, F)
    lanes = eval_lanes(F)
    W = 4 * lanes
    strides = -(-min(cn, N) * F // W)
    per = (nch + 3) // 4
    depth = {"loss": 4 * strides + 6 + 2 + per + 2}
    for k in ("sq", "ab", "std_mean"):
        depth[k] = strides + W // F + per + 2
    interior = d["row_weight"] != 0
    if dt == torch.float64:
        out = {}
        for k, x in q.items():
            v, e = x.v.double(), x.e.expand(x.v.shape)
            dims = (2, 3) if k == "loss" else (2,)
            out["step_loss" if k == "loss" else k] = (v.sum(dims), e.sum(dims) + U * depth[k] * v.abs().sum(dims))
        steps = list(map_steps)
        if steps:
            v, e = ent.v.double()[:, steps], ent.e.expand(ent.v.shape)[:, steps]
            R, bound = v.sum(-1), e.sum(-1) + U * F * v.abs().sum(-1)
            R = torch.where(interior, R, torch.full_like(R, float("nan")))
            out["maps"] = (R, bound)
        return out
    # the stand-in: per-chunk sums in fp32, then the chunks; defects as named
    out = {}
    for k, x in q.items():
        name = "step_loss" if k == "loss" else k
        chunks = [x.v[:, :, c * cn: (c + 1) * cn].sum((2, 3) if k == "loss" else 2) for c in range(nch)]
        if defect == "last_chunk_dropped_in_finish":
            chunks = chunks[:-1] if nch > 1 else chunks
        tot = chunks[0]
        for c in chunks[1:]:
            tot = tot + c
        out[name] = tot
    if defect == "sq_column_scaled":
        out["sq"] = out["sq"].clone()
        out["sq"][..., 0] *= 1.0 + 1e-4   # the variable with the smallest errors
    steps = list(map_steps)
    if steps:
        m = ent.v[:, steps].sum(-1)
        m = torch.where(interior, m, torch.full_like(m, float("nan")))
        if defect == "map_rows_of_later_strides_at_stride_0":
            rows = W // F
            wrong = torch.full_like(m, float("nan"))
            n = torch.arange(N)
            src_ok = (n % cn) < rows
            wrong[..., src_ok] = m[..., src_ok]
            # rows of later strides land on stride 0's nodes (the last writer wins); their own nodes are never written
            for c in range(nch):
                lo = c * cn
                hi_ = min(N, lo + cn)
                for it in range(1, -(-(hi_ - lo) // rows)):
                    a, b = lo + it * rows, min(hi_, lo + (it + 1) * rows)
                    wrong[..., lo: lo + (b - a)] = m[..., a:b]
            m = wrong
        out["maps"] = m
    return out


def compare_maps(got, R, bound, note=None):
    """maps: NaN exactly where the reference is NaN (the nodes of weight 0), the bound everywhere else -> failing names"""
    nan_ok = torch.equal(torch.isnan(got), torch.isnan(R))
    fin = ~torch.isnan(R)
    bad = compare({"maps": torch.where(fin, got.double(), torch.zeros((), dtype=torch.float64))},
                  {"maps": (torch.where(fin, R, torch.zeros_like(R)), bound)}, note)
    return bad if nan_ok else ["maps"]


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 stand-ins of the sweeping passes, with defects
# ---------------------------------------------------------------------------------------------------------------------------
TAIL_DEFECTS = ("second_sweep_skipped", "node_not_wrapped_in_later_sweep", "variable_restarts_each_sweep", "partial_of_block_dropped")
EVAL_DEFECTS = ("last_chunk_dropped_in_finish", "map_rows_of_later_strides_at_stride_0", "sq_column_scaled")


def standin_tail(d, term, affine, with_gpred, scale, gloss, sw, defect=None):
    """The plain step tail in torch fp32 on the CPU with the forward's launch geometry `sw`: pred, partials, loss, d_delta,
    d_prev.  Defects change where a later sweep reads its per-node / per-variable operands, or drop work."""
    B, N, F = d["delta"].shape
    f_i, n_i = true_index(B, N, F)
    later = (sw.sweep >= 1).view(B, N, F)
    if defect == "node_not_wrapped_in_later_sweep":   # the node counter runs on past the end of a sample
        e = torch.arange(B * N * F).view(B, N, F)
        n_i = torch.where(later, torch.clamp(e // F, max=N - 1), n_i)
    if defect == "variable_restarts_each_sweep":      # f counted from the start of the sweep, not of the tensor
        e = torch.arange(B * N * F)
        first = sw.sweep * (sw.nblocks * 256 * (4 if sw.vec else 1))
        f_i = ((e - first) % F).view(B, N, F)
    r = tail_math(d, term, affine, with_gpred, scale, gloss, dt=torch.float32, idx=(f_i, n_i))
    out = {k: r[k].v.clone() for k in ("pred", "d_delta", "d_prev")}
    terms = r["terms"].v.reshape(-1).clone()
    if defect == "second_sweep_skipped":
        out["pred"][(sw.sweep == 1).view(B, N, F)] = float("nan")
        terms[sw.sweep == 1] = 0.0
    partials = torch.stack([terms[sw.block == b].sum() for b in range(sw.nblocks)]) * torch.tensor(f32(scale))
    out["partials"] = partials
    out["loss"] = (partials[:1] if defect == "partial_of_block_dropped" else partials).sum()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# GPU side: inputs at a chosen alignment, NaN-filled outputs between NaN guards
# ---------------------------------------------------------------------------------------------------------------------------
def put(t, dev, off=0):
    """t's values on the device, 16-byte aligned (off = 0) or `off` floats past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, device=dev, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    view = buf[off: off + t.numel()].view(t.shape)
    view.copy_(t.to(torch.float32))
    return view


class Out:
    """An output buffer filled with NaN, GUARD NaN floats before and after it."""

    def __init__(self, shape, dev, off=0):
        n = int(np.prod(shape)) if len(shape) else 1
        self.n, self.front, self.shape = n, GUARD + off, tuple(shape)
        self.buf = torch.full((self.front + n + GUARD,), float("nan"), device=dev, dtype=torch.float32)
        self.view = self.buf[self.front: self.front + n]
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == 4 * off

    def ptr(self):
        return self.view.data_ptr()

    def read(self):
        full = self.buf.cpu()
        assert bool(torch.isnan(full[: self.front]).all()) and bool(torch.isnan(full[self.front + self.n:]).all()), "a guard was written"
        return full[self.front: self.front + self.n].view(self.shape)

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
