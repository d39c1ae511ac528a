"""Shared machinery of test_adamw_kernels.py: the hyper-parameter sets, the seeded problem builder, the float64 math of one
AdamW update (torch.optim.AdamW's, which adamw_ctl_one in csrc/nlam_hip.hip states in fp32) with its first-order error budget
per output, the fp32 stand-in for the kernel (adamw_ctl_one operation by operation, with injected defects), the float64 bias
corrections with the unit their error is measured in, and the NaN-guarded device buffers.  U, GUARD and compare_bounded are
those of mlp_kernel_ref.py; no constant is refitted here.  A plain module; nothing here is collected by pytest."""
import math
from dataclasses import dataclass
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np
import torch

from mlp_kernel_ref import GUARD, U, compare_bounded  # noqa: F401

F32_MIN, F32_MAX = 2.0 ** -126, float(np.finfo(np.float32).max)
WORK_ITEM_CAP = 256 * 8 * 256      # the launch cap of the update kernels: 256 * 8 workgroups of 256 (one element or one quad each)


def f32(x):
    """The fp32 value a C float argument holds, as a Python float."""
    return float(np.float32(x))


@dataclass(frozen=True)
class HP:
    name: str
    lr: float
    b1: float
    b2: float
    eps: float
    wd: float
    grad_scale: float
    clip: bool                 # a clip coefficient below 1 (a max_grad_norm below the gradient's norm), on the controlled paths
    t: int                     # the update the first call applies (the resident step count is written to t - 1 before it)

    def __str__(self):
        return self.name

    def rounded(self):
        """The hyper-parameters at the fp32 values the kernels receive."""
        return NS(lr=f32(self.lr), b1=f32(self.b1), b2=f32(self.b2), eps=f32(self.eps), wd=f32(self.wd), gs=f32(self.grad_scale))


HPARAMS = (
    HP("default_t1", 1e-3, 0.9, 0.95, 1e-8, 1e-2, 1.0, False, 1),
    HP("scaled_t3", 1e-3, 0.9, 0.95, 1e-8, 1e-2, 0.5, False, 3),
    HP("strong_clipped_t2", 0.1, 0.8, 0.999, 1e-3, 0.1, 1.0 / 3.0, True, 2),
    HP("no_momentum_clipped_t7", 1e-2, 0.0, 0.5, 1e-8, 0.0, 1.0, True, 7),
    HP("late_t1000", 3e-4, 0.9, 0.999, 1e-6, 0.3, 1.0 / 3.0, False, 1000),
)
BETA_PAIRS = tuple((h.b1, h.b2) for h in HPARAMS[1:])   # the four distinct pairs of the sets


def fma32(a, b, c):
    """fmaf(a, b, c) on fp32 values: the exact a b + c rounded to fp32 once (through exact rationals, not through float64)."""
    x = Fraction(a) * Fraction(b) + Fraction(c)
    r = np.float32(float(x))
    near = (r, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf)))
    return float(min(near, key=lambda q: abs(Fraction(float(q)) - x)))


# ---------------------------------------------------------------------------------------------------------------------------
# the bias corrections: float64 from the fp32-rounded betas, and the unit their error is measured in
# ---------------------------------------------------------------------------------------------------------------------------
def bias_corr64(b1, b2, t):
    """(1 - b1^t, sqrt(1 - b2^t)) in float64 from the fp32-rounded betas."""
    return 1.0 - f32(b1) ** t, math.sqrt(1.0 - f32(b2) ** t)


def bias_corr_ratios(got, b1, b2, t):
    """|got - R| of bias_corr[0] and bias_corr[1] in units of what ONE u = 2^-24 of absolute error in powf's value (at most 1,
    so u is half an ulp of its top binade) becomes behind it, plus one rounding of every later operation:
      1 - x:        u + u R                          (powf's u, the subtraction)
      sqrt(1 - x):  u (1 + R^2) / (2 R) + u R        (the above through the root: d sqrt(y) = dy / (2 sqrt(y)); sqrtf)
    The measured multiple of this unit is what nobody knew about powf on the device (test_bias_corrections...)."""
    r1, r2 = bias_corr64(b1, b2, t)
    unit1 = U * (1.0 + r1)
    unit2 = U * ((1.0 + r2 * r2) / (2.0 * r2) + r2)
    return abs(float(got[0]) - r1) / unit1, abs(float(got[1]) - r2) / unit2


# ---------------------------------------------------------------------------------------------------------------------------
# one update: float64 reference with its budget, fp32 stand-in with defects
# ---------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("l2_decay_in_gradient", "decay_after_update", "decay_without_lr", "eps_before_bc2_division", "eps_inside_sqrt", "no_bc2",
           "no_bc1", "update_from_old_m", "v_from_unscaled_gradient", "v_from_unclipped_gradient")


def _update(p, g, m, v, hp, bc1, bc2_sqrt, lr_t, coef, dt, defect=None, inter=None):
    """adamw_ctl_one's expressions in its order on tensors of dtype dt.  float32: every product, sum, quotient and root is rounded
    on its own, `decay` is the one fma.  -> (p', m', v', A, denom, step)"""
    h = hp.rounded()
    s = lambda x: torch.tensor(x, dtype=dt)
    lr, b1, b2, eps, wd, gs, cf, c1, c2 = (s(x) for x in (lr_t, h.b1, h.b2, h.eps, h.wd, h.gs, coef, bc1, bc2_sqrt))
    one = s(1.0)
    p, g, m, v = (x.to(dt) for x in (p, g, m, v))
    decay = s(fma32(-float(lr_t), h.wd, 1.0)) if dt == torch.float32 else one - lr * wd
    if defect == "decay_without_lr":
        decay = one - wd
    if defect in ("l2_decay_in_gradient", "decay_after_update"):
        decay_late, decay = decay, one
    if defect == "no_bc1":
        c1 = one
    if defect == "no_bc2":
        c2 = one
    step = lr / c1
    gsc = g * gs
    gm = gsc * cf
    if defect == "l2_decay_in_gradient":
        gm = gm + wd * p
    gv = {"v_from_unscaled_gradient": g * cf, "v_from_unclipped_gradient": gsc}.get(defect, gm)
    pd = p * decay
    t1, om1 = b1 * m, one - b1
    t2 = om1 * gm
    mi = t1 + t2
    w1, om2 = b2 * v, one - b2
    w2 = om2 * gv
    w3 = w2 * gv
    vi = w1 + w3
    if defect == "eps_inside_sqrt":
        root = torch.sqrt(vi + eps)
        quot = root / c2
        denom = quot
    elif defect == "eps_before_bc2_division":
        root = torch.sqrt(vi)
        quot = root + eps
        denom = quot / c2
    else:
        root = torch.sqrt(vi)
        quot = root / c2
        denom = quot + eps
    ratio = (m if defect == "update_from_old_m" else mi) / denom
    upd = step * ratio
    out = pd - upd
    if defect == "decay_after_update":
        out = out * decay_late
    if inter is not None:
        inter.extend([gsc, gm, pd, t1, t2, mi, w1, w2, w3, vi, root, quot, denom, ratio, upd, out])
    return out, mi, vi, t1.abs() + t2.abs(), denom, step


def adamw_step64(p, g, m, v, hp, bc1, bc2_sqrt, lr_t, coef, inter=None):
    """One update of torch.optim.AdamW in float64 from fp32 values (float64 tensors in and out; bc1, bc2_sqrt, lr_t and coef as
    read back from the device):
        g' = g grad_scale coef;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
        p' = p (1 - lr_t wd) - (lr_t / bc1) m' / (sqrt(v') / bc2_sqrt + eps)
    -> ({p, m, v}, {p, m, v}): the values and a first-order bound on what adamw_ctl_one's roundings move each of them by.
    inter: a list that receives every float64 intermediate (assert_normal_range)."""
    out, mi, vi, A, denom, step = _update(p, g, m, v, hp, bc1, bc2_sqrt, lr_t, coef, torch.float64, inter=inter)
    # The roundings of adamw_ctl_one, one u = 2^-24 for each fp32 operation (every input is taken at its fp32 value), [k] = the
    # units a factor carries:
    #   g  = (gr * gscale) * coef                                          two products: g = g' [2]
    #   mi = b1 * mo [1] + ((1 - b1) [1] * g [2]) [1], the sum [1]         2 u |b1 m| + 5 u |(1 - b1) g'| <= 5 u A
    #   vi = b2 * vo [1] + (((1 - b2) [1] * g [2]) [1] * g [2]) [1], the sum [1]
    #                                                                      2 u b2 v + 8 u (1 - b2) g'^2 <= 8 u v' (no cancellation)
    #   pv = pv * decay: the fma that makes decay [1], the product [1]; the last subtraction [1] acts on |p'| <= |p decay| + |T|
    #                                                                      3 u |p| + 1 u |T|,  T = step m' / denom
    #   T:  step = lr / bc1 [1], mi / denom [1], step * (..) [1]; denom = sqrtf(vi) [1] / bc2_sqrt [1] + eps [1], each at most
    #       that much of denom (sqrt(v') / bc2_sqrt <= denom); vi's own 8 u halved by the root [4]: 10 u |T| in all, and mi's
    #       own error as it stands (m' can cancel: absolute in A): 5 u A step / denom
    # Counted: m' 5 u A; v' 8 u v'; p' u (3 |p| + step (5 A + 11 |m'|) / denom).  The budgets keep the constants they were given
    # with: 6 and 9 (one u to spare each), and for p' 4 |p| + step (6 A + 14 |m'|) / denom = the count with m' at its budget and
    # one u more for each of sqrtf, the division and the last subtraction (3 + 1 on |p|; 11 + 3 on |m'|): the build has no
    # fast-math, but nothing here leans on those three being correctly rounded.
    bud = {"m": 6.0 * U * A, "v": 9.0 * U * vi, "p": U * (4.0 * p.abs() + step * (6.0 * A + 14.0 * mi.abs()) / denom)}
    return {"p": out, "m": mi, "v": vi}, bud


def adamw_standin32(p, g, m, v, hp, bc1, bc2_sqrt, lr_t, coef, defect=None):
    """The stand-in for a kernel: adamw_ctl_one operation by operation in torch fp32 on the CPU -> {p, m, v} (fp32)."""
    out, mi, vi, *_ = _update(p, g, m, v, hp, bc1, bc2_sqrt, lr_t, coef, torch.float32, defect=defect)
    return {"p": out, "m": mi, "v": vi}


def assert_normal_range(inter, what=""):
    """Every intermediate is an exact zero or a normal fp32 number with room to spare: a float64 reference disagrees with fp32
    about a flushed or overflowed value for no fault of the kernel."""
    for k, x in enumerate(inter):
        a = x.abs()
        nz = a[a != 0]
        assert bool(torch.isfinite(a).all()) and (nz.numel() == 0 or (float(nz.min()) >= 4.0 * F32_MIN and float(nz.max()) <= F32_MAX / 4.0)), \
            f"{what}: intermediate {k} leaves fp32's normal range ({float(nz.min()):.3g} .. {float(nz.max()):.3g})"


# ---------------------------------------------------------------------------------------------------------------------------
# the problem
# ---------------------------------------------------------------------------------------------------------------------------
def host_controls(g, hp, clip):
    """What the control kernel will decide for the gradient g (float64 of fp32 values), in its own expressions on the host:
    -> (max_grad_norm to ask for or None, the coefficient).  The tests read the coefficient actually used back from the device;
    this one places max_grad_norm at 0.37 of the norm and the cancelling moments of adamw_problem."""
    if not clip:
        return None, 1.0
    norm = np.float32(f32(hp.grad_scale) * math.sqrt(float(g.square().sum())))
    max_norm = np.float32(0.37) * norm   # (no power of two: the product with the coefficient rounds)
    assert max_norm > 0
    return float(max_norm), float(min(np.float32(1.0), max_norm / (norm + np.float32(1e-6))))


def host_bias_corr(hp, t):
    return tuple(f32(x) for x in bias_corr64(hp.b1, hp.b2, t))


def adamw_problem(n, seed, t, hp=HPARAMS[0], clip=None):
    """fp32 values as float64 tensors: p = randn 10^U(-3, 1); g = randn 10^U(-10, 4) with every 17th element exactly 0 (the small
    end lets eps dominate the denominator); for t > 1 arbitrary moments, m = randn 10^U(-10, 4) with every 5th element placed so
    that b1 m and (1 - b1) g' cancel to about 2^-18 of their size, v the square of such a value with every 13th element exactly
    0; zero moments at t = 1.  ema: where an average starts.  hp / clip (default: hp.clip) place the cancelling moments and
    max_grad_norm, and the builder asserts in float64 that every intermediate of the update stays in fp32's normal range."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(n, generator=gen, dtype=torch.float64)
    mag = lambda lo, hi: 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64))
    r32 = lambda x: x.float().double()
    clip = hp.clip if clip is None else clip
    h = hp.rounded()
    P = NS(n=n, t=t, hp=hp)
    P.p = r32(rn() * mag(-3, 1))
    P.ema = r32(rn() * mag(-3, 1))
    g = r32(rn() * mag(-10, 4))
    g[16::17] = 0.0
    P.g = g
    P.max_norm, P.coef = host_controls(g, hp, clip)
    m, v = rn() * mag(-10, 4), (rn() * mag(-10, 4)) ** 2
    near = 1.0 + 2.0 ** -18 * (1.0 + torch.rand(n, generator=gen, dtype=torch.float64))
    if t > 1:
        if h.b1 > 0:
            m[4::5] = (-(1.0 - h.b1) * (g * h.gs * P.coef) / h.b1 * near)[4::5]
        v[12::13] = 0.0
        P.m, P.v = r32(m), r32(v)
    else:
        P.m, P.v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    inter = []
    bc1, bc2_sqrt = host_bias_corr(hp, t)
    adamw_step64(P.p, P.g, P.m, P.v, hp, bc1, bc2_sqrt, h.lr, P.coef, inter=inter)
    assert_normal_range(inter, f"adamw_problem({n}, {seed}, {t}, {hp})")
    return P


# ---------------------------------------------------------------------------------------------------------------------------
# GPU side: a buffer with GUARD NaN floats on both sides of the values, optionally one float off a 16-byte boundary
# ---------------------------------------------------------------------------------------------------------------------------
class Guarded:
    def __init__(self, values, off=0):
        self.n, self.front = values.numel(), GUARD + off
        self.buf = torch.full((self.front + self.n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
        self.view = self.buf[self.front: self.front + self.n]
        self.view.copy_(values.float())
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == 4 * off

    def read(self):
        """-> (the values on the host, whether every guard float is still NaN)"""
        full = self.buf.cpu()
        inside = full[self.front: self.front + self.n]
        return inside, bool(torch.isnan(full[: self.front]).all()) and bool(torch.isnan(full[self.front + self.n:]).all())
