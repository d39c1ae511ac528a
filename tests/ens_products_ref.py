"""Reference of nlam_ens_products (include/nlam_hip.h) in float64 torch: exceedance probabilities, linear-interpolation quantile
fields, Brier score, reliability table, pinball loss and the counts of truths below a quantile.  The tables are the kernel's own:
``event_thr`` (standardised), ``q_frac`` and ``q_level`` are the fp32 values the kernel reads, cast to double here."""
import math

import torch


def quantile_tables(levels, members):
    """(index, frac): i = floor(q (M - 1)), g = q (M - 1) - i in float64 (what the engine's host side computes)."""
    pos = [float(q) * (members - 1) for q in levels]
    idx = [min(int(math.floor(v)), members - 1) for v in pos]
    return idx, [v - i for v, i in zip(pos, idx)]


def quantiles(x, q_index, q_frac, dim=1):
    """Q_j = x_(i) + g (x_(min(i + 1, M - 1)) - x_(i)) over ``dim`` of float64 ``x``: the new axis replaces ``dim``."""
    M = x.shape[dim]
    xs = torch.sort(x.double(), dim=dim).values
    out = []
    for i, g in zip(q_index, q_frac):
        i = int(i)
        lo, hi = xs.select(dim, i), xs.select(dim, min(i + 1, M - 1))
        out.append(lo + float(g) * (hi - lo))
    return torch.stack(out, dim=dim)


def ens_products(x, y, w, event_var=(), event_sense=(), event_thr=(), q_index=(), q_frac=(), q_level=(), state_mean=None,
                 state_std=None):
    """The outputs of nlam_ens_products for one lead.  x (S, M, N, F) members, y (S, N, F) truth or None, w (N) weights, all
    float64 and standardised.  Returns prob (S, E, N), count (S, E, N) int64, quant (S, Q, N, F) physical, quant_std the same in
    standardised units, and with a truth brier (S, E), rel_count / rel_obs (S, E, M + 1) int32, pinball (S, Q, F), below (S, Q, F)
    int32.  Parts that were not asked for are missing."""
    x, w = x.double(), w.double()
    S, M, N, F = x.shape
    live = w != 0
    r = {}
    E, Q = len(event_var), len(q_index)
    if E:
        count = torch.zeros(S, E, N, dtype=torch.int64)
        obs = torch.zeros(S, E, N, dtype=torch.bool)
        for e in range(E):
            v, thr = int(event_var[e]), float(event_thr[e])
            xe = x[:, :, :, v]
            count[:, e] = ((xe < thr) if int(event_sense[e]) else (xe > thr)).sum(1)
            if y is not None:
                ye = y.double()[:, :, v]
                obs[:, e] = (ye < thr) if int(event_sense[e]) else (ye > thr)
        r["count"] = count
        r["prob"] = count.double() / M
        if y is not None:
            r["brier"] = (w.view(1, 1, N) * (r["prob"] - obs.double()) ** 2).sum(2)
            rel_count = torch.zeros(S, E, M + 1, dtype=torch.int32)
            rel_obs = torch.zeros(S, E, M + 1, dtype=torch.int32)
            for c in range(M + 1):
                hit = (count == c) & live.view(1, 1, N)
                rel_count[:, :, c] = hit.sum(2)
                rel_obs[:, :, c] = (hit & obs).sum(2)
            r["rel_count"], r["rel_obs"] = rel_count, rel_obs
    if Q:
        qs = quantiles(x, q_index, q_frac, dim=1)   # (S, Q, N, F)
        r["quant_std"] = qs
        r["quant"] = qs if state_std is None else qs * state_std.double() + state_mean.double()
        if y is not None:
            yy = y.double()[:, None]
            lev = torch.tensor([float(q) for q in q_level], dtype=torch.float64).view(1, Q, 1, 1)
            rho = torch.where(yy >= qs, lev * (yy - qs), (1.0 - lev) * (qs - yy))
            r["pinball"] = (w.view(1, 1, N, 1) * rho).sum(2)
            r["below"] = ((yy < qs) & live.view(1, 1, N, 1)).sum(2).to(torch.int32)
    return r
