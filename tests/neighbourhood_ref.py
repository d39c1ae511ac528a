"""Reference of nlam_ens_neighbourhood (include/nlam_hip.h) in int64 and float64 torch: the three window sums by brute force --
one shifted slice of the grid per offset of the window, no summed-area table and no running sum, so it shares no trick with the
kernels --, the neighbourhood probability as the fp32 division the header defines, and the two sums of the fractions skill
score in float64.  ``event_thr`` holds the fp32 thresholds the kernel reads (standardised), cast to double here."""
import torch


def window_sums(a, r):
    """Sum of int64 ``a`` (..., nx, ny) over the window |i' - i| <= r, |j' - j| <= r clipped to the grid (no wrap, no padding)."""
    nx, ny = a.shape[-2:]
    out = torch.zeros_like(a)
    for di in range(-min(r, nx - 1), min(r, nx - 1) + 1):
        i0, i1 = max(0, -di), min(nx, nx - di)      # the rows i with 0 <= i + di < nx
        for dj in range(-min(r, ny - 1), min(r, ny - 1) + 1):
            j0, j1 = max(0, -dj), min(ny, ny - dj)
            out[..., i0:i1, j0:j1] += a[..., i0 + di:i1 + di, j0 + dj:j1 + dj]
    return out


def window_sum_explicit(a, r, i, j):
    """The same sum for one node of a 2-D ``a``, window by window: what ``window_sums`` is checked against."""
    nx, ny = a.shape
    return sum(int(a[ii, jj]) for ii in range(nx) for jj in range(ny) if abs(ii - i) <= r and abs(jj - j) <= r)


def counts(x, y, w, event_var, event_sense, event_thr):
    """C (S, E, N) int64: the members in the event; O (S, E, N) int64 or None: the truth in it; live (N) int64.  Not yet masked."""
    x = x.double()
    S, M, N, F = x.shape
    C = torch.zeros(S, len(event_var), N, dtype=torch.int64)
    O = None if y is None else torch.zeros(S, len(event_var), N, dtype=torch.int64)
    for e, (v, sense, thr) in enumerate(zip(event_var, event_sense, event_thr)):
        xe = x[:, :, :, int(v)]
        C[:, e] = ((xe < float(thr)) if int(sense) else (xe > float(thr))).sum(1)
        if y is not None:
            ye = y.double()[:, :, int(v)]
            O[:, e] = ((ye < float(thr)) if int(sense) else (ye > float(thr))).long()
    return C, O, (w != 0).long()


def ens_neighbourhood(x, y, w, event_var, event_sense, event_thr, radii, nx, ny):
    """The outputs of nlam_ens_neighbourhood for one lead.  x (S, M, N, F) members, y (S, N, F) truth or None, w (N) weights,
    N = nx * ny with node n = i * ny + j.  Returns A (W, N), SC (S, E, W, N) and SO (the same, with a truth) as int64, nprob
    (S, E, W, N) float32 = (float)SC / (float)(M A) with NaN where A = 0, p and o the same fractions in float64, and with a truth
    fbs / fbs_ref (S, E, W) in float64 over the live nodes."""
    S, M, N, F = x.shape
    assert N == nx * ny and M * N <= 2 ** 24
    C, O, live = counts(x, y, w, event_var, event_sense, event_thr)
    E = C.shape[1]
    grid = lambda t: t.reshape(*t.shape[:-1], nx, ny)   # noqa: E731
    A, SC, SO = [], [], []
    for r in radii:
        r = max(int(r), 0)
        A.append(window_sums(grid(live), r).reshape(N))
        SC.append(window_sums(grid(C * live), r).reshape(S, E, N))
        if O is not None:
            SO.append(window_sums(grid(O * live), r).reshape(S, E, N))
    out = {"A": torch.stack(A, 0), "SC": torch.stack(SC, 2)}
    A_ = out["A"].view(1, 1, len(radii), N)
    out["nprob"] = out["SC"].float() / (M * A_).float()          # both conversions exact, one correctly rounded division; 0 / 0 = NaN
    out["p"] = out["SC"].double() / (M * A_).double()
    if O is not None:
        out["SO"] = torch.stack(SO, 2)
        out["o"] = out["SO"].double() / A_.double()
        lv = (live != 0).view(1, 1, 1, N)
        wd = w.double().view(1, 1, 1, N)
        zero = torch.zeros((), dtype=torch.float64)
        p, o = torch.where(lv, out["p"], zero), torch.where(lv, out["o"], zero)   # a live node is in its own window: no NaN there
        out["fbs"] = (wd * (p - o) ** 2).sum(-1)
        out["fbs_ref"] = (wd * (p ** 2 + o ** 2)).sum(-1)
    return out


def fss(fbs, fbs_ref):
    """1 - sum_s fbs / sum_s fbs_ref over the leading axis; NaN where the denominator is 0."""
    return 1.0 - fbs.sum(0) / fbs_ref.sum(0)
