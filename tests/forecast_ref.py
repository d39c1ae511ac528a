"""float64 torch-CPU restatement of the forecast engine's two kernels (include/nlam_hip.h, nlam_forecast_t): the head's indexing
(restated from the comment of nlam_window_t: sample -> time indices, feature-major / window-minor forcing window, clamped time
index) and the tail's formulas (restated from the comment of nlam_step_tail_t: rescaled delta, the three clamp modes, softplus,
the boundary mix; then the de-standardisation and the two masked sums of nlam_forecast_tail).  test_forecast.py pins it against the
oracle's ARForecaster on the CPU and leans on it for the GPU tests.  Nothing here imports the product."""
import torch

CLAMP_NONE, CLAMP_BOTH, CLAMP_LOWER, CLAMP_UPPER = 0, 1, 2, 3
F64 = torch.float64
# the constants as torch holds them in fp32 (utils/tensor.py: inverse_softplus' lower clamp, inverse_sigmoid's clamp)
ISP_LOW = float(torch.log(torch.tensor(1.0 + 1e-6, dtype=torch.float32)))
SIG_LOW = float(torch.tensor(1e-6, dtype=torch.float32))
SIG_HIGH = float(torch.tensor(1.0 - 1e-6, dtype=torch.float32))
THRESHOLD = 20.0


def softplus(z):
    return torch.where(z > THRESHOLD, z, torch.log1p(torch.exp(torch.clamp(z, max=THRESHOLD))))


def inv_softplus(y):
    return torch.where(y > THRESHOLD, y, torch.log(torch.expm1(torch.clamp(y, ISP_LOW, THRESHOLD))))


def clamp_tables(predictor):
    """(modes [F], lo (F,), hi (F,)) float64 from the buffers ``prepare_clamping_params`` registers (oracle and product alike)."""
    n = predictor.state_mean.shape[0]
    modes, lo, hi = [CLAMP_NONE] * n, torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for j, i in enumerate(predictor.clamp_lower_upper_idx.tolist()):
        modes[i], lo[i], hi[i] = CLAMP_BOTH, float(predictor.sigmoid_lower_lims[j]), float(predictor.sigmoid_upper_lims[j])
    for j, i in enumerate(predictor.clamp_lower_idx.tolist()):
        modes[i], lo[i] = CLAMP_LOWER, float(predictor.softplus_lower_lims[j])
    for j, i in enumerate(predictor.clamp_upper_idx.tolist()):
        modes[i], hi[i] = CLAMP_UPPER, float(predictor.softplus_upper_lims[j])
    return modes, lo, hi


def plan(n_times, past, future, max_lead):
    """(off, number of valid starts): a start i has t0 = i + off - 1 and needs t0 + max_lead + future <= n_times - 1."""
    off = max(2, past)
    return off, max(0, n_times - (off + max_lead + future) + 1)


def lead_times(t0, k, past, future, n_times):
    """Clamped time indices lead k + 1 (k leads already produced) reads: (valid time, [window slot times])."""
    c = lambda t: min(max(t, 0), n_times - 1)   # noqa: E731
    tv = t0 + k + 1
    return c(tv), [c(tv - past + w) for w in range(past + future + 1)]


def head(state, forcing, t0s, k, past, future, state_mean, state_std, forcing_mean=None, forcing_std=None):
    """(forcing_windowed (B, N, d_forcing * window) or None, truth (B, N, F)), standardised, float64."""
    n_times = state.shape[0]
    fws, truths = [], []
    for t0 in t0s:
        tv, slots = lead_times(int(t0), k, past, future, n_times)
        truths.append((state[tv].to(F64) - state_mean.to(F64)) / state_std.to(F64))
        if forcing is not None:
            w = torch.stack([(forcing[t].to(F64) - forcing_mean.to(F64)) / forcing_std.to(F64) for t in slots])   # (window, N, f)
            fws.append(w.permute(1, 2, 0).reshape(w.shape[1], -1))   # feature-major, window-minor
    return (torch.stack(fws) if fws else None), torch.stack(truths)


def init(state, t0s, state_mean, state_std):
    """(prev_prev, prev): the standardised states at t0 - 1 and t0, float64."""
    n_times = state.shape[0]
    c = lambda t: min(max(int(t), 0), n_times - 1)   # noqa: E731
    z = lambda t: (state[c(t)].to(F64) - state_mean.to(F64)) / state_std.to(F64)   # noqa: E731
    return torch.stack([z(t0 - 1) for t0 in t0s]), torch.stack([z(t0) for t0 in t0s])


def tail(delta, prev, truth, dstd, dmean, bmask, modes, lo, hi, state_mean, state_std, row_weight=None):
    """One lead's tail in float64.  delta (B, N, F | 2 F), prev / truth (B, N, F), bmask / row_weight (N,).
    Returns dict: new (B, N, F) standardised, out_state physical, out_std physical or None, sq / ab (B, F) or None."""
    delta, prev, truth = delta.to(F64), prev.to(F64), truth.to(F64)
    F = prev.shape[-1]
    r = delta[..., :F] * dstd.to(F64) + dmean.to(F64)
    new = prev + r
    for f, m in enumerate(modes):
        p, rf = prev[..., f], r[..., f]
        lo_f, hi_f = float(lo[f]), float(hi[f])
        if m == CLAMP_BOTH:
            u = torch.clamp((p - lo_f) / (hi_f - lo_f), SIG_LOW, SIG_HIGH)
            new[..., f] = lo_f + (hi_f - lo_f) * torch.sigmoid(torch.log(u / (1 - u)) + rf)
        elif m == CLAMP_LOWER:
            new[..., f] = lo_f + softplus(inv_softplus(p - lo_f) + rf)
        elif m == CLAMP_UPPER:
            new[..., f] = hi_f - softplus(inv_softplus(hi_f - p) - rf)
    bm = bmask.to(F64).reshape(1, -1, 1)
    new = bm * truth + (1 - bm) * new
    out = {"new": new, "out_state": new * state_std.to(F64) + state_mean.to(F64), "out_std": None, "sq": None, "ab": None}
    if delta.shape[-1] == 2 * F:
        out["out_std"] = softplus(delta[..., F:]) * state_std.to(F64)
    if row_weight is not None:
        out["sq"], out["ab"] = masked_sums(new, truth, row_weight)
    return out


def masked_sums(new, truth, row_weight):
    """(sq, ab) (B, F): sum_n row_weight[n] * (new - truth)^2 and sum_n row_weight[n] * |new - truth| in float64."""
    w = row_weight.to(F64).reshape(1, -1, 1)
    d = new.to(F64) - truth.to(F64)
    return (w * d * d).sum(dim=1), (w * d.abs()).sum(dim=1)


def rollout(net, state, forcing, t0s, leads, past, future, stats, dstd, dmean, bmask, modes, lo, hi, row_weight=None):
    """``leads`` replays of head -> net -> tail.  ``net(prev, prev_prev, forcing_windowed)`` takes and returns fp32 tensors (the raw
    network output (B, N, F | 2 F)); the state handed to the next lead is the float64 result rounded to fp32, as the engine keeps it.
    Returns dict of stacked (B, leads, ...) float64 tensors: new, out_state, out_std, sq, ab."""
    f32 = torch.float32
    pprev, prev = (t.to(f32) for t in init(state, t0s, stats["state_mean"], stats["state_std"]))
    outs = []
    for k in range(leads):
        fw, truth = head(state, forcing, t0s, k, past, future, stats["state_mean"], stats["state_std"], stats.get("forcing_mean"),
                         stats.get("forcing_std"))
        fw = fw.to(f32) if fw is not None else torch.zeros(prev.shape[0], prev.shape[1], 0)
        truth = truth.to(f32)
        delta = net(prev, pprev, fw)
        o = tail(delta, prev, truth, dstd, dmean, bmask, modes, lo, hi, stats["state_mean"], stats["state_std"], row_weight)
        outs.append(o)
        pprev, prev = prev, o["new"].to(f32)
    stack = lambda key: None if outs[0][key] is None else torch.stack([o[key] for o in outs], dim=1)   # noqa: E731
    return {key: stack(key) for key in ("new", "out_state", "out_std", "sq", "ab")}
