"""Reference of the ensemble CRPS fine-tuning kernels (include/nlam_hip.h: nlam_latent_draw_fwd / _bwd, nlam_crps_ens_fwd / _bwd)
without the library: the float64 unbiased ensemble CRPS per element with the magnitudes of the pieces the kernel adds, its
closed-form (sub)gradient, the float64 prior draw and its gradient, and the closed-form CRPS of a Gaussian.  test_efm_crps.py checks
these against a brute-force double loop, float64 autograd and a Monte-Carlo estimate before it uses them on the GPU."""
import math

import torch

import elbo_ref as E

MEMBER_KEY_OFFSET = 0xD1B54A32D192ED03


def member_key(seed, rank):
    """The key of the member draws: the posterior's key (seed + rank * golden ratio) plus the offset, mod 2^64."""
    return (int(seed) + int(rank) * 0x9E3779B97F4A7C15 + MEMBER_KEY_OFFSET) & 0xFFFFFFFFFFFFFFFF


def bracket(x, y):
    """x (B, M, N, F) members, y (B, N, F) target -> float64 (B, N, F): 1/M sum_m |x_m - y| - 1/(M (M - 1)) sum_{i<j} |x_i - x_j|,
    and the magnitude 1/M sum |x_m - y| + 1/(M (M - 1)) sum_{i<j} |x_i - x_j| of the two pieces (the bracket cancels)."""
    x, y = x.to(torch.float64), y.to(torch.float64)
    M = x.shape[1]
    skill = (x - y[:, None]).abs().sum(1) / M
    pair = torch.zeros_like(skill)
    for i in range(M):
        for j in range(i + 1, M):
            pair = pair + (x[:, i] - x[:, j]).abs()
    pair = pair / (M * (M - 1))
    return skill - pair, skill + pair


def weights(w, c, F):
    """(N, F) float64: row_weight[n] * var_weight[f] of the fp32 values handed in (var_weight None: ones)."""
    w = w.to(torch.float64).reshape(-1, 1)
    return w * (torch.ones(1, F, dtype=torch.float64) if c is None else c.to(torch.float64).reshape(1, F))


def forward(x, y, w, c, weight):
    """(crps (B,), term, mag (B,)) in float64: crps[b] = sum_n,f w_n c_f bracket, term = weight * sum_b crps[b]; mag[b] the sum of
    the magnitudes of what is added."""
    v, m = bracket(x, y)
    wc = weights(w, c, x.shape[-1])
    crps = (v * wc).sum((1, 2))
    return crps, float(weight) * float(crps.sum()), (m * wc.abs()).sum((1, 2))


def sgn(a, b):
    """(a > b) - (a < b): the sign by comparison, 0 at a tie."""
    return (a > b).to(torch.float64) - (a < b).to(torch.float64)


def backward(x, y, w, c, gw):
    """The closed-form (sub)gradient of gw * sum_b crps[b] with respect to x, float64 (B, M, N, F), and the magnitude
    |gw w_n c_f| (|sgn(x_m - y)| / M + |sum_{j != m} sgn(x_m - x_j)| / (M (M - 1))) of its two pieces."""
    x, y = x.to(torch.float64), y.to(torch.float64)
    M = x.shape[1]
    wc = weights(w, c, x.shape[-1])
    sy = sgn(x, y[:, None])
    pairs = torch.zeros_like(x)
    for m in range(M):
        for j in range(M):
            if j != m:
                pairs[:, m] += sgn(x[:, m], x[:, j])
    g = float(gw) * wc * (sy / M - pairs / (M * (M - 1)))
    mag = abs(float(gw)) * wc.abs() * (sy.abs() / M + pairs.abs() / (M * (M - 1)))
    return g, mag


def draw(params, eps, D):
    """float64 latent = mean + std eps of params (B, R, D | 2 D), and |mean| + |std eps|."""
    params, eps = params.to(torch.float64), eps.to(torch.float64)
    mean = params[..., :D]
    std = E.LATENT_STD_EPS + torch.nn.functional.softplus(params[..., D:]) if params.shape[-1] == 2 * D else torch.ones_like(mean)
    return mean + std * eps, mean.abs() + (std * eps).abs()


def draw_backward(params, eps, g, D):
    """float64 g_params of (latent * g).sum(): g | g eps softplus'(raw) (threshold 20: derivative 1 above)."""
    params, eps, g = params.to(torch.float64), eps.to(torch.float64), g.to(torch.float64)
    if params.shape[-1] == D:
        return g
    raw = params[..., D:]
    return torch.cat((g, g * eps * torch.where(raw > 20.0, torch.ones_like(raw), torch.sigmoid(raw))), -1)


def gaussian_crps(mu, sigma, y):
    """The closed-form CRPS of N(mu, sigma^2) at y (Gneiting & Raftery 2007, eq. 21)."""
    z = (y - mu) / sigma
    pdf = math.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    cdf = 0.5 * (1 + math.erf(z / math.sqrt(2)))
    return sigma * (z * (2 * cdf - 1) + 2 * pdf - 1 / math.sqrt(math.pi))
