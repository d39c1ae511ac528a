"""Reference of the ensemble kernels (include/nlam_hip.h: nlam_philox_normal_fill, nlam_latent_sample, nlam_ens_scores) without the
library: Philox4x32-10 in plain Python integers and vectorised in numpy, its float64 Box-Muller normals, the float64
reparameterised draw, and the float64 ensemble scores.  test_ensemble_forecast.py pins the generator against the Random123 known
answers and the score math against hand-computed cases before it uses either on the GPU."""
import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Ten rounds on one counter of four 32-bit words under a key of two: plain Python integers."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_blocks(q, c1, c2, c3, seed):
    """(len(q), 4) uint64 array of 32-bit words: the blocks of the counters (q[i], c1, c2, c3) under the 64-bit seed."""
    q = np.asarray(q, dtype=np.uint64)
    mask = np.uint64(MASK)
    s32 = np.uint64(32)
    c = [q & mask] + [np.full_like(q, int(v) & MASK) for v in (c1, c2, c3)]
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]   # 32 x 32 bits: no overflow in 64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=1)


def uniforms(words):
    """((x >> 9) + 0.5) * 2^-23 in float64 (the value the kernel holds exactly in fp32)."""
    return ((np.asarray(words, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(n, seed, c1, c2, c3):
    """float64 values of nlam_philox_normal_fill: element i is number i % 4 of counter (i // 4, c1, c2, c3); the four numbers of
    a block are (r_a cos, r_a sin, r_b cos, r_b sin) of the Box-Muller pairs (u0, u1) and (u2, u3)."""
    nq = (n + 3) // 4
    u = uniforms(philox_blocks(np.arange(nq), c1, c2, c3, seed))
    z = np.empty((nq, 4))
    for h in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[:, 2 * h]))
        ang = 2.0 * np.pi * u[:, 2 * h + 1]
        z[:, 2 * h], z[:, 2 * h + 1] = r * np.cos(ang), r * np.sin(ang)
    return z.reshape(-1)[:n]


def latent_noise(lead, members, t0, per, seed):
    """(len(t0), per) float64: the draws of nlam_latent_sample at lead ``lead`` for batch items b with start times t0[b]."""
    return np.stack([normals(per, seed, lead, b % members, int(t) & MASK) for b, t in enumerate(t0)])


def latent_sample(params, noise, diagonal, dtype=torch.float64):
    """mean + (1e-4 + softplus(std_raw)) * noise, or mean + noise for an isotropic prior, in ``dtype`` on the CPU."""
    params, noise = params.to(dtype), noise.to(dtype)
    if not diagonal:
        return params + noise
    mean, raw = params.chunk(2, dim=-1)
    return mean + (1e-4 + torch.nn.functional.softplus(raw)) * noise


def ens_scores(x, y, w, state_mean=None, state_std=None):
    """The outputs of nlam_ens_scores for one lead in float64.  x (S, M, N, F) members, y (S, N, F) truth, w (N) weights."""
    x, y, w = x.to(torch.float64), y.to(torch.float64), w.to(torch.float64)
    S, M, N, F = x.shape
    xbar = x.mean(dim=1)
    wn = w.view(1, N, 1)
    var = ((x - xbar[:, None]) ** 2).sum(dim=1) / (M - 1) if M > 1 else torch.zeros_like(xbar)
    pair = torch.zeros_like(xbar)
    for i in range(M):
        for j in range(i):
            pair = pair + (x[:, i] - x[:, j]).abs()
    pair = pair / (M * (M - 1)) if M > 1 else pair
    out = {"ens_sq": (wn * (xbar - y) ** 2).sum(dim=1), "ens_var": (wn * var).sum(dim=1),
           "ens_abs": (wn * (x - y[:, None]).abs().mean(dim=1)).sum(dim=1), "ens_pair": (wn * pair).sum(dim=1)}
    rank = (x < y[:, None]).sum(dim=1)   # (S, N, F): members strictly below the truth
    live = (w != 0).view(1, N, 1)
    out["rank_hist"] = torch.stack([((rank == r) & live).sum(dim=1) for r in range(M + 1)], dim=-1).to(torch.int32)   # (S, F, M + 1)
    mean = torch.zeros(F, dtype=torch.float64) if state_mean is None else state_mean.to(torch.float64)
    std = torch.ones(F, dtype=torch.float64) if state_std is None else state_std.to(torch.float64)
    out["mean"], out["spread"] = xbar * std + mean, var.sqrt() * std
    return out
