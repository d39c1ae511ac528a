"""Reference of the Graph-EFM training kernels (include/nlam_hip.h: nlam_latent_kl_fwd / nlam_latent_kl_bwd) without the library:
the float64 posterior draw, the per-element KL terms and their magnitudes, the closed-form gradients, and the Philox draws of
the kernel's counter.  test_efm_training.py checks the KL against torch.distributions and the gradients against float64
autograd before it uses either on the GPU."""
import numpy as np
import torch

import philox_ref as P

LATENT_STD_EPS = 1e-4


def split(pq, pp):
    """(mu_q, raw_q, mu_p, raw_p | None) in float64; pq (B, R, 2 D), pp (B, R, D | 2 D)."""
    pq, pp = pq.to(torch.float64), pp.to(torch.float64)
    D = pq.shape[-1] // 2
    mu_q, raw_q = pq[..., :D], pq[..., D:]
    if pp.shape[-1] == 2 * D:
        return mu_q, raw_q, pp[..., :D], pp[..., D:]
    return mu_q, raw_q, pp, None


def stds(raw_q, raw_p):
    sp = torch.nn.functional.softplus
    s_q = LATENT_STD_EPS + sp(raw_q)
    s_p = torch.ones_like(s_q) if raw_p is None else LATENT_STD_EPS + sp(raw_p)
    return s_q, s_p


def forward(pq, pp, eps):
    """float64: z (B, R, D), the per-element KL terms (B, R, D) and the sum of the magnitudes of the pieces the kernel adds per
    element (|log r| + r^2 / 2 + n^2 / 2 + 1 / 2): what a rounding-error budget scales with where the KL itself cancels."""
    mu_q, raw_q, mu_p, raw_p = split(pq, pp)
    s_q, s_p = stds(raw_q, raw_p)
    z = mu_q + s_q * eps.to(torch.float64)
    r, n = s_q / s_p, (mu_q - mu_p) / s_p
    term = torch.log(s_p / s_q) + (s_q ** 2 + (mu_q - mu_p) ** 2) / (2 * s_p ** 2) - 0.5
    mag = torch.log(r).abs() + 0.5 * r * r + 0.5 * n * n + 0.5
    return z, term, mag


def kl_per_item(pq, pp):
    """(B,) float64: KL_b = sum_{r,d} of the terms."""
    return forward(pq, pp, torch.zeros(pq.shape[:-1] + (pq.shape[-1] // 2,)))[1].sum((1, 2))


def backward(pq, pp, eps, g_z, w):
    """The closed-form gradients of  (z * g_z).sum() + w * sum_b KL_b  in float64: (g_pq, g_pp, magnitudes of g_pq's and g_pp's
    pieces).  ``g_z`` None is a zero cotangent."""
    mu_q, raw_q, mu_p, raw_p = split(pq, pp)
    s_q, s_p = stds(raw_q, raw_p)
    eps = eps.to(torch.float64)
    g = torch.zeros_like(mu_q) if g_z is None else g_z.to(torch.float64)
    dlt = mu_q - mu_p
    dsp = lambda x: torch.where(x > 20.0, torch.ones_like(x), torch.sigmoid(x))   # noqa: E731  softplus' (threshold 20: linear above)
    sig_q = dsp(raw_q)
    d_mu_q = g + w * dlt / s_p ** 2
    d_raw_q = (g * eps + w * (s_q / s_p ** 2 - 1 / s_q)) * sig_q
    d_mu_p = -w * dlt / s_p ** 2
    mag_mu = g.abs() + (w * dlt / s_p ** 2).abs()
    mag_raw_q = ((g * eps).abs() + abs(w) * (s_q / s_p ** 2 + 1 / s_q)) * sig_q
    g_pq, mag_pq = torch.cat((d_mu_q, d_raw_q), -1), torch.cat((mag_mu, mag_raw_q), -1)
    if raw_p is None:
        return g_pq, d_mu_p, mag_pq, d_mu_p.abs()
    sig_p = dsp(raw_p)
    d_raw_p = w * (1 / s_p - (s_q ** 2 + dlt ** 2) / s_p ** 3) * sig_p
    mag_raw_p = abs(w) * (1 / s_p + (s_q ** 2 + dlt ** 2) / s_p ** 3) * sig_p
    return g_pq, torch.cat((d_mu_p, d_raw_p), -1), mag_pq, torch.cat((d_mu_p.abs(), mag_raw_p), -1)


def noise(seed, draw, t, batch, per):
    """(batch, per) float64: the draws of nlam_latent_kl_fwd -- element e of item b is number e % 4 of the Philox counter
    (e // 4, t, b, low word of draw) under the 64-bit ``seed``."""
    return np.stack([P.normals(per, seed, t, b, int(draw) & P.MASK) for b in range(batch)])
