"""Float64 reference of nlam_dct_spectra and the rounding budget its tests hold the launch to.  Nothing here comes from the code
under test: the transform is scipy.fft.dctn, the basis of the budget scipy.fft.dct of the identity, the bins a double loop in
Python integers.

The reference.  For a window g (cx, cy) of one field, G = dctn(g, type=2, norm="ortho") in float64 of the fp32 inputs,
s2 = G^2 / (cx cy), and bin b holds scale * the sum of s2 over the coefficients (m, n) with bin_of[m][n] == b.  By Parseval the
bins of the default table add up to scale * g.var() (the population variance): (0, 0) carries the mean and is dropped.

The budget is derived, not tuned.  The launch computes G as two chained fp32 dot products on v_mfma_f32_16x16x4_f32 (bit for bit
an fp32 fmaf chain in ascending index order): first along j, length cy, then along i, length cx, with basis entries that were
rounded once from float64 to fp32.  With u = 2^-24 and the standard bound of a recursive dot product (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1: |fl(x.y) - x.y| <= gamma_n |x|.|y|, gamma_n ~ n u):
    first pass    |dT(i, n)|  <= (cy + 1) u sum_j |Cy[n][j]| |g(i, j)|          (cy roundings of the chain + 1 of the basis entry)
    second pass   |dG(m, n)|  <= (cx + 1) u sum_i |Cx[m][i]| |T(i, n)| + sum_i |Cx[m][i]| |dT(i, n)|
and since |T| <= |g| |Cy^T| entry by entry, to first order in u
    e(m, n) = (cx + cy + 2) u (|Cx| |g| |Cy^T|)(m, n).
A bin then adds count values G^2 (the square is exact inside the fma that adds it): |(G + dG)^2 - G^2| <= 2 |G| e + e^2 per
coefficient, the fixed-order sum of count non-negative terms loses at most count u of the sum, and the scale and the final
rounding two more u:
    budget(bin) = scale / (cx cy) sum_bin (2 |G| e + e^2) + (count + 2) u S_bin.
A CPU experiment with numpy fp32 matmuls in place of the launch stayed at 2e-4 to 2e-2 of this budget at the tests' shapes, and a
window shifted by one row exceeded it 50 to 1e5 times in the median bin: the budget is neither tight enough to fail a correct
launch nor loose enough to pass a wrong one.  The tests also assert, from the reference alone and before they compare, that the
budget is at most 5 % of the bin's power in every bin (white fields at every shape; red fields, amplitude ~ alpha^-2, up to
70 x 45)."""
import functools
import math

import numpy as np
import scipy.fft

U = 2.0 ** -24   # fp32 unit roundoff


def bins_ref(cx, cy):
    """bin_of (cx, cy) int64 by the double loop in Python integers: the Denis binning with Nmin = min(cx, cy)."""
    return _bins_ref(int(cx), int(cy)).copy()


@functools.lru_cache(maxsize=None)
def _bins_ref(cx, cy):
    nmin = min(cx, cy)
    out = np.full((cx, cy), -1, dtype=np.int64)
    for m in range(cx):
        for n in range(cy):
            if m == 0 and n == 0:
                continue
            num = (m * m * cy * cy + n * n * cx * cx) * nmin * nmin
            den = cx * cx * cy * cy
            k = 0
            while (k + 1) * (k + 1) * den <= num:   # the largest k with k^2 den <= num
                k += 1
            out[m, n] = max(k, 1) - 1 if k <= nmin - 1 else nmin - 1
    return out


def basis_ref(n):
    """The orthonormal DCT-II matrix C[k][i]: scipy's transform of the identity."""
    return scipy.fft.dct(np.eye(n), type=2, norm="ortho", axis=0)


def spectra_ref(field, bin_of, nb, scale=1.0, with_budget=True):
    """``field`` (cx, cy) (any float dtype; taken to float64), ``bin_of`` (cx, cy) integers in [-1, nb).  Returns ``(spec, budget)``,
    both (nb) float64; ``budget`` is None without ``with_budget``."""
    g = np.asarray(field, dtype=np.float64)
    cx, cy = g.shape
    bin_of = np.asarray(bin_of).reshape(cx, cy)
    G = scipy.fft.dctn(g, type=2, norm="ortho")
    s2 = G * G / (cx * cy)
    keep = bin_of >= 0
    spec = np.bincount(bin_of[keep], weights=s2[keep], minlength=nb)[:nb] * scale
    if not with_budget:
        return spec, None
    e = (cx + cy + 2) * U * (np.abs(basis_ref(cx)) @ np.abs(g) @ np.abs(basis_ref(cy)).T)
    per = (2.0 * np.abs(G) * e + e * e) * (scale / (cx * cy))
    count = np.bincount(bin_of[keep], minlength=nb)[:nb]
    budget = np.bincount(bin_of[keep], weights=per[keep], minlength=nb)[:nb] + (count + 2) * U * spec
    return spec, budget


def white_field(rng, shape):
    """Zero-mean unit-variance white noise, fp32."""
    return rng.standard_normal(shape).astype(np.float32)


def red_field(rng, cx, cy):
    """A red spectrum: DCT coefficients of amplitude k^-2 with random signs, k = Nmin alpha the wavenumber in units of the first bin
    (alpha the normalised wavenumber), flat below k = 1, no mean; normalised to unit variance, fp32.  For windows up to 70 x 45
    (the precondition of the module docstring)."""
    m, n = np.meshgrid(np.arange(cx), np.arange(cy), indexing="ij")
    k = np.maximum(np.sqrt((m / cx) ** 2 + (n / cy) ** 2) * min(cx, cy), 1.0)
    coef = rng.choice([-1.0, 1.0], size=(cx, cy)) / k ** 2
    coef[0, 0] = 0.0
    g = scipy.fft.idctn(coef, type=2, norm="ortho")
    return (g / g.std()).astype(np.float32)


def wavenumbers(nb):
    """k / Nmin of bin k - 1; NaN for the corner bin."""
    wn = np.arange(1, nb + 1, dtype=np.float64) / nb
    wn[-1] = math.nan
    return wn
