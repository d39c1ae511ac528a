"""Numpy fp32 stand-ins of the reductions and grid-stride loops of the forecast path (nlam_forecast.inc, nlam_ensemble.inc,
nlam_ens_products.inc, nlam_ens_neighbourhood.inc, nlam_series.inc), with the defects tests/test_forecast_scale_kernels.py injects.

The chunk reductions.  A workgroup of forecast_tail_kernel / ens_scores_kernel / ens_products_kernel adds the terms of its chunk of
``cn`` nodes per output in node order (``chunk_partials``); forecast_finish_kernel / ens_finish_kernel / ens_products_finish_kernel
split the C chunks over four waves, ``per = (C + 3) // 4`` consecutive chunks each, added in order under an unroll by 8, and
combine the waves as (0 + 1) + (2 + 3) (``finish``).  Every addition is one fp32 addition (numpy float32 arrays; cumsum
accumulates in order).

Defects of ``finish``:
  wave3_dropped              the chunks of wave 3 are not added
  unroll_remainder_dropped   a wave that ran an unrolled body of 8 leaves out the chunks behind its last multiple of 8
  last_chunk_dropped         chunk C - 1 (the partial one) is not added
"""
import numpy as np

F32 = np.float32
ROW_CAP = 512 * 2048          # elements of a data row one sweep of window_grid / fc_row_blocks covers
FILL_CAP_QUADS = 4096 * 256   # quads of one sweep of nlam_philox_normal_fill
LATENT_CAP_QUADS = 1024 * 256  # quads of one sweep of nlam_latent_sample, per batch item
FINISH_DEFECTS = ("wave3_dropped", "unroll_remainder_dropped", "last_chunk_dropped")


def chunks_of(nodes, cn):
    return -(-nodes // cn)


def wave_split(C):
    """[(c0, c1)] of the four waves."""
    per = (C + 3) // 4
    return [(min(C, w * per), min(C, w * per + per)) for w in range(4)]


def regime(C):
    """What a chunk count reaches: per, the waves' chunk counts, whether a wave runs an unrolled body with a remainder."""
    counts = [c1 - c0 for c0, c1 in wave_split(C)]
    return {"per": (C + 3) // 4, "counts": counts, "waves_used": sum(n > 0 for n in counts), "two_in_a_wave": max(counts) >= 2,
            "body_and_remainder": any(n >= 8 and n % 8 for n in counts), "remainder_only": any(0 < n < 8 for n in counts)}


def chunk_partials(terms, cn):
    """terms (..., N) -> (..., C): the fp32 sum of each chunk of cn nodes, in node order (trailing zeros of the last chunk are exact)."""
    terms = np.asarray(terms)
    N = terms.shape[-1]
    C = chunks_of(N, cn)
    pad = np.zeros(terms.shape[:-1] + (C * cn - N,), terms.dtype)
    t = np.concatenate([terms, pad], axis=-1).reshape(terms.shape[:-1] + (C, cn))
    return np.cumsum(t, axis=-1, dtype=terms.dtype)[..., -1]


def finish(parts, defect=None):
    """parts (..., C) fp32 or integer -> (...): the finishers' order in the dtype of ``parts``."""
    assert defect is None or defect in FINISH_DEFECTS, defect
    parts = np.asarray(parts)
    C = parts.shape[-1]
    waves = []
    for w, (c0, c1) in enumerate(wave_split(C)):
        if defect == "wave3_dropped" and w == 3:
            c1 = c0
        if defect == "unroll_remainder_dropped" and c1 - c0 >= 8:
            c1 = c0 + (c1 - c0) // 8 * 8
        if defect == "last_chunk_dropped":
            c1 = min(c1, C - 1)
        v = np.zeros(parts.shape[:-1], parts.dtype)
        for c in range(c0, c1):
            v = v + parts[..., c]
        waves.append(v)
    return (waves[0] + waves[1]) + (waves[2] + waves[3])


def chunked_sum(terms64, cn, defect=None):
    """float64 per-node terms (..., N) -> the fp32 stand-in of one output: each term rounded to fp32 (U of it, inside every
    budget's per-node allowance), the chunk sums in node order, the finishers' order; returned as float64."""
    return finish(chunk_partials(np.asarray(terms64, dtype=np.float64).astype(F32), cn), defect).astype(np.float64)


def chunked_count(flags, cn, defect=None):
    """The same passes over integer counts (rank histogram, reliability table, `below`)."""
    return finish(chunk_partials(np.asarray(flags).astype(np.int32), cn), defect)


def forecast_finish(ws, defect=None):
    """forecast_finish_kernel on its workspace ws (B, C, 2 F) fp32 -> (B, 2 F): lane m0 + lane of round m0 owns sum m = b * 2 F + j.
    Defect ``second_round_wrong_item``: a sum of a later round (m >= 64) is read from the batch item of its lane in round 0."""
    assert defect in (None, "second_round_wrong_item") + FINISH_DEFECTS
    ws = np.asarray(ws, dtype=F32)
    B, C, W2 = ws.shape
    out = np.empty((B, W2), F32)
    for m in range(B * W2):
        b, j = divmod(m, W2)
        src = b if not (defect == "second_round_wrong_item" and m >= 64) else (m & 63) // W2
        out[b, j] = finish(ws[src, :, j], defect if defect in FINISH_DEFECTS else None)
    return out


def nbr_finish(words, defect=None):
    """nbr_finish_kernel on the words (..., nblocks) fp32 of one (start, event, scale, sum): lane l adds words l, l + 64, ... in
    order, then the shuffle tree d = 32 .. 1.  Defect ``words_past_64_dropped``: only the first round is added."""
    assert defect in (None, "words_past_64_dropped")
    words = np.asarray(words, dtype=F32)
    nb = words.shape[-1]
    v = np.zeros(words.shape[:-1] + (64,), F32)
    for b0 in range(0, nb if defect is None else min(nb, 64), 64):
        n = min(64, nb - b0)
        v[..., :n] = v[..., :n] + words[..., b0:b0 + n]
    d = 32
    while d:
        v[..., :d] = v[..., :d] + v[..., d:2 * d]
        d >>= 1
    return v[..., 0]


def nbr_words(terms64, block=256):
    """float64 per-node terms (..., N) -> (..., nblocks) fp32: the sum of each evaluation workgroup's 256 nodes (in node order: the
    budget of nlam_ens_neighbourhood's sums holds for any order)."""
    return chunk_partials(np.asarray(terms64, dtype=np.float64).astype(F32), block)


def row_with_cap_defect(row, sentinel=np.nan):
    """A data row whose elements at or past the capped grid's first sweep were never written."""
    out = np.array(row, dtype=F32, copy=True).reshape(-1)
    out[ROW_CAP:] = sentinel
    return out.reshape(np.shape(row))


def quad_normals(q, seed, c1, c2, c3):
    """float64 Box-Muller normals (len(q), 4) of the counters (q[i], c1, c2, c3): philox_ref.normals for any quad indices."""
    import philox_ref as P

    u = P.uniforms(P.philox_blocks(np.asarray(q), c1, c2, c3, seed))
    z = np.empty((len(q), 4))
    for h in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[:, 2 * h]))
        ang = 2.0 * np.pi * u[:, 2 * h + 1]
        z[:, 2 * h], z[:, 2 * h + 1] = r * np.cos(ang), r * np.sin(ang)
    return z


def normals_standin(n, seed, c1, c2, c3, cap_quads=None):
    """fp32 values of the generator for elements [0, n): the float64 normals rounded once.  ``cap_quads``: the defect -- the quad
    index of the counter taken modulo the grid's threads, so that a later sweep repeats the first."""
    q = np.arange((n + 3) // 4)
    if cap_quads is not None:
        q = q % cap_quads
    return quad_normals(q, seed, c1, c2, c3).reshape(-1)[:n].astype(F32)
