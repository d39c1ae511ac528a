// nlam_ens_products: exceedance probabilities and quantile fields of a sampled ensemble, and the scores that verify them,
// inside the recorded forecast step (after nlam_ens_scores, before nlam_forecast_finish).
//
// The geometry of ens_scores_kernel: a workgroup owns (start, chunk of fc_chunk_nodes whole nodes) and passes the chunk through
// an LDS tile in pieces of whole nodes -- rows 0 .. M - 1 the members, the last row the truth -- with 16-byte loads where every
// row of the piece is aligned (DESIGN 4.17's rule).  A piece then goes through three phases, a barrier between them:
//   events     one thread per (event, node), node-minor: it reads the M members of (node, event_var) from the tile, counts those in
//              the event, writes prob = c / M straight to global memory -- prob[e][n] is contiguous in n, so consecutive lanes
//              write consecutive words and the tile would only transpose nothing -- and leaves (c, truth in the event) of a live
//              node in a side table of the LDS.
//   quantiles  one thread per element: the members go into registers (a template on the member count rounded up to a power of
//              two, padded with the largest key: above +inf and every NaN, so the M smallest are always the members), a
//              compile-time bitonic network sorts them as order-preserving integer keys (an exact permutation: signed zeros
//              and NaNs keep their bits, and a NaN member gives NaN quantiles), the M sorted values return to the
//              element's own column, and the Q order statistics are read back from that column at the run-time indices of the
//              quantile table -- a run-time index into the register array would put it in scratch.  The padding never leaves
//              the registers.  Q_j = fma(g, x_(hi) - x_(lo), x_(lo)) replaces rows 0 .. Q - 1 of the column, in standardised units.
//   out        the Q rows leave through the tile, rescaled to physical units, with 16-byte stores where the row is aligned;
//              Q F threads add pinball loss and count the truths below per (quantile, variable) in node order, E threads add the
//              Brier terms, 2 E (M + 1) threads count the reliability table, all into the workgroup's own workspace words.
// ens_products_finish_kernel adds the chunks in the order of ens_finish_kernel.  No floating-point atomics: two runs give the
// same bits.  With truth == NULL the truth row and the side table are not filled (they stay in the sizing, so a piece has the same
// nodes with and without the truth), nothing is summed and there is no finishing launch.  Both kernels only read
// *lead and do nothing once *lead >= max_lead.  The tables' indices are clamped into range as they are staged (their ranges are
// the caller's to check; a bad one must not become an address).
// Included from nlam_hip.hip inside NLAM_IN_TU(1), behind nlam_ensemble.inc (ens_store_quad, kEnsTileFloats; fc_chunk_nodes, launch<>).

namespace {

constexpr int kProdTabWords = 3 * NLAM_ENS_MAX_EVENTS + 3 * NLAM_ENS_MAX_QUANTILES;

// rows of the tile: M members going in, Q quantiles coming out, and the truth behind both
__host__ __device__ __forceinline__ int prod_rows(int members, int quantiles) { return (members > quantiles ? members : quantiles) + 1; }
// whole nodes per piece: what kEnsTileFloats words hold of tile rows, the E side-table words of a node and the tables; a multiple
// of 4 where there are that many, never more than the chunk
__host__ __device__ __forceinline__ int prod_tile_nodes(int nvars, int members, int events, int quantiles) {
    int n = (kEnsTileFloats - kProdTabWords) / (prod_rows(members, quantiles) * nvars + events);
    if (n >= 4) n &= ~3;
    const int cn = fc_chunk_nodes(nvars);
    return n < 1 ? 1 : (n > cn ? cn : n);
}
__host__ __device__ __forceinline__ int prod_stride(int tile_nodes, int nvars) { return (tile_nodes * nvars + 3) & ~3; }
// words per (start, chunk) of the workspace: E Brier and Q F pinball sums (float), then rel_count and rel_obs E (M + 1) each and
// the Q F counts of truths below (int32)
__host__ __device__ __forceinline__ int prod_ws_words(int nvars, int members, int events, int quantiles) {
    return events * (2 * members + 3) + 2 * quantiles * nvars;
}

// A float as an int32 key of the same order (its own inverse): the sign bit flips the magnitude bits of a negative value.  The
// network then runs on v_min_i32 / v_max_i32 -- an exact permutation for every bit pattern (-0 below +0, negative NaNs at the
// bottom, positive ones above +inf, the padding 0x7fffffff on top) at two instructions per pair and no compare mask in SGPRs.
__device__ __forceinline__ int prod_key(int bits) { return bits ^ ((bits >> 31) & 0x7fffffff); }

// compare-and-swap of v[I] and v[I ^ J] in bitonic stage (K, J): ascending where bit K of I is clear
template <int I, int K, int J, int MB>
__device__ __forceinline__ void prod_cas(int (&v)[MB]) {
    constexpr int P = I ^ J;
    if constexpr (P > I) {
        const int a = v[I], b = v[P];
        v[I] = (I & K) == 0 ? min(a, b) : max(a, b);
        v[P] = (I & K) == 0 ? max(a, b) : min(a, b);
    }
}
template <int K, int J, int MB, int... I>
__device__ __forceinline__ void prod_stage(int (&v)[MB], std::integer_sequence<int, I...>) {
    (prod_cas<I, K, J, MB>(v), ...);
}
template <int K, int J, int MB>
__device__ __forceinline__ void prod_merge(int (&v)[MB]) {
    prod_stage<K, J, MB>(v, std::make_integer_sequence<int, MB>{});
    if constexpr (J > 1) prod_merge<K, J / 2, MB>(v);
}
// v ascending: the bitonic network, MB log2(MB) (log2(MB) + 1) / 4 pairs, every index a compile-time constant
template <int K, int MB>
__device__ __forceinline__ void prod_sort(int (&v)[MB]) {
    prod_merge<K, K / 2, MB>(v);
    if constexpr (K < MB) prod_sort<2 * K, MB>(v);
}

template <int MB>
__global__ __launch_bounds__(256) void ens_products_kernel(const nlam_ens_products_t p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int k = *p.lead;
    if (k >= p.max_lead) return;   // the same in every thread of the grid, ahead of every barrier
    const int M = p.members, F = p.d_state, N = p.nodes, E = p.events, Q = p.quantiles;
    const int s = blockIdx.y, chunk = blockIdx.x;
    const int cn = fc_chunk_nodes(F), tn = prod_tile_nodes(F, M, E, Q), stride = prod_stride(tn, F);
    const int RT = prod_rows(M, Q) - 1;   // the truth's row
    const int n0 = chunk * cn, n1 = min(N, n0 + cn);
    const long per = (long)N * F;
    const bool score = p.truth != nullptr;
    float* const tile = smem;
    int* const cnt = reinterpret_cast<int*>(tile + (RT + 1) * stride);   // [E][tn]: c | o << 8 of a live node, -1 of a dead one
    int* const evar = cnt + E * tn;
    int* const esense = evar + NLAM_ENS_MAX_EVENTS;
    float* const ethr = reinterpret_cast<float*>(esense + NLAM_ENS_MAX_EVENTS);
    int* const qidx = reinterpret_cast<int*>(ethr + NLAM_ENS_MAX_EVENTS);
    float* const qfrac = reinterpret_cast<float*>(qidx + NLAM_ENS_MAX_QUANTILES);
    float* const qlev = qfrac + NLAM_ENS_MAX_QUANTILES;
    for (int i = threadIdx.x; i < E; i += blockDim.x) {
        evar[i] = min(max(p.event_var[i], 0), F - 1);
        esense[i] = p.event_sense[i];
        ethr[i] = p.event_thr[i];
    }
    for (int i = threadIdx.x; i < Q; i += blockDim.x) {
        qidx[i] = min(max(p.q_index[i], 0), M - 1);
        qfrac[i] = p.q_frac[i];
        qlev[i] = p.q_level[i];
    }
    const int W = prod_ws_words(F, M, E, Q), WF = E + Q * F, EB = E * (M + 1);
    float* const ws = p.workspace + ((long)s * gridDim.x + chunk) * W;
    int* const wsi = reinterpret_cast<int*>(ws + WF);
    const float fm = (float)M;
    const long slot = (long)s * p.max_lead + k;
    for (int t0 = n0; t0 < n1; t0 += tn) {
        const int t1 = min(n1, t0 + tn), tnodes = t1 - t0;
        const int cnt_e = tnodes * F, nq = (cnt_e + 3) / 4;
        const long base = (long)t0 * F;
        const bool first = t0 == n0;
        const float* const x0 = p.prev + (long)s * M * per + base;
        const float* const y0 = score ? p.truth + (long)s * M * per + base : x0;
        const bool vec_in = ((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(y0)) & 15) == 0 && (M == 1 || (per & 3) == 0);
        for (int i = threadIdx.x; i < (M + (score ? 1 : 0)) * nq; i += blockDim.x) {   // rows 0 .. M - 1: the members, row RT: the truth
            const int m = i / nq, e = 4 * (i - m * nq);
            const float* const src = m < M ? x0 + (long)m * per : y0;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (vec_in && e + 3 < cnt_e) {
                v = *reinterpret_cast<const f32x4*>(src + e);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (e + c < cnt_e) v[c] = src[e + c];
            }
            *reinterpret_cast<f32x4*>(tile + (m < M ? m : RT) * stride + e) = v;   // e + 3 < stride: tn * F rounded up to a quad
        }
        __syncthreads();   // the tile and, the first time, the tables
        for (int i = threadIdx.x; i < E * tnodes; i += blockDim.x) {   // (event, node), node-minor
            const int ev = i / tnodes, r = i - ev * tnodes;
            const float* const col = tile + r * F + evar[ev];
            const float thr = ethr[ev];
            const bool less = esense[ev] != 0;
            int c = 0;
            for (int m = 0; m < M; ++m) {
                const float v = col[m * stride];
                c += (less ? v < thr : v > thr) ? 1 : 0;
            }
            p.prob[(slot * E + ev) * N + t0 + r] = (float)c / fm;
            if (score) {
                const float y = col[RT * stride];
                const int o = (less ? y < thr : y > thr) ? 1 : 0;
                cnt[ev * tn + r] = p.row_weight[t0 + r] != 0.f ? (c | o << 8) : -1;
            }
        }
        __syncthreads();   // the quantile phase sorts the columns the event phase read
        if (Q > 0) {
            for (int e = threadIdx.x; e < cnt_e; e += blockDim.x) {
                int x[MB];
#pragma unroll
                for (int m = 0; m < MB; ++m) x[m] = m < M ? prod_key(__float_as_int(tile[m * stride + e])) : 0x7fffffff;   // the largest key
                prod_sort<2, MB>(x);
#pragma unroll
                for (int m = 0; m < MB; ++m)
                    if (m < M) tile[m * stride + e] = __int_as_float(prod_key(x[m]));   // this element's column is this thread's alone
                float qv[NLAM_ENS_MAX_QUANTILES];
#pragma unroll
                for (int j = 0; j < NLAM_ENS_MAX_QUANTILES; ++j) {
                    qv[j] = 0.f;
                    if (j < Q) {
                        const int lo = qidx[j], hi = min(lo + 1, M - 1);
                        const float a = tile[lo * stride + e];
                        qv[j] = __fmaf_rn(qfrac[j], tile[hi * stride + e] - a, a);
                    }
                }
#pragma unroll
                for (int j = 0; j < NLAM_ENS_MAX_QUANTILES; ++j)
                    if (j < Q) tile[j * stride + e] = qv[j];
            }
            __syncthreads();
            for (int q = threadIdx.x; q < Q * nq; q += blockDim.x) {   // the Q fields of slot k, physical units
                const int j = q / nq, e = 4 * (q - j * nq);
                float* const dst = p.quant + (slot * Q + j) * per + base;
                const f32x4 v = *reinterpret_cast<const f32x4*>(tile + j * stride + e);
                float vv[4];
                int f = e % F;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    vv[c] = __fmaf_rn(v[c], p.state_std[f], p.state_mean[f]);
                    if (++f == F) f = 0;
                }
                ens_store_quad(dst, e, cnt_e, (reinterpret_cast<uintptr_t>(dst) & 15) == 0, vv);
            }
        }
        if (score) {
            for (int j = threadIdx.x; j < Q * F; j += blockDim.x) {   // j = quantile * F + f: pinball loss and truths below, node order
                const int jq = j / F, f = j - jq * F;
                const float* const col = tile + jq * stride + f;
                const float* const ycol = tile + RT * stride + f;
                const float lev = qlev[jq], vel = 1.f - lev;
                float acc = first ? 0.f : ws[E + j];
                int nb = first ? 0 : wsi[2 * EB + j];
                for (int r = 0; r < tnodes; ++r) {
                    const float qj = col[r * F], y = ycol[r * F], w = p.row_weight[t0 + r];
                    const float rho = y >= qj ? lev * (y - qj) : vel * (qj - y);
                    if (w != 0.f) {
                        acc += w * rho;
                        nb += y < qj ? 1 : 0;
                    }
                }
                ws[E + j] = acc;
                wsi[2 * EB + j] = nb;
            }
            for (int ev = threadIdx.x; ev < E; ev += blockDim.x) {   // the Brier score of the event, node order
                float acc = first ? 0.f : ws[ev];
                for (int r = 0; r < tnodes; ++r) {
                    const int cw = cnt[ev * tn + r];
                    if (cw >= 0) {
                        const float d = (float)(cw & 255) / fm - (float)(cw >> 8);
                        acc += p.row_weight[t0 + r] * (d * d);
                    }
                }
                ws[ev] = acc;
            }
            for (int j = threadIdx.x; j < 2 * EB; j += blockDim.x) {   // j = (table * E + event) * (M + 1) + c: the live nodes with c members in
                const int obs = j >= EB ? 1 : 0, jj = j - obs * EB;
                const int ev = jj / (M + 1), c = jj - ev * (M + 1);
                int t = first ? 0 : wsi[j];
                for (int r = 0; r < tnodes; ++r) {
                    const int cw = cnt[ev * tn + r];
                    t += cw >= 0 && (cw & 255) == c && (cw >> 8) >= obs ? 1 : 0;
                }
                wsi[j] = t;
            }
        }
        __syncthreads();   // the next piece overwrites the tile
    }
}

// blockIdx.y = start, blockIdx.x = 64 words of the workspace row; the four waves split the chunks and meet as in ens_finish_kernel
__global__ __launch_bounds__(256) void ens_products_finish_kernel(const nlam_ens_products_t p, int nchunks) {
    __shared__ float red[4][64];
    const int k = *p.lead;
    if (k >= p.max_lead) return;
    const int M = p.members, F = p.d_state, E = p.events, Q = p.quantiles;
    const int W = prod_ws_words(F, M, E, Q), WF = E + Q * F, EB = E * (M + 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.y, j = blockIdx.x * 64 + lane;
    const bool isf = j < WF;
    const int per = (nchunks + 3) / 4, c0 = wave * per, c1 = min(nchunks, c0 + per);
    float v = 0.f;
    int iv = 0;
    if (j < W) {
        const float* src = p.workspace + (long)s * nchunks * W + j;
#pragma unroll 8
        for (int c = c0; c < c1; ++c) {
            const float t = src[(long)c * W];
            if (isf) v += t;
            else iv += __float_as_int(t);
        }
    }
    red[wave][lane] = isf ? v : __int_as_float(iv);
    __syncthreads();
    if (wave != 0 || j >= W) return;
    const long row = (long)s * p.max_lead + k;
    if (isf) {
        const float t = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        if (j < E) p.brier[row * E + j] = t;
        else p.pinball[row * Q * F + (j - E)] = t;
    } else {
        int t = 0;
        for (int wv = 0; wv < 4; ++wv) t += __float_as_int(red[wv][lane]);
        const int i = j - WF;
        if (i < EB) p.rel_count[row * EB + i] = t;
        else if (i < 2 * EB) p.rel_obs[row * EB + (i - EB)] = t;
        else p.below[row * Q * F + (i - 2 * EB)] = t;
    }
}

// every check before any launch
int32_t ens_products_check(const nlam_ens_products_t* p) {
    if (p == nullptr || p->lead == nullptr) return NLAM_EINVAL;
    if (p->starts < 1 || p->members < 1 || p->nodes < 1 || p->d_state < 1 || p->max_lead < 1) return NLAM_EINVAL;
    const int E = p->events, Q = p->quantiles;
    if (E < 0 || Q < 0 || (E == 0 && Q == 0)) return NLAM_EINVAL;
    if (p->members > NLAM_ENS_MAX_MEMBERS || p->d_state > NLAM_EVAL_MAX_VARS || p->starts > 65535) return NLAM_EUNSUP;
    if (E > NLAM_ENS_MAX_EVENTS || Q > NLAM_ENS_MAX_QUANTILES) return NLAM_EUNSUP;
    if ((long)p->nodes * p->d_state >= (1L << 31)) return NLAM_EUNSUP;
    if (p->prev == nullptr || p->row_weight == nullptr || p->state_mean == nullptr || p->state_std == nullptr || p->workspace == nullptr)
        return NLAM_EINVAL;
    if (E > 0 && (p->event_var == nullptr || p->event_sense == nullptr || p->event_thr == nullptr || p->prob == nullptr)) return NLAM_EINVAL;
    if (Q > 0 && (p->q_index == nullptr || p->q_frac == nullptr || p->q_level == nullptr || p->quant == nullptr)) return NLAM_EINVAL;
    if (p->truth == nullptr) {   // no scores without the truth
        if (p->brier != nullptr || p->rel_count != nullptr || p->rel_obs != nullptr || p->pinball != nullptr || p->below != nullptr)
            return NLAM_EINVAL;
    } else {                     // and with it, every score of what was asked for
        if (E > 0 && (p->brier == nullptr || p->rel_count == nullptr || p->rel_obs == nullptr)) return NLAM_EINVAL;
        if (Q > 0 && (p->pinball == nullptr || p->below == nullptr)) return NLAM_EINVAL;
    }
    if (p->workspace_floats < (long)p->starts * fc_nchunks(p->nodes, p->d_state) * prod_ws_words(p->d_state, p->members, E, Q))
        return NLAM_EINVAL;
    return 0;
}

}  // namespace

extern "C" {

int32_t nlam_ens_products(const nlam_ens_products_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_ens_products");
    if (const int32_t rc = ens_products_check(p)) return rc;
    const int M = p->members, F = p->d_state, E = p->events, Q = p->quantiles;
    const int nchunks = fc_nchunks(p->nodes, F);
    const int tn = prod_tile_nodes(F, M, E, Q);
    const size_t lds = ((size_t)prod_rows(M, Q) * prod_stride(tn, F) + (size_t)E * tn + kProdTabWords) * sizeof(float);
    const dim3 grid(nchunks, p->starts);
    const hipStream_t stream = (hipStream_t)hip_stream;
    const int mb = M <= 4 ? 4 : (M <= 8 ? 8 : (M <= 16 ? 16 : (M <= 32 ? 32 : 64)));
    const int32_t rc = pick<4, 8, 16, 32, 64>(mb, [&](auto v) { return launch<ens_products_kernel<decltype(v)::value>>(grid, dim3(256), lds, stream, *p); });
    if (rc != 0 || p->truth == nullptr) return rc;
    hipLaunchKernelGGL(ens_products_finish_kernel, dim3((prod_ws_words(F, M, E, Q) + 63) / 64, p->starts), dim3(256), 0, stream, *p, nchunks);
    return (int32_t)hipGetLastError();
}

int64_t nlam_ens_products_workspace_floats(int32_t starts, int32_t members, int32_t nodes, int32_t nvars, int32_t events, int32_t quantiles) {
    if (starts < 1 || members < 1 || nodes < 1 || nvars < 1 || events < 0 || quantiles < 0 || (events == 0 && quantiles == 0)) return NLAM_EINVAL;
    if (members > NLAM_ENS_MAX_MEMBERS || nvars > NLAM_EVAL_MAX_VARS || events > NLAM_ENS_MAX_EVENTS || quantiles > NLAM_ENS_MAX_QUANTILES)
        return NLAM_EUNSUP;
    return (int64_t)starts * fc_nchunks(nodes, nvars) * prod_ws_words(nvars, members, events, quantiles);
}

}  // extern "C"
