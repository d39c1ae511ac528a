// nlam_philox_normal_fill / nlam_latent_sample / nlam_ens_scores: sampled ensembles inside the recorded forecast step.
//
// The draw.  A replayed launch cannot be handed new generator state by the host, so the noise is a pure function of what
// the launch reads on the device: Philox4x32-10 (Salmon et al., SC'11; the constants and the round of Random123) with
//   counter = (q, k, m, t0)   q: quad of four consecutive latent elements of the batch item, k = *lead, m = b % members,
//                             t0 = low word of start[b]
//   key     = the 64-bit seed (low word, high word), read through a device pointer
// so the forecast of (seed, start, member) does not depend on the batch it ran in, and a new seed needs no new recording.
// The four words of one block become four normals by two Box-Muller pairs: u = ((x >> 9) + 0.5) * 2^-23 -- an odd integer
// below 2^24 times 2^-24: exact in fp32, never 0 or 1 --, r = sqrtf(-2 logf(u_a)), (sin, cos) = sincospif(2 u_b) (2 u_b is
// exact, 2 pi is never rounded), z = (r cos, r sin).
//
// The scores.  A workgroup of ens_scores_kernel owns (start, chunk of whole nodes: the tail's chunks) and stages the chunk of
// every member and of the truth in LDS, a piece at a time, with 16-byte accesses where every row of the chunk is aligned (DESIGN 4.17's rule), single elements
// otherwise.  One thread then owns one element: its members go from LDS into registers (the kernel is a template on the
// member count rounded up to a power of two), the mean, the unbiased variance, the mean absolute error, the pair sum of
// fair CRPS and the truth's rank are computed in member order, and the weighted terms replace the element's column of the
// tile (only its own thread reads that column).  4 F threads add the terms per variable in node order, F (M + 1) threads
// count the ranks, both into the workspace; ens_finish_kernel adds the chunks in the order of forecast_finish_kernel.  No floating-point atomics:
// two runs give the same bits.  Both kernels only read *lead and do nothing once *lead >= max_lead.
// Included from nlam_hip.hip inside NLAM_IN_TU(1), behind nlam_forecast.inc (softplus_fwd, f32x4, launch<>).

namespace {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct Philox4 {
    uint32_t v[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float philox_uniform(uint32_t x) { return (float)(2u * (x >> 9) + 1u) * 0x1p-24f; }

// the four normals of counter (q, c1, c2, c3) under `seed`
__device__ __forceinline__ void philox_normal4(uint32_t q, uint32_t c1, uint32_t c2, uint32_t c3, uint64_t seed, float z[4]) {
    const Philox4 x = philox4x32_10(q, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float r = sqrtf(-2.f * logf(philox_uniform(x.v[2 * h])));
        float sn, cs;
        sincospif(2.f * philox_uniform(x.v[2 * h + 1]), &sn, &cs);
        z[2 * h] = r * cs;
        z[2 * h + 1] = r * sn;
    }
}

__device__ __forceinline__ void ens_store_quad(float* dst, long e, long count, bool vec, const float v[4]) {
    if (vec && e + 3 < count) {
        *reinterpret_cast<f32x4*>(dst + e) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (e + c < count) dst[e + c] = v[c];
    }
}

__global__ __launch_bounds__(256) void philox_normal_fill_kernel(float* out, long n, uint64_t seed, uint32_t c1, uint32_t c2, uint32_t c3) {
    const long nq = (n + 3) / 4;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        float z[4];
        philox_normal4((uint32_t)q, c1, c2, c3, seed, z);
        ens_store_quad(out, 4 * q, n, vec, z);
    }
}

// blockIdx.y = batch item, blockIdx.x strides over the item's quads
__global__ __launch_bounds__(256) void latent_sample_kernel(const nlam_latent_sample_t p) {
    const int k = *p.lead;
    if (k >= p.max_lead) return;
    const int b = blockIdx.y, D = p.latent_dim;
    const int P = p.diagonal ? 2 * D : D;
    const long per = (long)p.rows * D;
    const float* const params = p.params + (long)b * p.rows * P;
    float* const latent = p.latent + (long)b * per;
    const long slot = ((long)k * p.batch + b) * per;
    const float* const nin = p.noise_in != nullptr ? p.noise_in + slot : nullptr;
    float* const nout = p.noise_out != nullptr ? p.noise_out + slot : nullptr;
    const uint32_t m = (uint32_t)(b % p.members), t0 = (uint32_t)p.start[b];
    const uint64_t seed = nin == nullptr ? *p.seed : 0;
    const bool vec = ((reinterpret_cast<uintptr_t>(latent) | reinterpret_cast<uintptr_t>(nin) | reinterpret_cast<uintptr_t>(nout)) & 15) == 0;
    const long nq = (per + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const long e = 4 * q;
        float z[4] = {0.f, 0.f, 0.f, 0.f}, v[4];
        if (nin != nullptr) {
            if (vec && e + 3 < per) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(nin + e);
                z[0] = x[0]; z[1] = x[1]; z[2] = x[2]; z[3] = x[3];
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (e + c < per) z[c] = nin[e + c];
            }
        } else {
            philox_normal4((uint32_t)q, (uint32_t)k, m, t0, seed, z);
        }
        long row = e / D;
        int col = (int)(e - row * D);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = 0.f;
            if (e + c < per) {
                const float* pr = params + row * P + col;
                v[c] = p.diagonal ? pr[0] + (1e-4f + softplus_fwd(pr[D])) * z[c] : pr[0] + z[c];
            }
            if (++col == D) {
                col = 0;
                ++row;
            }
        }
        ens_store_quad(latent, e, per, vec, v);
        if (nout != nullptr) ens_store_quad(nout, e, per, vec, z);
    }
}

constexpr int kEnsTileFloats = 16384;   // the LDS tile of ens_scores_kernel: rows x tile elements, 64 KiB

// rows of the tile: M members and the truth going in, five terms and the two fields coming out
__host__ __device__ __forceinline__ int ens_rows(int members) { return members + 1 < 7 ? 7 : members + 1; }
// whole nodes per tile: what the LDS budget holds, a multiple of 4 where there are that many (a tile then starts on a 16-byte
// boundary when its chunk does) and never more than the chunk
__host__ __device__ __forceinline__ int ens_tile_nodes(int nvars, int members) {
    int n = kEnsTileFloats / ens_rows(members) / nvars;
    if (n >= 4) n &= ~3;
    const int cn = fc_chunk_nodes(nvars);
    return n < 1 ? 1 : (n > cn ? cn : n);
}
__host__ __device__ __forceinline__ int ens_stride(int nvars, int members) { return (ens_tile_nodes(nvars, members) * nvars + 3) & ~3; }
// words per (start, chunk) of the workspace: four float sums per variable, then the int32 counts of the M + 1 ranks per variable
__host__ __device__ __forceinline__ int ens_ws_words(int nvars, int members) { return nvars * (members + 5); }

// mean of v[0 .. M): v[0] + (sum of the differences from v[0]) / M -- exactly v[0] when the members are equal
template <int MB>
__device__ __forceinline__ float ens_mean(const float (&v)[MB], int M, float fm) {
    float s = 0.f;
#pragma unroll
    for (int m = 1; m < MB; ++m)
        if (m < M) s += v[m] - v[0];
    return v[0] + s / fm;
}

// blockIdx.y = start, blockIdx.x = chunk of fc_chunk_nodes nodes: the chunks of forecast_tail_kernel, and with ens_finish_kernel
// its order of additions per variable (node order inside a chunk, the chunks over four waves, (0 + 1) + (2 + 3)), so that an
// ensemble of identical members gets the bits of the tail's own sums.  A chunk passes through the LDS tile in pieces of
// ens_tile_nodes nodes; the per-variable sums run on in registers from piece to piece.
template <int MB>
__global__ __launch_bounds__(256) void ens_scores_kernel(const nlam_ens_scores_t p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int k = *p.lead;
    if (k >= p.max_lead) return;   // the same in every thread of the grid, ahead of every barrier
    const int M = p.members, F = p.d_state, N = p.nodes;
    const int s = blockIdx.y, chunk = blockIdx.x;
    const int cn = fc_chunk_nodes(F), tn = ens_tile_nodes(F, M), stride = ens_stride(F, M);
    const int n0 = chunk * cn, n1 = min(N, n0 + cn);
    const long per = (long)N * F;
    float* const tile = smem;
    float* const ws = p.workspace + ((long)s * gridDim.x + chunk) * ens_ws_words(F, M);
    int* const wsi = reinterpret_cast<int*>(ws + 4 * F);
    const float fm = (float)M;
    float run[4] = {0.f, 0.f, 0.f, 0.f};   // the sums j = threadIdx.x + 256 i < 4 F of this thread (F <= 256)
    for (int t0 = n0; t0 < n1; t0 += tn) {
        const int t1 = min(n1, t0 + tn);
        const int cnt = (t1 - t0) * F, nq = (cnt + 3) / 4;
        const long base = (long)t0 * F;
        const float* const x0 = p.prev + (long)s * M * per + base;
        const float* const y0 = p.truth + (long)s * M * per + base;
        const long obase = ((long)s * p.max_lead + k) * per + base;
        float* const omean = p.out_mean + obase;
        float* const ospread = p.out_spread + obase;
        const bool vec_in = ((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(y0)) & 15) == 0 && (M == 1 || (per & 3) == 0);
        const bool vec_out = ((reinterpret_cast<uintptr_t>(omean) | reinterpret_cast<uintptr_t>(ospread)) & 15) == 0;
        for (int i = threadIdx.x; i < (M + 1) * nq; i += blockDim.x) {   // rows 0 .. M - 1: the members, row M: the truth
            const int m = i / nq, e = 4 * (i - m * nq);
            const float* const src = m < M ? x0 + (long)m * per : y0;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (vec_in && e + 3 < cnt) {
                v = *reinterpret_cast<const f32x4*>(src + e);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (e + c < cnt) v[c] = src[e + c];
            }
            *reinterpret_cast<f32x4*>(tile + m * stride + e) = v;   // e + 3 < stride: stride is tn * F rounded up to a quad
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
            const int row = e / F, f = e - row * F;
            float x[MB], a[MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) x[m] = m < M ? tile[m * stride + e] : 0.f;
            const float y = tile[M * stride + e];
            const float w = p.row_weight[t0 + row];
            int rank = 0;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                a[m] = fabsf(x[m] - y);
                if (m < M) rank += x[m] < y ? 1 : 0;
            }
            const float xbar = ens_mean<MB>(x, M, fm), ab = ens_mean<MB>(a, M, fm);
            float ss = 0.f, pr = 0.f;
#pragma unroll
            for (int i = 0; i < MB; ++i)
                if (i < M) {
                    const float d = x[i] - xbar;
                    ss += d * d;
#pragma unroll
                    for (int j = 0; j < i; ++j) pr += fabsf(x[i] - x[j]);
                }
            const float var = M > 1 ? ss / (fm - 1.f) : 0.f;
            const float d = xbar - y;
            const bool live = w != 0.f;
            const float sd = p.state_std[f];
            // the column of this element belongs to this thread alone: its inputs are in registers, its terms take their place
            tile[0 * stride + e] = live ? w * (d * d) : 0.f;
            tile[1 * stride + e] = live ? w * var : 0.f;
            tile[2 * stride + e] = live ? w * ab : 0.f;
            tile[3 * stride + e] = live && M > 1 ? w * (pr / (fm * (fm - 1.f))) : 0.f;
            tile[4 * stride + e] = __int_as_float(live ? rank : -1);
            tile[5 * stride + e] = xbar * sd + p.state_mean[f];
            tile[6 * stride + e] = sqrtf(var) * sd;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < 2 * nq; q += blockDim.x) {   // the two fields of slot k, physical units
            const int r = q / nq, e = 4 * (q - r * nq);
            const f32x4 v = *reinterpret_cast<const f32x4*>(tile + (5 + r) * stride + e);
            const float vv[4] = {v[0], v[1], v[2], v[3]};
            ens_store_quad(r == 0 ? omean : ospread, e, cnt, vec_out, vv);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // j = term * F + f: the chunk's sum of variable f, in node order
            const int j = threadIdx.x + 256 * i;
            if (j < 4 * F) {
                const int q = j / F, f = j - q * F;
                const float* col = tile + q * stride + f;
                float v = run[i];
                for (int r = 0; r < t1 - t0; ++r) v += col[r * F];
                run[i] = v;
            }
        }
        for (int j = threadIdx.x; j < F * (M + 1); j += blockDim.x) {   // j = f * (M + 1) + rank: the chunk's nodes of that rank
            const int f = j / (M + 1), rk = j - f * (M + 1);
            const float* col = tile + 4 * stride + f;
            int c = t0 == n0 ? 0 : wsi[j];   // this thread's own word
            for (int r = 0; r < t1 - t0; ++r) c += __float_as_int(col[r * F]) == rk ? 1 : 0;
            wsi[j] = c;
        }
        __syncthreads();   // the next piece overwrites the tile
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = threadIdx.x + 256 * i;
        if (j < 4 * F) ws[j] = run[i];
    }
}

// blockIdx.y = start, blockIdx.x = 64 words of the workspace row; the four waves split the chunks and meet as in forecast_finish_kernel
__global__ __launch_bounds__(256) void ens_finish_kernel(const nlam_ens_scores_t p, int nchunks) {
    __shared__ float red[4][64];
    const int k = *p.lead;
    if (k >= p.max_lead) return;
    const int M = p.members, F = p.d_state, W = ens_ws_words(F, M);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.y, j = blockIdx.x * 64 + lane;
    const bool isf = j < 4 * F;
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
        const int q = j / F, f = j - q * F;
        float* const dst = q == 0 ? p.ens_sq : (q == 1 ? p.ens_var : (q == 2 ? p.ens_abs : p.ens_pair));
        dst[row * F + f] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    } else {
        int t = 0;
        for (int wv = 0; wv < 4; ++wv) t += __float_as_int(red[wv][lane]);
        p.rank_hist[row * F * (M + 1) + (j - 4 * F)] = t;
    }
}

// every check before any launch
int32_t ens_scores_check(const nlam_ens_scores_t* p) {
    if (p == nullptr || p->lead == nullptr) return NLAM_EINVAL;
    if (p->starts < 1 || p->members < 1 || p->nodes < 1 || p->d_state < 1 || p->max_lead < 1) return NLAM_EINVAL;
    if (p->members > NLAM_ENS_MAX_MEMBERS || p->d_state > NLAM_EVAL_MAX_VARS || p->starts > 65535) return NLAM_EUNSUP;
    if ((long)p->nodes * p->d_state >= (1L << 31)) return NLAM_EUNSUP;
    if (p->prev == nullptr || p->truth == nullptr || p->row_weight == nullptr || p->state_mean == nullptr || p->state_std == nullptr ||
        p->ens_sq == nullptr || p->ens_var == nullptr || p->ens_abs == nullptr || p->ens_pair == nullptr || p->rank_hist == nullptr ||
        p->out_mean == nullptr || p->out_spread == nullptr || p->workspace == nullptr)
        return NLAM_EINVAL;
    if (p->workspace_floats < (long)p->starts * fc_nchunks(p->nodes, p->d_state) * ens_ws_words(p->d_state, p->members))
        return NLAM_EINVAL;
    return 0;
}

}  // namespace

extern "C" {

int32_t nlam_philox_normal_fill(float* out, int64_t n, uint64_t seed, uint32_t c1, uint32_t c2, uint32_t c3, void* hip_stream) {
    NLAM_RANGE("nlam_philox_normal_fill");
    if (out == nullptr || n < 0) return NLAM_EINVAL;
    if (n > (1L << 34)) return NLAM_EUNSUP;   // the quad index is one 32-bit word of the counter
    if (n == 0) return 0;
    const long blocks = (n + 1023) / 1024;
    hipLaunchKernelGGL(philox_normal_fill_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, (hipStream_t)hip_stream, out,
                       (long)n, seed, c1, c2, c3);
    return (int32_t)hipGetLastError();
}

int32_t nlam_latent_sample(const nlam_latent_sample_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_latent_sample");
    if (p == nullptr || p->lead == nullptr) return NLAM_EINVAL;
    if (p->batch < 1 || p->members < 1 || p->rows < 1 || p->latent_dim < 1 || p->max_lead < 1 || p->batch % p->members != 0 ||
        (p->diagonal != 0 && p->diagonal != 1))
        return NLAM_EINVAL;
    if (p->batch > 65535 || (long)p->rows * p->latent_dim >= (1L << 31)) return NLAM_EUNSUP;
    if (p->params == nullptr || p->latent == nullptr || p->start == nullptr || (p->noise_in == nullptr && p->seed == nullptr)) return NLAM_EINVAL;
    const long quads = ((long)p->rows * p->latent_dim + 3) / 4;
    const long blocks = (quads + 255) / 256;
    hipLaunchKernelGGL(latent_sample_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), p->batch), dim3(256), 0, (hipStream_t)hip_stream, *p);
    return (int32_t)hipGetLastError();
}

int32_t nlam_ens_scores(const nlam_ens_scores_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_ens_scores");
    if (const int32_t rc = ens_scores_check(p)) return rc;
    const int M = p->members, F = p->d_state;
    const int nchunks = fc_nchunks(p->nodes, F);
    const size_t lds = (size_t)ens_rows(M) * ens_stride(F, M) * sizeof(float);
    const dim3 grid(nchunks, p->starts);
    const hipStream_t stream = (hipStream_t)hip_stream;
    const int mb = M <= 4 ? 4 : (M <= 8 ? 8 : (M <= 16 ? 16 : (M <= 32 ? 32 : 64)));
    const int32_t rc = pick<4, 8, 16, 32, 64>(mb, [&](auto v) { return launch<ens_scores_kernel<decltype(v)::value>>(grid, dim3(256), lds, stream, *p); });
    if (rc != 0) return rc;
    hipLaunchKernelGGL(ens_finish_kernel, dim3((ens_ws_words(F, M) + 63) / 64, p->starts), dim3(256), 0, stream, *p, nchunks);
    return (int32_t)hipGetLastError();
}

int64_t nlam_ens_scores_workspace_floats(int32_t starts, int32_t members, int32_t nodes, int32_t nvars) {
    if (starts < 1 || members < 1 || nodes < 1 || nvars < 1) return NLAM_EINVAL;
    if (members > NLAM_ENS_MAX_MEMBERS || nvars > NLAM_EVAL_MAX_VARS) return NLAM_EUNSUP;
    return (int64_t)starts * fc_nchunks(nodes, nvars) * ens_ws_words(nvars, members);
}

}  // extern "C"
