// nlam_latent_kl_fwd / nlam_latent_kl_bwd: the posterior draw and the KL term of the Graph-EFM training objective
// (Oskarsson et al. 2024, section 3) inside the recorded training step.
//
// One pass over (batch, rows, latent_dim).  With u = 1e-4, pq (batch, rows, 2 D) the encoder's parameters and pp
// (batch, rows, P) the prior's (P = D: mean, std 1; P = 2 D: mean | raw std):
//   mu_q = pq[.., :D], s_q = u + softplus(pq[.., D:]);  mu_p, s_p alike from pp
//   z = mu_q + s_q eps
//   term = 1/2 (r^2 + n^2) - 1/2 - log r,  r = s_q / s_p,  n = (mu_q - mu_p) / s_p
// term is log(s_p / s_q) + (s_q^2 + (mu_q - mu_p)^2) / (2 s_p^2) - 1/2 written on the two ratios: with q == p, r is exactly 1
// and n exactly 0, so the term is exactly 0 (the closed form cancels to rounding noise there).
//
// The draw is that of nlam_latent_sample with another counter: Philox4x32-10 under *seed with
//   counter = (q, t, b, d)   q: quad of four consecutive latent elements of the item, t: the AR step (a struct member),
//                            b: the batch item, d: the low word of *draw (a device int64 the kernel only reads)
// so a replay of a recorded step draws new noise once the host's launch in front of it has advanced *draw.  eps goes to
// eps_out: the backward reads it there.  (Redrawing it would need *draw as it was at the forward, which a replayed backward
// cannot know once gradient accumulation or a second forward has advanced it; B R D floats are nothing beside the step.)
//
// The sum.  A workgroup adds the terms of its threads' quads -- each thread in element order over its grid-stride quads, the
// 64 lanes of a wave by the xor tree of block_sum_to_partial, the four waves as (0 + 1) + (2 + 3) -- into workspace[b][block];
// latent_kl_finish_kernel (one workgroup) adds an item's partials in block order into kl[b], then the items: thread i takes
// b = i, i + 256, .. in order, and the 256 sums meet in the same wave tree.  kl_term = *kl_weight * that sum.  No floating-point
// atomics: two runs give the same bits.
// Included from nlam_hip.hip inside NLAM_IN_TU(1), behind nlam_ensemble.inc (philox_normal4, ens_store_quad; softplus_fwd,
// softplus_grad and block_sum_to_partial of the step tails).

namespace {

constexpr int kLatentKlMaxBlocks = 64;   // workgroups (= partial sums) per batch item; beyond 64 * 256 quads the grid strides
constexpr float kLatentStdEps = 1e-4f;   // latent_std_eps

__host__ __device__ __forceinline__ int latent_kl_blocks(long per) {
    const long blocks = ((per + 3) / 4 + 255) / 256;
    return (int)(blocks > kLatentKlMaxBlocks ? kLatentKlMaxBlocks : blocks);
}

__device__ __forceinline__ void lkl_load_quad(const float* src, long e, long count, bool vec, float v[4]) {
    if (vec && e + 3 < count) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(src + e);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = e + c < count ? src[e + c] : 0.f;
    }
}

// the parameters of elements e .. e + 3 of one item: cols [0, D) of the rows of a (rows, ld) matrix, and cols [D, 2 D) with `two`.
// vec (D a multiple of 4, 16-byte aligned rows): the quad lies in one row
__device__ __forceinline__ void lkl_load_params(const float* base, int ld, int D, bool two, long e, long per, bool vec, float mu[4],
                                                float raw[4]) {
    const long row = e / D;
    const int col = (int)(e - row * D);
    if (vec) {
        const float* a = base + row * ld + col;
        const f32x4 x = *reinterpret_cast<const f32x4*>(a);
        mu[0] = x[0]; mu[1] = x[1]; mu[2] = x[2]; mu[3] = x[3];
        if (two) {
            const f32x4 y = *reinterpret_cast<const f32x4*>(a + D);
            raw[0] = y[0]; raw[1] = y[1]; raw[2] = y[2]; raw[3] = y[3];
        }
        return;
    }
    long r = row;
    int c0 = col;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        mu[c] = raw[c] = 0.f;
        if (e + c < per) {
            const float* a = base + r * ld + c0;
            mu[c] = a[0];
            if (two) raw[c] = a[D];
        }
        if (++c0 == D) {
            c0 = 0;
            ++r;
        }
    }
}

// the counterpart of lkl_load_params for the gradients
__device__ __forceinline__ void lkl_store_params(float* base, int ld, int D, bool two, long e, long per, bool vec, const float gmu[4],
                                                 const float graw[4]) {
    const long row = e / D;
    const int col = (int)(e - row * D);
    if (vec) {
        float* a = base + row * ld + col;
        *reinterpret_cast<f32x4*>(a) = f32x4{gmu[0], gmu[1], gmu[2], gmu[3]};
        if (two) *reinterpret_cast<f32x4*>(a + D) = f32x4{graw[0], graw[1], graw[2], graw[3]};
        return;
    }
    long r = row;
    int c0 = col;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (e + c < per) {
            float* a = base + r * ld + c0;
            a[0] = gmu[c];
            if (two) a[D] = graw[c];
        }
        if (++c0 == D) {
            c0 = 0;
            ++r;
        }
    }
}

__device__ __forceinline__ bool lkl_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// blockIdx.y = batch item, blockIdx.x strides over the item's quads
__global__ __launch_bounds__(256) void latent_kl_fwd_kernel(const nlam_latent_kl_t p) {
    const int b = blockIdx.y, D = p.latent_dim;
    const int P = p.diagonal ? 2 * D : D;
    const long per = (long)p.rows * D;
    const float* const pq = p.pq + (long)b * p.rows * 2 * D;
    const float* const pp = p.pp + (long)b * p.rows * P;
    float* const latent = p.latent + (long)b * per;
    float* const eout = p.eps + (long)b * per;
    const float* const nin = p.noise_in != nullptr ? p.noise_in + (long)b * per : nullptr;
    const uint64_t seed = nin == nullptr ? *p.seed : 0;
    const uint32_t d = nin == nullptr ? (uint32_t)*p.draw : 0u;
    const bool vec = lkl_aligned(latent, eout, nin);
    const bool vecp = (D & 3) == 0 && lkl_aligned(pq, pp);
    const long nq = (per + 3) / 4;
    float acc = 0.f;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const long e = 4 * q;
        float eps[4], mq[4], rq[4], mp[4], rp[4], z[4];
        if (nin != nullptr) lkl_load_quad(nin, e, per, vec, eps);
        else philox_normal4((uint32_t)q, (uint32_t)p.t, (uint32_t)b, d, seed, eps);
        lkl_load_params(pq, 2 * D, D, true, e, per, vecp, mq, rq);
        lkl_load_params(pp, P, D, p.diagonal != 0, e, per, vecp, mp, rp);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            z[c] = 0.f;
            if (e + c < per) {
                const float sq = kLatentStdEps + softplus_fwd(rq[c]);
                const float sp = p.diagonal ? kLatentStdEps + softplus_fwd(rp[c]) : 1.f;
                const float r = sq / sp, n = (mq[c] - mp[c]) / sp;
                z[c] = mq[c] + sq * eps[c];
                acc += (0.5f * (r * r + n * n) - 0.5f) - logf(r);
            }
        }
        ens_store_quad(latent, e, per, vec, z);
        ens_store_quad(eout, e, per, vec, eps);
    }
    block_sum_to_partial(acc, 1.f, p.workspace + (long)b * gridDim.x);
}

// one workgroup: kl[b] = the item's partials in block order; kl_term = *kl_weight * sum_b kl[b]
__global__ __launch_bounds__(256) void latent_kl_finish_kernel(const nlam_latent_kl_t p, int nblk) {
    __shared__ float total[1];
    float s = 0.f;
    for (int b = threadIdx.x; b < p.batch; b += 256) {
        const float* ws = p.workspace + (long)b * nblk;
        float v = ws[0];
        for (int i = 1; i < nblk; ++i) v += ws[i];
        p.kl[b] = v;
        s += v;
    }
    block_sum_to_partial(s, 1.f, total);   // blockIdx.x is 0
    __syncthreads();
    if (threadIdx.x == 0) *p.kl_term = *p.kl_weight * total[0];
}

// elementwise: g_pq (always) and g_pp (unless NULL) from the saved pq, pp, eps
__global__ __launch_bounds__(256) void latent_kl_bwd_kernel(const nlam_latent_kl_t p) {
    const int b = blockIdx.y, D = p.latent_dim;
    const int P = p.diagonal ? 2 * D : D;
    const long per = (long)p.rows * D;
    const float* const pq = p.pq + (long)b * p.rows * 2 * D;
    const float* const pp = p.pp + (long)b * p.rows * P;
    const float* const esv = p.eps + (long)b * per;
    const float* const gz = p.g_latent != nullptr ? p.g_latent + (long)b * per : nullptr;
    float* const gpq = p.g_pq + (long)b * p.rows * 2 * D;
    float* const gpp = p.g_pp != nullptr ? p.g_pp + (long)b * p.rows * P : nullptr;
    const float w = *p.g_kl_term * *p.kl_weight;
    const bool vec = lkl_aligned(esv, gz);
    const bool vecp = (D & 3) == 0 && lkl_aligned(pq, pp, gpq, gpp);
    const long nq = (per + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const long e = 4 * q;
        float eps[4], g[4] = {0.f, 0.f, 0.f, 0.f}, mq[4], rq[4], mp[4], rp[4], gmq[4], grq[4], gmp[4], grp[4];
        lkl_load_quad(esv, e, per, vec, eps);
        if (gz != nullptr) lkl_load_quad(gz, e, per, vec, g);
        lkl_load_params(pq, 2 * D, D, true, e, per, vecp, mq, rq);
        lkl_load_params(pp, P, D, p.diagonal != 0, e, per, vecp, mp, rp);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float sq = kLatentStdEps + softplus_fwd(rq[c]);
            const float sp = p.diagonal ? kLatentStdEps + softplus_fwd(rp[c]) : 1.f;
            const float isp = 1.f / sp, dlt = mq[c] - mp[c];
            const float dm = w * dlt * isp * isp;
            gmq[c] = g[c] + dm;
            grq[c] = (g[c] * eps[c] + w * (sq * isp * isp - 1.f / sq)) * softplus_grad(rq[c]);
            gmp[c] = -dm;
            grp[c] = p.diagonal ? w * (isp - (sq * sq + dlt * dlt) * isp * isp * isp) * softplus_grad(rp[c]) : 0.f;
        }
        lkl_store_params(gpq, 2 * D, D, true, e, per, vecp, gmq, grq);
        if (gpp != nullptr) lkl_store_params(gpp, P, D, p.diagonal != 0, e, per, vecp, gmp, grp);
    }
}

// the checks both entry points share, before any launch
int32_t latent_kl_check(const nlam_latent_kl_t* p) {
    if (p == nullptr) return NLAM_EINVAL;
    if (p->batch < 1 || p->rows < 1 || p->latent_dim < 1 || (p->diagonal != 0 && p->diagonal != 1) || p->t < 0) return NLAM_EINVAL;
    if (p->batch > 65535 || (long)p->rows * p->latent_dim >= (1L << 31)) return NLAM_EUNSUP;
    if (p->pq == nullptr || p->pp == nullptr || p->eps == nullptr || p->kl_weight == nullptr) return NLAM_EINVAL;
    return 0;
}

}  // namespace

extern "C" {

int64_t nlam_latent_kl_workspace_floats(int32_t batch, int32_t rows, int32_t latent_dim) {
    if (batch < 1 || rows < 1 || latent_dim < 1) return NLAM_EINVAL;
    return (int64_t)batch * latent_kl_blocks((long)rows * latent_dim);
}

int32_t nlam_latent_kl_fwd(const nlam_latent_kl_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_latent_kl_fwd");
    if (const int32_t rc = latent_kl_check(p)) return rc;
    if (p->latent == nullptr || p->kl == nullptr || p->kl_term == nullptr || p->workspace == nullptr ||
        (p->noise_in == nullptr && (p->seed == nullptr || p->draw == nullptr)))
        return NLAM_EINVAL;
    const int nblk = latent_kl_blocks((long)p->rows * p->latent_dim);
    if (p->workspace_floats < (int64_t)p->batch * nblk) return NLAM_EINVAL;
    const hipStream_t stream = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(latent_kl_fwd_kernel, dim3(nblk, p->batch), dim3(256), 0, stream, *p);
    if (const int32_t rc = (int32_t)hipGetLastError()) return rc;
    hipLaunchKernelGGL(latent_kl_finish_kernel, dim3(1), dim3(256), 0, stream, *p, nblk);
    return (int32_t)hipGetLastError();
}

int32_t nlam_latent_kl_bwd(const nlam_latent_kl_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_latent_kl_bwd");
    if (const int32_t rc = latent_kl_check(p)) return rc;
    if (p->g_kl_term == nullptr || p->g_pq == nullptr) return NLAM_EINVAL;
    const int nblk = latent_kl_blocks((long)p->rows * p->latent_dim);
    hipLaunchKernelGGL(latent_kl_bwd_kernel, dim3(nblk, p->batch), dim3(256), 0, (hipStream_t)hip_stream, *p);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
