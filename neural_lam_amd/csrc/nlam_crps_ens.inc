// nlam_latent_draw_fwd / _bwd and nlam_crps_ens_fwd / _bwd: the ensemble CRPS fine-tuning term of the Graph-EFM training schedule
// (Oskarsson et al. 2024, section 3: L_Var + lambda_CRPS L_CRPS) inside the recorded training step.
//
// (a) The draw.  params (batch, rows, P) are the prior's (P = D: mean, std 1; P = 2 D: mean | raw std, std = 1e-4 + softplus):
//   latent = mean + std eps,   eps written for the backward
//   g_params[.., :D] = g,   g_params[.., D:] = g eps softplus'(raw)
// eps is element e % 4 of the Philox counter (e / 4, t, b, low word of *draw) under *seed -- the generator, the Box-Muller pairs
// and the quad layout of latent_kl_fwd_kernel -- or noise_in[b][e].  The caller hands in a key of its own (models.EFMForecasterStep:
// the posterior's key + 0xD1B54A32D192ED03), so the member draws never meet the posterior's (key, counter) pairs.
//
// (b) The term.  pred (batch * members, nodes, nvars), item b * M + m member m of batch item b (the member-minor layout of
// nlam_ens_scores); per element (n, f) of item b, with x_m the members and y the target:
//   v = 1/M sum_m |x_m - y|  -  1/(M (M - 1)) sum_{i<j} |x_i - x_j|        (ens_abs - ens_pair of nlam_ens_scores per element)
//   crps[b] = sum_{n,f} (row_weight[n] var_weight[f]) v,   term = *weight * sum_b crps[b]
// One thread per quad of four consecutive elements of an item; it loads the quad of every member (stride nodes * nvars: each
// load instruction of a wave reads 1 KiB in a row) into registers, sums |x_m - y| over m = 0 .. M - 1 and |x_i - x_j| over
// i = 0 .. M - 2, j = i + 1 .. M - 1 in that order.  The sum: as latent_kl_fwd_kernel -- a thread in element order over its
// grid-stride quads, block_sum_to_partial into workspace[b][block], one finishing workgroup that adds an item's partials in
// block order and the items as thread i <- b = i, i + 256, .. through the same tree.  A zero row weight is a weight like any
// other: no early-out, the order never depends on the data.  No floating-point atomics: two runs give the same bits.
// The backward is elementwise and recomputes from pred and target (saving the signs would cost M bytes per element and a
// second kernel signature; the loads are the ones the forward made).  With g = (*g_term * *weight) (row_weight[n] var_weight[f]):
//   g_pred[b M + m][n][f] = g ( sgn(x_m - y) / M  -  1/(M (M - 1)) sum_{j != m} sgn(x_m - x_j) )
// sgn(a - b) = (a > b) - (a < b): compared, never taken from a rounded difference (a denormal difference flushed to zero
// would turn a strict order into a tie), so a tie gives exactly 0 and the sign sums are small integers.
// Members in registers: the kernels are instantiated on M = 2, 3, 4, 8; every other count up to 16 runs the MT = 16
// instantiation, whose loops are unrolled over 16 members under the uniform test m < members -- the register arrays are only
// ever indexed by constants.  var_weight (ones when NULL) lives in LDS, as the loss kernels keep their per-variable constants.
// Included from nlam_hip.hip inside NLAM_IN_TU(1), behind nlam_latent_kl.inc (lkl_*, latent_kl_blocks, kLatentStdEps).

namespace {

constexpr int kCrpsMaxMembers = NLAM_CRPS_MAX_MEMBERS;

// blockIdx.y = batch item, blockIdx.x strides over the item's quads
__global__ __launch_bounds__(256) void latent_draw_fwd_kernel(const nlam_latent_draw_t p) {
    const int b = blockIdx.y, D = p.latent_dim;
    const int P = p.diagonal ? 2 * D : D;
    const long per = (long)p.rows * D;
    const float* const pp = p.params + (long)b * p.rows * P;
    float* const latent = p.latent + (long)b * per;
    float* const eout = p.eps + (long)b * per;
    const float* const nin = p.noise_in != nullptr ? p.noise_in + (long)b * per : nullptr;
    const uint64_t seed = nin == nullptr ? *p.seed : 0;
    const uint32_t d = nin == nullptr ? (uint32_t)*p.draw : 0u;
    const bool vec = lkl_aligned(latent, eout, nin);
    const bool vecp = (D & 3) == 0 && lkl_aligned(pp);
    const long nq = (per + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const long e = 4 * q;
        float eps[4], mu[4], raw[4], z[4];
        if (nin != nullptr) lkl_load_quad(nin, e, per, vec, eps);
        else philox_normal4((uint32_t)q, (uint32_t)p.t, (uint32_t)b, d, seed, eps);
        lkl_load_params(pp, P, D, p.diagonal != 0, e, per, vecp, mu, raw);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float s = p.diagonal ? kLatentStdEps + softplus_fwd(raw[c]) : 1.f;
            z[c] = mu[c] + s * eps[c];
        }
        ens_store_quad(latent, e, per, vec, z);
        ens_store_quad(eout, e, per, vec, eps);
    }
}

__global__ __launch_bounds__(256) void latent_draw_bwd_kernel(const nlam_latent_draw_t p) {
    const int b = blockIdx.y, D = p.latent_dim;
    const int P = p.diagonal ? 2 * D : D;
    const long per = (long)p.rows * D;
    const float* const pp = p.params + (long)b * p.rows * P;
    const float* const esv = p.eps + (long)b * per;
    const float* const gz = p.g_latent + (long)b * per;
    float* const gpp = p.g_params + (long)b * p.rows * P;
    const bool vec = lkl_aligned(esv, gz);
    const bool vecp = (D & 3) == 0 && lkl_aligned(pp, gpp);
    const long nq = (per + 3) / 4;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const long e = 4 * q;
        float eps[4], g[4], mu[4], raw[4], graw[4];
        lkl_load_quad(esv, e, per, vec, eps);
        lkl_load_quad(gz, e, per, vec, g);
        if (p.diagonal) lkl_load_params(pp, P, D, true, e, per, vecp, mu, raw);
#pragma unroll
        for (int c = 0; c < 4; ++c) graw[c] = p.diagonal ? g[c] * eps[c] * softplus_grad(raw[c]) : 0.f;
        lkl_store_params(gpp, P, D, p.diagonal != 0, e, per, vecp, g, graw);
    }
}

int32_t latent_draw_check(const nlam_latent_draw_t* p) {
    if (p == nullptr) return NLAM_EINVAL;
    if (p->batch < 1 || p->rows < 1 || p->latent_dim < 1 || (p->diagonal != 0 && p->diagonal != 1) || p->t < 0) return NLAM_EINVAL;
    if (p->batch > 65535 || (long)p->rows * p->latent_dim >= (1L << 31)) return NLAM_EUNSUP;
    if (p->params == nullptr || p->eps == nullptr) return NLAM_EINVAL;
    return 0;
}

// the quad of elements e .. e + 3 of one (item, member): zeros past the item's end
__device__ __forceinline__ void crps_load_quad(const float* src, unsigned e, unsigned per, bool vec, float v[4]) {
    if (vec) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(src + e);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = e + c < per ? src[e + c] : 0.f;
    }
}

// row_weight[n] * var_weight[f] of the quad's four elements (0 past the item's end): one division per quad
__device__ __forceinline__ void crps_quad_weights(const float* row_weight, const float* vw, unsigned e, unsigned per, unsigned F,
                                                  float wc[4]) {
    unsigned n = e / F, f = e - n * F;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        wc[c] = e + c < per ? row_weight[n] * vw[f] : 0.f;
        if (++f == F) {
            f = 0;
            ++n;
        }
    }
}

__device__ __forceinline__ void crps_stage_var_weight(const float* var_weight, int F, float* vw) {
    for (int i = threadIdx.x; i < F; i += 256) vw[i] = var_weight != nullptr ? var_weight[i] : 1.f;
    __syncthreads();
}

// MT: the members the loops are unrolled over; GENERIC: p.members <= MT of them are there (else exactly MT)
template <int MT, bool GENERIC>
__global__ __launch_bounds__(256) void crps_ens_fwd_kernel(const nlam_crps_ens_t p) {
    extern __shared__ float crps_vw[];
    crps_stage_var_weight(p.var_weight, p.nvars, crps_vw);
    const int M = GENERIC ? p.members : MT;
    const int b = blockIdx.y;
    const unsigned F = (unsigned)p.nvars, per = (unsigned)p.nodes * F;
    const float* const x0 = p.pred + (long)b * M * per;
    const float* const y0 = p.target + (long)b * per;
    const bool vec_all = (per & 3) == 0 && lkl_aligned(p.pred, p.target);
    const float inv_m = 1.f / (float)M, inv_mm = 1.f / (float)(M * (M - 1));
    const unsigned nq = (per + 3) / 4;
    float acc = 0.f;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < nq; q += gridDim.x * 256u) {
        const unsigned e = 4 * q;
        float x[MT][4], y[4], wc[4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            if (m < M) crps_load_quad(x0 + (long)m * per, e, per, vec_all, x[m]);
        crps_load_quad(y0, e, per, vec_all, y);
        crps_quad_weights(p.row_weight, crps_vw, e, per, F, wc);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float sa = 0.f, sp = 0.f;
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < M) sa += fabsf(x[m][c] - y[c]);
#pragma unroll
            for (int i = 0; i < MT - 1; ++i)
#pragma unroll
                for (int j = i + 1; j < MT; ++j)
                    if (j < M) sp += fabsf(x[i][c] - x[j][c]);
            acc += wc[c] * (sa * inv_m - sp * inv_mm);
        }
    }
    block_sum_to_partial(acc, 1.f, p.workspace + (long)b * gridDim.x);
}

// one workgroup: crps[b] = the item's partials in block order; term = *weight * sum_b crps[b] (the scheme of latent_kl_finish_kernel)
__global__ __launch_bounds__(256) void crps_ens_finish_kernel(const nlam_crps_ens_t p, int nblk) {
    __shared__ float total[1];
    float s = 0.f;
    for (int b = threadIdx.x; b < p.batch; b += 256) {
        const float* ws = p.workspace + (long)b * nblk;
        float v = ws[0];
        for (int i = 1; i < nblk; ++i) v += ws[i];
        p.crps[b] = v;
        s += v;
    }
    block_sum_to_partial(s, 1.f, total);   // blockIdx.x is 0
    __syncthreads();
    if (threadIdx.x == 0) *p.term = *p.weight * total[0];
}

__device__ __forceinline__ int crps_sgn(float a, float b) { return (int)(a > b) - (int)(a < b); }

template <int MT, bool GENERIC>
__global__ __launch_bounds__(256) void crps_ens_bwd_kernel(const nlam_crps_ens_t p) {
    extern __shared__ float crps_vw[];
    crps_stage_var_weight(p.var_weight, p.nvars, crps_vw);
    const int M = GENERIC ? p.members : MT;
    const int b = blockIdx.y;
    const unsigned F = (unsigned)p.nvars, per = (unsigned)p.nodes * F;
    const float* const x0 = p.pred + (long)b * M * per;
    const float* const y0 = p.target + (long)b * per;
    float* const g0 = p.g_pred + (long)b * M * per;
    const bool vec_all = (per & 3) == 0 && lkl_aligned(p.pred, p.target, p.g_pred);
    const float inv_m = 1.f / (float)M, inv_mm = 1.f / (float)(M * (M - 1));
    const float gw = *p.g_term * *p.weight;
    const unsigned nq = (per + 3) / 4;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < nq; q += gridDim.x * 256u) {
        const unsigned e = 4 * q;
        float x[MT][4], y[4], wc[4];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            if (m < M) crps_load_quad(x0 + (long)m * per, e, per, vec_all, x[m]);
        crps_load_quad(y0, e, per, vec_all, y);
        crps_quad_weights(p.row_weight, crps_vw, e, per, F, wc);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < M) {
                float g[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    int pairs = 0;
#pragma unroll
                    for (int j = 0; j < MT; ++j)
                        if (j != m && j < M) pairs += crps_sgn(x[m][c], x[j][c]);
                    g[c] = (gw * wc[c]) * ((float)crps_sgn(x[m][c], y[c]) * inv_m - (float)pairs * inv_mm);
                }
                ens_store_quad(g0 + (long)m * per, e, per, vec_all, g);
            }
        }
    }
}

int32_t crps_ens_check(const nlam_crps_ens_t* p) {
    if (p == nullptr) return NLAM_EINVAL;
    if (p->batch < 1 || p->members < 2 || p->nodes < 1 || p->nvars < 1) return NLAM_EINVAL;
    if (p->members > kCrpsMaxMembers || p->batch > 65535 || p->nvars > NLAM_LOSS_MAX_VARS || (long)p->nodes * p->nvars >= (1L << 31))
        return NLAM_EUNSUP;
    if (p->pred == nullptr || p->target == nullptr || p->row_weight == nullptr || p->weight == nullptr) return NLAM_EINVAL;
    return 0;
}

// f(integral_constant<int, MT>, integral_constant<bool, GENERIC>) for the instantiation that serves `members`
template <typename F>
int32_t crps_pick_members(int members, F&& f) {
    switch (members) {
        case 2: return f(std::integral_constant<int, 2>{}, std::false_type{});
        case 3: return f(std::integral_constant<int, 3>{}, std::false_type{});
        case 4: return f(std::integral_constant<int, 4>{}, std::false_type{});
        case 8: return f(std::integral_constant<int, 8>{}, std::false_type{});
        default: return f(std::integral_constant<int, kCrpsMaxMembers>{}, std::true_type{});
    }
}

}  // namespace

extern "C" {

int32_t nlam_latent_draw_fwd(const nlam_latent_draw_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_latent_draw_fwd");
    if (const int32_t rc = latent_draw_check(p)) return rc;
    if (p->latent == nullptr || (p->noise_in == nullptr && (p->seed == nullptr || p->draw == nullptr))) return NLAM_EINVAL;
    const int nblk = latent_kl_blocks((long)p->rows * p->latent_dim);
    hipLaunchKernelGGL(latent_draw_fwd_kernel, dim3(nblk, p->batch), dim3(256), 0, (hipStream_t)hip_stream, *p);
    return (int32_t)hipGetLastError();
}

int32_t nlam_latent_draw_bwd(const nlam_latent_draw_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_latent_draw_bwd");
    if (const int32_t rc = latent_draw_check(p)) return rc;
    if (p->g_latent == nullptr) return NLAM_EINVAL;
    if (p->g_params == nullptr) return 0;   // a constant prior: nothing to write
    const int nblk = latent_kl_blocks((long)p->rows * p->latent_dim);
    hipLaunchKernelGGL(latent_draw_bwd_kernel, dim3(nblk, p->batch), dim3(256), 0, (hipStream_t)hip_stream, *p);
    return (int32_t)hipGetLastError();
}

int64_t nlam_crps_ens_workspace_floats(int32_t batch, int32_t members, int32_t nodes, int32_t nvars) {
    if (batch < 1 || members < 2 || nodes < 1 || nvars < 1) return NLAM_EINVAL;
    if (members > kCrpsMaxMembers || nvars > NLAM_LOSS_MAX_VARS || (long)nodes * nvars >= (1L << 31)) return NLAM_EUNSUP;
    return (int64_t)batch * latent_kl_blocks((long)nodes * nvars);
}

int32_t nlam_crps_ens_fwd(const nlam_crps_ens_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_crps_ens_fwd");
    if (const int32_t rc = crps_ens_check(p)) return rc;
    if (p->crps == nullptr || p->term == nullptr || p->workspace == nullptr) return NLAM_EINVAL;
    const int nblk = latent_kl_blocks((long)p->nodes * p->nvars);
    if (p->workspace_floats < (int64_t)p->batch * nblk) return NLAM_EINVAL;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const size_t lds = (size_t)p->nvars * sizeof(float);
    const int32_t rc = crps_pick_members(p->members, [&](auto mt, auto generic) {
        hipLaunchKernelGGL((crps_ens_fwd_kernel<mt, generic>), dim3(nblk, p->batch), dim3(256), lds, stream, *p);
        return (int32_t)hipGetLastError();
    });
    if (rc) return rc;
    hipLaunchKernelGGL(crps_ens_finish_kernel, dim3(1), dim3(256), 0, stream, *p, nblk);
    return (int32_t)hipGetLastError();
}

int32_t nlam_crps_ens_bwd(const nlam_crps_ens_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_crps_ens_bwd");
    if (const int32_t rc = crps_ens_check(p)) return rc;
    if (p->g_term == nullptr || p->g_pred == nullptr) return NLAM_EINVAL;
    const int nblk = latent_kl_blocks((long)p->nodes * p->nvars);
    const hipStream_t stream = (hipStream_t)hip_stream;
    const size_t lds = (size_t)p->nvars * sizeof(float);
    return crps_pick_members(p->members, [&](auto mt, auto generic) {
        hipLaunchKernelGGL((crps_ens_bwd_kernel<mt, generic>), dim3(nblk, p->batch), dim3(256), lds, stream, *p);
        return (int32_t)hipGetLastError();
    });
}

}  // extern "C"
