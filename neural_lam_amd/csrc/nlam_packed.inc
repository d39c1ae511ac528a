// Packed int16 resident series: the data kernels over series kept as 16-bit codes with a per-feature affine decode.
//
//   decode   x = fadd(fmul((float)q, scale[f]), offset[f])                       two separately rounded fp32 operations
//   encode   q = clamp(rintf(fdiv(fsub(x, offset[f]), scale[f])), -32767, 32767)   round to nearest even, -32768 never written
// Standardisation, where asked for, follows on the decoded value as in the fp32 kernels (IEEE sub, then div): the two affine
// maps are never folded, so a packed series gives the bits of an fp32 series holding the decoded values.
//   nlam_series_range        per-feature min / max / non-finite count of an fp32 chunk, merged into running tables
//   nlam_series_pack_q16     encode an fp32 chunk into the resident int16 buffer
//   nlam_window_batch_q16    window_batch_ens_kernel's launch shape and row loops; a packed block is read 4 codes (8 bytes) per
//                            lane where the block starts on an 8-byte boundary, code by code otherwise (strides are counted in
//                            int16 elements, so a block may start on any 2-byte boundary)
//   nlam_window_moments_q16  moments_partials_kernel's split, lanes and fp64 sums over decoded quads; moments_finish_kernel as it is
//   nlam_forecast_init_q16 / nlam_forecast_head_q16   the strided init / head pair over packed series
// A series whose packed pointer is NULL in nlam_q16_src_t is read as fp32 through the float pointer and float strides of the
// parameter struct (state packed and forcing fp32, or the reverse, in one launch).
// Included once from nlam_hip.hip: the row loops are shared by slice 5 (range, pack, batch, moments: beside nlam_stats.inc)
// and slice 1 (the forecast pair: beside nlam_forecast.inc, whose checks and sample arithmetic it uses).

#if NLAM_IN_TU(1) || NLAM_IN_TU(5)
namespace {

// The product is rounded before the sum.  Plain operators under contract(off), as adamw_ctl_one: __fmul_rn / __fadd_rn are
// header functions that multiply and add under the translation unit's own contraction mode, so after inlining the compiler
// fuses the pair into one fma (measured: the batches then differ from the numpy decode in the last bit).
__device__ __forceinline__ float q16_decode(int16_t q, float scale, float offset) {
#pragma clang fp contract(off)
    const float prod = (float)q * scale;
    return prod + offset;
}

// four consecutive codes of an 8-byte aligned address
__device__ __forceinline__ void q16_load4(const int16_t* src, int16_t (&q)[4]) {
    const uint2 w = *reinterpret_cast<const uint2*>(src);
    q[0] = (int16_t)(w.x & 0xffffu);
    q[1] = (int16_t)(w.x >> 16);
    q[2] = (int16_t)(w.y & 0xffffu);
    q[3] = (int16_t)(w.y >> 16);
}

// One series of a _q16 launch: T = int16_t (packed, decoded with the tables) or float (read as it is).
template <typename T>
struct Q16Series {
    const T* base;
    const float* scale;
    const float* offset;
};

template <typename T>
__device__ __forceinline__ float q16_value(const Q16Series<T>& s, const T* at, unsigned f) {
    if constexpr (std::is_same_v<T, float>) return *at;
    else return q16_decode(*at, s.scale[f], s.offset[f]);
}

// one contiguous (nodes x d) block of a state series -> fp32, optionally standardised: window_batch_ens_kernel's state rows
template <typename T>
__device__ __forceinline__ void q16_state_row(const Q16Series<T>& s, const T* __restrict__ src, float* __restrict__ dst,
                                              const float* __restrict__ mean, const float* __restrict__ std, unsigned per, unsigned d,
                                              unsigned tid, unsigned nthr) {
    constexpr size_t kSrcAlign = 4 * sizeof(T) - 1;   // 16 bytes of floats, 8 bytes of codes
    const bool stdz = mean != nullptr;
    const bool vec = (per & 3u) == 0 && (reinterpret_cast<size_t>(src) & kSrcAlign) == 0 && (reinterpret_cast<size_t>(dst) & 15) == 0;
    for (unsigned q = tid; q < (per + 3) / 4; q += nthr) {
        const unsigned e0 = 4 * q;
        float v[4];
        if constexpr (std::is_same_v<T, float>) {
            if (vec) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(src + e0);
                v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = e0 + k < per ? src[e0 + k] : 0.f;
            }
        } else {
            int16_t c[4] = {0, 0, 0, 0};
            if (vec) {
                q16_load4(src + e0, c);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e0 + k < per) c[k] = src[e0 + k];
            }
            unsigned f = e0 % d;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = q16_decode(c[k], s.scale[f], s.offset[f]);
                f = f + 1 == d ? 0 : f + 1;
            }
        }
        if (stdz) {
            unsigned f = e0 % d;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = __fdiv_rn(__fsub_rn(v[k], mean[f]), std[f]);
                f = f + 1 == d ? 0 : f + 1;
            }
        }
        if (vec) {
            *reinterpret_cast<f32x4*>(dst + e0) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < per) dst[e0 + k] = v[k];
        }
    }
}

// one (nodes x d_forcing * window) row of windowed forcing: window_batch_ens_kernel's per-node (window x d_forcing) ->
// (d_forcing x window) transpose.  slot(w) is the (nodes x d_forcing) block that window slot w reads.
template <typename T, typename SLOT>
__device__ __forceinline__ void q16_forcing_row(const Q16Series<T>& s, float* __restrict__ dst, const float* __restrict__ mean,
                                                const float* __restrict__ std, unsigned nodes, unsigned df, unsigned W, unsigned tid,
                                                unsigned nthr, SLOT slot) {
    const unsigned fw = df * W;
    const unsigned per_out = nodes * fw;
    const bool stdz = mean != nullptr;
    const bool vec = (per_out & 3u) == 0 && (reinterpret_cast<size_t>(dst) & 15) == 0;
    for (unsigned q = tid; q < (per_out + 3) / 4; q += nthr) {
        const unsigned e0 = 4 * q;
        unsigned n = e0 / fw;
        unsigned jj = e0 - n * fw;
        unsigned fi = jj / W, w = jj - fi * W;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float x = 0.f;
            if (e0 + k < per_out) {
                x = q16_value(s, slot(w) + ((long)n * df + fi), fi);
                if (stdz) x = __fdiv_rn(__fsub_rn(x, mean[fi]), std[fi]);
            }
            v[k] = x;
            if (++w == W) {
                w = 0;
                if (++fi == df) {
                    fi = 0;
                    ++n;
                }
            }
        }
        if (vec) {
            *reinterpret_cast<f32x4*>(dst + e0) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < per_out) dst[e0 + k] = v[k];
        }
    }
}

// the checks every _q16 entry shares: the state is read from somewhere, and a packed series comes with both of its tables
int32_t q16_src_check(const nlam_q16_src_t* c, const float* state_f32, const float* forcing_f32, int d_forcing) {
    if (c == nullptr) return NLAM_EINVAL;
    if (c->state == nullptr && state_f32 == nullptr) return NLAM_EINVAL;
    if (c->state != nullptr && (c->state_scale == nullptr || c->state_offset == nullptr)) return NLAM_EINVAL;
    if (d_forcing > 0) {
        if (c->forcing == nullptr && forcing_f32 == nullptr) return NLAM_EINVAL;
        if (c->forcing != nullptr && (c->forcing_scale == nullptr || c->forcing_offset == nullptr)) return NLAM_EINVAL;
    }
    return 0;
}

}  // namespace
#endif

#if NLAM_IN_TU(5)
namespace {

// ---- nlam_series_range ----
// A workgroup owns a span of whole strides of W = 4 * lanes elements, lanes a multiple of nvars, so a lane's four elements keep
// their features (moments_partials_kernel's layout): min, max and the count of non-finite values stay in registers, meet in LDS,
// and the nvars columns of the workgroup go to the workspace.  series_range_finish_kernel folds the workgroups into the running
// tables.  min and max are exact and order-independent; non-finite values are counted and take no part in them.
constexpr int kRngThreads = 256;
constexpr int kRngMaxBlocks = 1024;

__host__ __device__ __forceinline__ int rng_lanes(int nvars) { return (kRngThreads / nvars) * nvars; }

struct RngSplit {
    long span;     // elements per workgroup (whole strides)
    int nblocks;
};

inline RngSplit rng_split(long n, int nvars) {
    const long W = 4L * rng_lanes(nvars);
    const long nstrides = (n + W - 1) / W;
    const long span = ((nstrides + kRngMaxBlocks - 1) / kRngMaxBlocks) * W;
    return RngSplit{span, (int)((n + span - 1) / span)};
}

// ws[(block * 3 + 0) * F + f] the bits of the minimum, + 1 of the maximum, + 2 the non-finite count
__global__ __launch_bounds__(kRngThreads) void series_range_partials_kernel(const float* __restrict__ x, long n, int F, long span,
                                                                            uint32_t* __restrict__ ws) {
    __shared__ float smin[4 * kRngThreads];
    __shared__ float smax[4 * kRngThreads];
    __shared__ uint32_t sbad[4 * kRngThreads];
    const int lanes = rng_lanes(F), W = 4 * lanes;
    const int tid = threadIdx.x;
    const long e0 = blockIdx.x * span, e1 = min(n, e0 + span);
    const float inf = __builtin_huge_valf();
    float mn[4] = {inf, inf, inf, inf}, mx[4] = {-inf, -inf, -inf, -inf};
    uint32_t bad[4] = {0u, 0u, 0u, 0u};
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    if (tid < lanes) {
        for (long e = e0 + 4 * tid; e < e1; e += W) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (vec && e + 3 < e1) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(x + e);
                v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < e1) v[k] = x[e + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e + k < e1) {
                    if (isfinite(v[k])) {
                        mn[k] = fminf(mn[k], v[k]);
                        mx[k] = fmaxf(mx[k], v[k]);
                    } else {
                        ++bad[k];
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            smin[4 * tid + k] = mn[k];
            smax[4 * tid + k] = mx[k];
            sbad[4 * tid + k] = bad[k];
        }
    }
    __syncthreads();
    uint32_t* out = ws + (long)blockIdx.x * 3 * F;
    for (int f = tid; f < F; f += kRngThreads) {   // entries f, f + F, ... of the W the lanes left
        float a = inf, b = -inf;
        uint32_t c = 0u;
        for (int i = f; i < W; i += F) {
            a = fminf(a, smin[i]);
            b = fmaxf(b, smax[i]);
            c += sbad[i];
        }
        out[f] = __float_as_uint(a);
        out[F + f] = __float_as_uint(b);
        out[2 * F + f] = c;
    }
}

__global__ __launch_bounds__(kRngThreads) void series_range_finish_kernel(const uint32_t* __restrict__ ws, int nblocks, int F,
                                                                          float* run_min, float* run_max, int64_t* run_bad) {
    for (int f = threadIdx.x; f < F; f += kRngThreads) {
        float a = run_min[f], b = run_max[f];
        int64_t c = run_bad[f];
        for (int k = 0; k < nblocks; ++k) {
            const uint32_t* src = ws + (long)k * 3 * F;
            a = fminf(a, __uint_as_float(src[f]));
            b = fmaxf(b, __uint_as_float(src[F + f]));
            c += src[2 * F + f];
        }
        run_min[f] = a;
        run_max[f] = b;
        run_bad[f] = c;
    }
}

// ---- nlam_series_pack_q16 ----
__device__ __forceinline__ int16_t q16_encode(float x, float scale, float offset) {
    const float r = rintf(__fdiv_rn(__fsub_rn(x, offset), scale));
    return (int16_t)(int)fminf(fmaxf(r, -32767.f), 32767.f);
}

// four consecutive elements per thread: a 16-byte load and one 8-byte store where the chunk and the destination allow it
__global__ __launch_bounds__(256) void series_pack_q16_kernel(const float* __restrict__ x, unsigned n, unsigned F,
                                                              const float* __restrict__ scale, const float* __restrict__ offset,
                                                              int16_t* __restrict__ dst) {
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
    const bool vin = (reinterpret_cast<uintptr_t>(x) & 15) == 0, vout = (reinterpret_cast<uintptr_t>(dst) & 7) == 0;
    for (unsigned q = tid; q < (n + 3) / 4; q += nthr) {
        const unsigned e0 = 4 * q;
        const bool full = e0 + 3 < n;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (vin && full) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(x + e0);
            v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < n) v[k] = x[e0 + k];
        }
        unsigned f = e0 % F;
        int16_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] = q16_encode(v[k], scale[f], offset[f]);
            f = f + 1 == F ? 0 : f + 1;
        }
        if (vout && full) {
            uint2 w;
            w.x = (uint32_t)(uint16_t)c[0] | ((uint32_t)(uint16_t)c[1] << 16);
            w.y = (uint32_t)(uint16_t)c[2] | ((uint32_t)(uint16_t)c[3] << 16);
            *reinterpret_cast<uint2*>(dst + e0) = w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < n) dst[e0 + k] = c[k];
        }
    }
}

// ---- nlam_window_batch_q16 ----
// window_batch_ens_kernel over packed series: the same grid (blockIdx.z = batch item, blockIdx.y = row), the same clamp and split
// of the flat index, the same rows and target times.  SQ / FQ: the state / the forcing is packed.
template <bool SQ, bool FQ>
__global__ __launch_bounds__(256) void window_batch_q16_kernel(const nlam_window_ens_t p, const nlam_q16_src_t c, long n_flat) {
    using ST = std::conditional_t<SQ, int16_t, float>;
    using FT = std::conditional_t<FQ, int16_t, float>;
    const int b = blockIdx.z;
    const long idx = min(max(p.sample_idx[b], 0L), n_flat - 1);
    const long s = idx / p.members, m = idx - s * p.members;
    const int past = p.num_past_forcing_steps, fut = p.num_future_forcing_steps;
    const int off = max(2, past);
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
    const int nstate_rows = 2 + p.ar_steps;
    if ((int)blockIdx.y < nstate_rows) {
        const int r = blockIdx.y;
        const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
        const long j = max(0, past - 2) + r;
        Q16Series<ST> ser;
        if constexpr (SQ) ser = {c.state, c.state_scale, c.state_offset};
        else ser = {p.state, nullptr, nullptr};
        const ST* src = ser.base + s * p.state_stride_sample + j * p.state_stride_step + m * p.state_stride_member;
        float* dst = r < 2 ? p.init_states + ((long)b * 2 + r) * per : p.target_states + ((long)b * p.ar_steps + (r - 2)) * per;
        q16_state_row(ser, src, dst, p.state_mean, p.state_std, per, (unsigned)p.d_state, tid, nthr);
        if (r == 2 && p.target_times != nullptr && blockIdx.x == 0 && (int)threadIdx.x < p.ar_steps) {
            const long jt = off + (long)threadIdx.x;
            long tt;
            if (p.is_forecast) tt = p.times != nullptr ? p.times[s] + p.elapsed[jt] : jt;   // lead-time index without stamps
            else tt = p.times != nullptr ? p.times[s + jt] : s + jt;                        // time index without stamps
            p.target_times[(long)b * p.ar_steps + threadIdx.x] = tt;
        }
    } else {
        if (p.d_forcing == 0) return;
        const int step = (int)blockIdx.y - nstate_rows;
        const unsigned W = past + fut + 1, df = p.d_forcing;
        const long sw = p.forcing_stride_step;   // elements between window slots
        Q16Series<FT> ser;
        if constexpr (FQ) ser = {c.forcing, c.forcing_scale, c.forcing_offset};
        else ser = {p.forcing, nullptr, nullptr};
        const FT* src0 = ser.base + s * p.forcing_stride_sample + (long)(off + step - past) * sw + m * p.forcing_stride_member;
        float* dst = p.forcing_windowed + ((long)b * p.ar_steps + step) * ((long)p.nodes * df * W);
        q16_forcing_row(ser, dst, p.forcing_mean, p.forcing_std, (unsigned)p.nodes, df, W, tid, nthr,
                        [&](unsigned w) { return src0 + (long)w * sw; });
    }
}

// ---- nlam_window_moments_q16 ----
// quad e .. e + 3 of a packed row, decoded with the lane's four (scale, offset) pairs (entries at or beyond e1 read as code 0 and
// are not counted by the caller)
__device__ __forceinline__ f32x4 mom_load_q16(const int16_t* row, long e, long e1, bool vec, const float (&sc)[4], const float (&of)[4]) {
    int16_t c[4] = {0, 0, 0, 0};
    if (vec && e + 3 < e1) {
        q16_load4(row + e, c);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < e1) c[k] = row[e + k];
    }
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = q16_decode(c[k], sc[k], of[k]);
    return v;
}

// moments_partials_kernel with the rows read through mom_load_q16: the same split, lanes, order of the fp64 sums and workspace
template <bool DIFF>
__global__ __launch_bounds__(kMomThreads) void moments_partials_q16_kernel(const nlam_moments_t p, const int16_t* __restrict__ series,
                                                                           const float* __restrict__ scale,
                                                                           const float* __restrict__ offset, long n_flat, long span,
                                                                           int nslot) {
    __shared__ double red[2 * 4 * kMomThreads];
    __shared__ double seg[2 * kMomThreads];
    const int F = p.nvars;
    const int lanes = mom_lanes(F), W = 4 * lanes;
    const int S = DIFF ? p.step : 1;
    const long o = blockIdx.x / nslot;
    const int slot = (int)(blockIdx.x - o * nslot);
    const long i = o / S;
    const int k = (int)(o - i * S);
    const long idx = min(max(p.first + i, 0L), n_flat - 1);
    const long s = idx / p.members, m = idx - s * p.members;
    const long per_row = (long)p.nodes * F;
    const long e0 = slot * span, e1 = min(per_row, e0 + span);
    const int tid = threadIdx.x;
    const int16_t* base = series + s * p.stride_sample + m * p.stride_member;
    double sum[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid < lanes) {
        float sc[4], of[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int f = (4 * tid + kk) % F;
            sc[kk] = scale[f];
            of[kk] = offset[f];
        }
        if constexpr (!DIFF) {
            for (long c = e0; c < e1; c += (long)W * kMomQuads) {
#pragma unroll 2
                for (int r = 0; r < p.nrows; ++r) {
                    const int16_t* row = base + (long)(p.row_begin + r) * p.stride_step;
                    const bool vec = (reinterpret_cast<uintptr_t>(row) & 7) == 0;
                    f32x4 v[kMomQuads];
#pragma unroll
                    for (int q = 0; q < kMomQuads; ++q) v[q] = mom_load_q16(row, c + (long)q * W + 4 * tid, e1, vec, sc, of);
#pragma unroll
                    for (int q = 0; q < kMomQuads; ++q) {
                        const long e = c + (long)q * W + 4 * tid;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
                            if (e + kk < e1) {
                                const double x = (double)v[q][kk];
                                sum[kk] += x;
                                sq[kk] = fma(x, x, sq[kk]);
                            }
                        }
                    }
                }
            }
        } else {
            float mu[4], sd[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int f = (4 * tid + kk) % F;
                mu[kk] = p.mean[f];
                sd[kk] = p.std[f];
            }
            const int nsub = p.nrows / S;
            for (long c = e0; c < e1; c += (long)W * kMomQuads) {
                float zp[kMomQuads][4] = {};
#pragma unroll 2
                for (int r = 0; r < nsub; ++r) {
                    const int16_t* row = base + (long)(p.row_begin + k + r * S) * p.stride_step;
                    const bool vec = (reinterpret_cast<uintptr_t>(row) & 7) == 0;
                    f32x4 v[kMomQuads];
#pragma unroll
                    for (int q = 0; q < kMomQuads; ++q) v[q] = mom_load_q16(row, c + (long)q * W + 4 * tid, e1, vec, sc, of);
#pragma unroll
                    for (int q = 0; q < kMomQuads; ++q) {
                        const long e = c + (long)q * W + 4 * tid;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
                            const float z = __fdiv_rn(__fsub_rn(v[q][kk], mu[kk]), sd[kk]);
                            if (r > 0 && e + kk < e1) {
                                const double x = (double)__fsub_rn(z, zp[q][kk]);
                                sum[kk] += x;
                                sq[kk] = fma(x, x, sq[kk]);
                            }
                            zp[q][kk] = z;
                        }
                    }
                }
            }
        }
    }
    if (tid < lanes) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            red[4 * tid + kk] = sum[kk];
            red[W + 4 * tid + kk] = sq[kk];
        }
    }
    __syncthreads();
    const int C2 = 2 * F, R = W / F, G = max(1, kMomThreads / C2), seglen = (R + G - 1) / G;
    for (int u = tid; u < C2 * G; u += kMomThreads) {
        const int g = u / C2, j = u - g * C2, q = j / F, f = j - q * F;
        const int r1 = min(R, (g + 1) * seglen);
        double v = 0.0;
        for (int r = g * seglen; r < r1; ++r) v += red[q * W + f + r * F];
        seg[u] = v;
    }
    __syncthreads();
    double* out = p.workspace + (long)blockIdx.x * C2;
    for (int j = tid; j < C2; j += kMomThreads) {
        double v = 0.0;
        for (int g = 0; g < G; ++g) v += seg[g * C2 + j];
        out[j] = v;
    }
}

}  // namespace

extern "C" {

int64_t nlam_series_range_workspace_words(int64_t rows, int32_t nvars) {
    if (rows < 1 || nvars < 1) return NLAM_EINVAL;
    if (nvars > NLAM_MOMENTS_MAX_VARS) return NLAM_EUNSUP;
    const int64_t W = 4L * rng_lanes(nvars);
    if (rows > ((1L << 62) / nvars)) return NLAM_EUNSUP;
    const int64_t nstrides = (rows * nvars + W - 1) / W;
    return (nstrides < kRngMaxBlocks ? nstrides : kRngMaxBlocks) * 3 * nvars;   // an upper bound of the split, monotone in rows
}

int32_t nlam_series_range(const float* x, int64_t rows, int32_t nvars, float* run_min, float* run_max, int64_t* run_bad,
                          uint32_t* workspace, int64_t workspace_words, void* hip_stream) {
    NLAM_RANGE("nlam_series_range");
    if (x == nullptr || run_min == nullptr || run_max == nullptr || run_bad == nullptr || workspace == nullptr) return NLAM_EINVAL;
    if (rows < 1 || nvars < 1) return NLAM_EINVAL;
    if (nvars > NLAM_MOMENTS_MAX_VARS || rows > ((1L << 62) / nvars)) return NLAM_EUNSUP;
    const long n = (long)rows * nvars;
    const RngSplit sp = rng_split(n, nvars);
    if (workspace_words < (int64_t)sp.nblocks * 3 * nvars) return NLAM_EINVAL;
    const hipStream_t stream = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(series_range_partials_kernel, dim3((unsigned)sp.nblocks), dim3(kRngThreads), 0, stream, x, n, (int)nvars, sp.span,
                       workspace);
    hipLaunchKernelGGL(series_range_finish_kernel, dim3(1), dim3(kRngThreads), 0, stream, (const uint32_t*)workspace, sp.nblocks,
                       (int)nvars, run_min, run_max, run_bad);
    return (int32_t)hipGetLastError();
}

int32_t nlam_series_pack_q16(const float* x, int64_t rows, int32_t nvars, const float* scale, const float* offset, int16_t* dst,
                             int64_t dst_offset, void* hip_stream) {
    NLAM_RANGE("nlam_series_pack_q16");
    if (x == nullptr || scale == nullptr || offset == nullptr || dst == nullptr) return NLAM_EINVAL;
    if (rows < 1 || nvars < 1 || dst_offset < 0) return NLAM_EINVAL;
    if (rows > ((1L << 31) - 4) / nvars) return NLAM_EUNSUP;   // 32-bit offsets inside a chunk
    const long n = (long)rows * nvars;
    long blocks = (n + 2047) / 2048;   // four elements per thread, two rounds
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(series_pack_q16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, x, (unsigned)n,
                       (unsigned)nvars, scale, offset, dst + dst_offset);
    return (int32_t)hipGetLastError();
}

int32_t nlam_window_batch_q16(const nlam_window_ens_t* p, const nlam_q16_src_t* src, void* hip_stream) {
    NLAM_RANGE("nlam_window_batch_q16");
    if (p == nullptr || src == nullptr || p->sample_idx == nullptr || p->init_states == nullptr || p->target_states == nullptr)
        return NLAM_EINVAL;
    if (p->batch < 0 || p->nodes < 0 || p->d_state < 1 || p->d_forcing < 0 || p->ar_steps < 1 || p->ar_steps > 256 ||
        p->num_past_forcing_steps < 0 || p->num_future_forcing_steps < 0 || p->n_times < 1 || p->members < 1 ||
        (p->is_forecast != 0 && p->is_forecast != 1))
        return NLAM_EINVAL;
    if (p->state_stride_sample < 0 || p->state_stride_step < 0 || p->state_stride_member < 0 || p->forcing_stride_sample < 0 ||
        p->forcing_stride_step < 0 || p->forcing_stride_member < 0)
        return NLAM_EINVAL;
    if (const int32_t rc = q16_src_check(src, p->state, p->forcing, p->d_forcing)) return rc;
    if (p->d_forcing > 0 && p->forcing_windowed == nullptr) return NLAM_EINVAL;
    if ((p->state_mean == nullptr) != (p->state_std == nullptr) || (p->forcing_mean == nullptr) != (p->forcing_std == nullptr)) return NLAM_EINVAL;
    if (p->state_mean != nullptr && p->d_forcing > 0 && p->forcing_mean == nullptr) return NLAM_EINVAL;   // all or nothing
    const int32_t past = p->num_past_forcing_steps, fut = p->num_future_forcing_steps;
    const int64_t off = past > 2 ? past : 2;
    int64_t base_len;
    if (p->is_forecast) {
        if ((p->times == nullptr) != (p->elapsed == nullptr)) return NLAM_EINVAL;
        if (p->state_steps < off + p->ar_steps) return NLAM_EINVAL;                                // lead-time axis too short
        if (p->d_forcing > 0 && p->forcing_steps < off + p->ar_steps + fut) return NLAM_EINVAL;
        base_len = p->n_times;
    } else {
        if (p->elapsed != nullptr) return NLAM_EINVAL;
        base_len = nlam_window_len(p->n_times, p->d_forcing > 0 ? p->n_times : -1, p->ar_steps, past, fut);
        if (base_len < 1) return NLAM_EINVAL;   // the series is shorter than one sample
    }
    if (p->batch == 0 || p->nodes == 0) return 0;
    const long window = past + fut + 1;
    const long e_state = (long)p->nodes * p->d_state;
    const long e_forc = (long)p->nodes * p->d_forcing * window;
    if (e_state >= (1L << 31) || e_forc >= (1L << 31) || p->batch > 65535) return NLAM_EUNSUP;   // 32-bit offsets inside a row
    long blocks = ((e_state > e_forc ? e_state : e_forc) + 2047) / 2048;
    if (blocks < 1) blocks = 1;
    if (blocks > 512) blocks = 512;
    const int rows = 2 + p->ar_steps + (p->d_forcing > 0 ? p->ar_steps : 0);
    const dim3 grid((int)blocks, rows, p->batch);
    const long n_flat = (long)(base_len * p->members);
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool sq = src->state != nullptr, fq = p->d_forcing > 0 && src->forcing != nullptr;
    if (sq && fq) hipLaunchKernelGGL((window_batch_q16_kernel<true, true>), grid, dim3(256), 0, stream, *p, *src, n_flat);
    else if (sq) hipLaunchKernelGGL((window_batch_q16_kernel<true, false>), grid, dim3(256), 0, stream, *p, *src, n_flat);
    else if (fq) hipLaunchKernelGGL((window_batch_q16_kernel<false, true>), grid, dim3(256), 0, stream, *p, *src, n_flat);
    else hipLaunchKernelGGL((window_batch_q16_kernel<false, false>), grid, dim3(256), 0, stream, *p, *src, n_flat);
    return (int32_t)hipGetLastError();
}

int32_t nlam_window_moments_q16(const nlam_moments_t* p, const int16_t* series, const float* scale, const float* offset,
                                void* hip_stream) {
    NLAM_RANGE("nlam_window_moments_q16");
    if (p == nullptr || series == nullptr || scale == nullptr || offset == nullptr || p->workspace == nullptr ||
        p->out_mean == nullptr || p->out_sq == nullptr)
        return NLAM_EINVAL;
    if (p->nodes < 1 || p->nvars < 1 || p->members < 1 || p->n_times < 1 || p->nrows < 1 || p->row_begin < 0 || p->step < 0 ||
        p->first < 0 || p->count < 1 || (p->is_forecast != 0 && p->is_forecast != 1))
        return NLAM_EINVAL;
    if (p->stride_sample < 0 || p->stride_step < 0 || p->stride_member < 0) return NLAM_EINVAL;
    if (p->nvars > NLAM_MOMENTS_MAX_VARS) return NLAM_EUNSUP;
    if (p->step > 0) {
        if (p->mean == nullptr || p->std == nullptr || p->nrows / p->step < 2) return NLAM_EINVAL;   // at least one pair
    } else if (p->mean != nullptr || p->std != nullptr) {
        return NLAM_EINVAL;
    }
    const int64_t window = (int64_t)p->row_begin + p->nrows;
    int64_t base_len;
    if (p->is_forecast) {
        if (p->steps < window) return NLAM_EINVAL;   // the lead-time axis is shorter than a sample
        base_len = p->n_times;
    } else {
        base_len = p->n_times - window + 1;
        if (base_len < 1) return NLAM_EINVAL;        // the series is shorter than one sample
    }
    const int64_t n_flat = base_len * p->members;
    if (p->count > n_flat || p->first > n_flat - p->count) return NLAM_EINVAL;
    const MomSplit sp = mom_split(p->nodes, p->nvars);
    if (sp.per_row >= (1L << 31)) return NLAM_EUNSUP;
    const int64_t S = p->step > 0 ? p->step : 1;
    const int64_t n_out = p->count * S;
    const int64_t blocks = n_out * sp.nslot;
    if (n_out > 0x7fffffffL || blocks > 0x7fffffffL) return NLAM_EUNSUP;
    if (p->workspace_doubles < blocks * 2L * p->nvars) return NLAM_EINVAL;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const double count = (double)(p->step > 0 ? p->nrows / p->step - 1 : p->nrows) * p->nodes;
    if (p->step > 0)
        hipLaunchKernelGGL(moments_partials_q16_kernel<true>, dim3((unsigned)blocks), dim3(kMomThreads), 0, stream, *p, series, scale,
                           offset, (long)n_flat, sp.span, sp.nslot);
    else
        hipLaunchKernelGGL(moments_partials_q16_kernel<false>, dim3((unsigned)blocks), dim3(kMomThreads), 0, stream, *p, series, scale,
                           offset, (long)n_flat, sp.span, sp.nslot);
    hipLaunchKernelGGL(moments_finish_kernel, dim3((unsigned)n_out), dim3(kMomThreads), 0, stream, *p, sp.nslot, count);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
#endif

#if NLAM_IN_TU(1)
namespace {

// ---- nlam_forecast_init_q16 / nlam_forecast_head_q16 ----
// the contiguous (nodes x d) block of row j of (sample, member): fc_src_block's clamps, on a series of either element type
template <typename T>
__device__ __forceinline__ const T* fc_q16_block(const T* base, long stride_sample, long stride_step, long stride_member,
                                                 const nlam_forecast_src_t& c, int steps, FcSample i, long j) {
    if (c.is_forecast) return base + i.s * stride_sample + fc_clamp_time(j, steps - 1) * stride_step + i.m * stride_member;
    return base + fc_clamp_time(i.s + j, c.n_times - 1) * stride_step + i.m * stride_member;
}

struct ForecastQ16Args {
    ForecastSrcArgs a;
    nlam_q16_src_t q;
};

// forecast_init_strided_kernel over packed series: rows off - 2 and off - 1 of the sample
template <bool SQ>
__global__ __launch_bounds__(256) void forecast_init_q16_kernel(const ForecastQ16Args g) {
    using ST = std::conditional_t<SQ, int16_t, float>;
    const nlam_forecast_t& p = g.a.p;
    const nlam_forecast_src_t& c = g.a.s;
    const int b = blockIdx.z, r = blockIdx.y;
    const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
    const long j = max(2, p.num_past_forcing_steps) - 2 + r;
    Q16Series<ST> ser;
    if constexpr (SQ) ser = {g.q.state, g.q.state_scale, g.q.state_offset};
    else ser = {c.state, nullptr, nullptr};
    const ST* src = fc_q16_block(ser.base, c.state_stride_sample, c.state_stride_step, c.state_stride_member, c, c.state_steps,
                                 fc_sample(g.a, b), j);
    q16_state_row(ser, src, (r == 0 ? p.prev_prev : p.prev) + (long)b * per, p.state_mean, p.state_std, per, (unsigned)p.d_state,
                  blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    if (blockIdx.x == 0 && r == 0 && b == 0 && threadIdx.x == 0) *p.lead = 0;
}

// forecast_head_strided_kernel over packed series: the truth is row off + k, window slot w of the forcing row off + k - past + w
template <bool SQ, bool FQ>
__global__ __launch_bounds__(256) void forecast_head_q16_kernel(const ForecastQ16Args g) {
    using ST = std::conditional_t<SQ, int16_t, float>;
    using FT = std::conditional_t<FQ, int16_t, float>;
    const nlam_forecast_t& p = g.a.p;
    const nlam_forecast_src_t& c = g.a.s;
    const int k = *p.lead;
    if (k >= p.max_lead) return;   // the same in every thread of the grid
    const bool forc = blockIdx.y == 1;
    const int b = blockIdx.z;
    const FcSample i = fc_sample(g.a, b);
    const int past = p.num_past_forcing_steps;
    const long jv = max(2, past) + k;   // the row of this lead
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
    if (!forc) {
        const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
        Q16Series<ST> ser;
        if constexpr (SQ) ser = {g.q.state, g.q.state_scale, g.q.state_offset};
        else ser = {c.state, nullptr, nullptr};
        const ST* src = fc_q16_block(ser.base, c.state_stride_sample, c.state_stride_step, c.state_stride_member, c, c.state_steps, i, jv);
        q16_state_row(ser, src, p.truth + (long)b * per, p.state_mean, p.state_std, per, (unsigned)p.d_state, tid, nthr);
        return;
    }
    const unsigned W = past + p.num_future_forcing_steps + 1, df = p.d_forcing;
    Q16Series<FT> ser;
    if constexpr (FQ) ser = {g.q.forcing, g.q.forcing_scale, g.q.forcing_offset};
    else ser = {c.forcing, nullptr, nullptr};
    q16_forcing_row(ser, p.forcing_windowed + (long)b * p.nodes * (df * W), p.forcing_mean, p.forcing_std, (unsigned)p.nodes, df, W, tid,
                    nthr, [&](unsigned w) {
                        return fc_q16_block(ser.base, c.forcing_stride_sample, c.forcing_stride_step, c.forcing_stride_member, c,
                                            c.forcing_steps, i, jv - past + (long)w);
                    });
}

// forecast_src_check with the packed source in place of the float series: a packed series stands in for the float pointer the
// shared checks ask for (no kernel of the pair reads it through that pointer)
int32_t forecast_q16_check(const nlam_forecast_t* p, const nlam_forecast_src_t* s, const nlam_q16_src_t* q, int which,
                           ForecastQ16Args* g) {
    if (p == nullptr || s == nullptr || q == nullptr) return NLAM_EINVAL;
    if (const int32_t rc = q16_src_check(q, s->state, s->forcing, p->d_forcing)) return rc;
    nlam_forecast_src_t s2 = *s;
    if (q->state != nullptr) s2.state = reinterpret_cast<const float*>(q->state);
    if (p->d_forcing > 0 && q->forcing != nullptr) s2.forcing = reinterpret_cast<const float*>(q->forcing);
    if (const int32_t rc = forecast_src_check(p, &s2, which, &g->a)) return rc;
    g->a.s = *s;
    g->q = *q;
    return 0;
}

}  // namespace

extern "C" {

int32_t nlam_forecast_init_q16(const nlam_forecast_t* p, const nlam_forecast_src_t* src, const nlam_q16_src_t* packed,
                               void* hip_stream) {
    NLAM_RANGE("nlam_forecast_init_q16");
    ForecastQ16Args g;
    if (const int32_t rc = forecast_q16_check(p, src, packed, kFcInit, &g)) return rc;
    const dim3 grid(fc_row_blocks((long)p->nodes * p->d_state), 2, p->batch);
    const hipStream_t stream = (hipStream_t)hip_stream;
    if (packed->state != nullptr) hipLaunchKernelGGL(forecast_init_q16_kernel<true>, grid, dim3(256), 0, stream, g);
    else hipLaunchKernelGGL(forecast_init_q16_kernel<false>, grid, dim3(256), 0, stream, g);
    return (int32_t)hipGetLastError();
}

int32_t nlam_forecast_head_q16(const nlam_forecast_t* p, const nlam_forecast_src_t* src, const nlam_q16_src_t* packed,
                               void* hip_stream) {
    NLAM_RANGE("nlam_forecast_head_q16");
    ForecastQ16Args g;
    if (const int32_t rc = forecast_q16_check(p, src, packed, kFcHead, &g)) return rc;
    const long window = (long)p->num_past_forcing_steps + p->num_future_forcing_steps + 1;
    const long e_state = (long)p->nodes * p->d_state, e_forc = (long)p->nodes * p->d_forcing * window;
    const dim3 grid(fc_row_blocks(e_state > e_forc ? e_state : e_forc), p->d_forcing > 0 ? 2 : 1, p->batch);
    const hipStream_t stream = (hipStream_t)hip_stream;
    const bool sq = packed->state != nullptr, fq = p->d_forcing > 0 && packed->forcing != nullptr;
    if (sq && fq) hipLaunchKernelGGL((forecast_head_q16_kernel<true, true>), grid, dim3(256), 0, stream, g);
    else if (sq) hipLaunchKernelGGL((forecast_head_q16_kernel<true, false>), grid, dim3(256), 0, stream, g);
    else if (fq) hipLaunchKernelGGL((forecast_head_q16_kernel<false, true>), grid, dim3(256), 0, stream, g);
    else hipLaunchKernelGGL((forecast_head_q16_kernel<false, false>), grid, dim3(256), 0, stream, g);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
#endif
