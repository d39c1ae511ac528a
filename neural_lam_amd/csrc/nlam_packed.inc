// Packing a resident series into int16 codes with a per-feature affine decode (the decode, and every kernel that reads a
// packed series, is in nlam_series.inc, nlam_stats.inc and nlam_forecast.inc).
//
//   encode   q = clamp(rintf(fdiv(fsub(x, offset[f]), scale[f])), -32767, 32767)   round to nearest even, -32768 never written
//   nlam_series_range        per-feature min / max / non-finite count of an fp32 chunk, merged into running tables
//   nlam_series_pack_q16     encode an fp32 chunk into the resident int16 buffer
//   q16_src_check            what every _q16 entry asks of nlam_q16_src_t.  A series whose packed pointer is NULL there is read
//                            as fp32 through the float pointer and float strides of the parameter struct (state packed and
//                            forcing fp32, or the reverse, in one launch).
// Included once from nlam_hip.hip, ahead of those files: range and pack in slice 5, the check in slices 1 and 5.

#if NLAM_IN_TU(1) || NLAM_IN_TU(5)
namespace {

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

}  // extern "C"
#endif
