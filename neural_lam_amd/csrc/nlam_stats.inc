// nlam_window_moments: per-sample means and second moments of a resident series (the standardization statistics of
// npyfilesmeps/compute_standardization_stats.py), read in place with the strided addressing of nlam_window_batch_ens.
//
// A workgroup owns one output row (a sample, or a (sample, sub-offset) in the difference mode) and a fixed span of its
// (nodes x nvars) block, the same span in every row it reads.  Its lanes take 16-byte quads with a stride of W = 4 * lanes
// elements, lanes a multiple of nvars, so every lane sees the same four features at every stride (eval_partials_kernel's
// layout): the difference mode keeps the previous row's standardized quads in registers and reads every element once.
// Sums are fp64 from the first element: the HBM stream sets the pace (two fp64 adds per fp32 element are far below the
// fp64 vector rate) and a per-sample mean then matches a float64 restatement to ~1e-12 whatever the sample's size or the
// data's offset, where fp32 lanes would lose digits on 70 M-element samples with a large mean.  The lanes' sums meet in
// LDS in a fixed order, the spans' partial sums go to the workspace, and moments_finish_kernel adds them in a fixed order.
// The split depends on nodes and nvars only: a sample's row is bit-identical whichever [first, first + count) covers it.
// nlam_window_moments_q16 is the same kernel over a packed int16 series (Series<int16_t>, mom_load of nlam_series.inc): the
// quads are decoded on load and everything behind the load is shared, so its rows are those of the decoded series.
// Included from nlam_hip.hip inside NLAM_IN_TU(5).

namespace {

constexpr int kMomThreads = 256;
constexpr int kMomQuads = 2;     // quads per lane per row of one chunk (W * kMomQuads elements)
constexpr int kMomSlots = 256;   // workgroups per output row aimed at: whole chunks, at most this many spans

__host__ __device__ __forceinline__ int mom_lanes(int nvars) { return (kMomThreads / nvars) * nvars; }

struct MomSplit {
    long per_row;   // elements of one (nodes x nvars) block
    long span;      // elements per workgroup (whole chunks)
    int nslot;      // workgroups per output row
};

__host__ __device__ inline MomSplit mom_split(int nodes, int nvars) {
    const long per_row = (long)nodes * nvars;
    const long chunk = 4L * mom_lanes(nvars) * kMomQuads;
    const long nchunks = (per_row + chunk - 1) / chunk;
    const long span = ((nchunks + kMomSlots - 1) / kMomSlots) * chunk;
    return MomSplit{per_row, span, (int)((per_row + span - 1) / span)};
}

// workspace[(o * nslot + slot) * 2 * nvars + j]: j < nvars the sum of feature j, then the sums of squares.  T: the element type
// of the series (mom_load): a packed row is decoded with the lane's four (scale, offset) pairs, kept in registers.
template <bool DIFF, typename T>
__global__ __launch_bounds__(kMomThreads) void moments_partials_kernel(const nlam_moments_t p, const Series<T> ser, long n_flat,
                                                                       long span, int nslot) {
    __shared__ double red[2 * 4 * kMomThreads];   // [2][W] the lanes' sums and sums of squares
    __shared__ double seg[2 * kMomThreads];       // [G][2 * nvars] segment sums (G * 2 * nvars <= 512)
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
    const T* base = ser.base + s * p.stride_sample + m * p.stride_member;
    double sum[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid < lanes) {
        float sc[4], of[4];   // the lane's decode pairs; T = float: never set and never read (mom_load<float> ignores them)
        if constexpr (!std::is_same_v<T, float>) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int f = (4 * tid + kk) % F;
                sc[kk] = ser.scale[f];
                of[kk] = ser.offset[f];
            }
        }
        if constexpr (!DIFF) {
            for (long c = e0; c < e1; c += (long)W * kMomQuads) {
#pragma unroll 2
                for (int r = 0; r < p.nrows; ++r) {
                    const T* row = base + (long)(p.row_begin + r) * p.stride_step;
                    const bool vec = (reinterpret_cast<uintptr_t>(row) & kQuadAlign<T>) == 0;
                    f32x4 v[kMomQuads];
#pragma unroll
                    for (int q = 0; q < kMomQuads; ++q) v[q] = mom_load(row, c + (long)q * W + 4 * tid, e1, vec, sc, of);
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
            const int nsub = p.nrows / S;   // rows of one sub-sequence: used / step
            for (long c = e0; c < e1; c += (long)W * kMomQuads) {
                float zp[kMomQuads][4] = {};
#pragma unroll 2
                for (int r = 0; r < nsub; ++r) {
                    const T* row = base + (long)(p.row_begin + k + r * S) * p.stride_step;
                    const bool vec = (reinterpret_cast<uintptr_t>(row) & kQuadAlign<T>) == 0;
                    f32x4 v[kMomQuads];
#pragma unroll
                    for (int q = 0; q < kMomQuads; ++q) v[q] = mom_load(row, c + (long)q * W + 4 * tid, e1, vec, sc, of);
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
    // column j = q * F + f holds the R = W / F entries f, f + F, ...: G segments of them per column, then the segments in order
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

// one output row per workgroup: its nslot partial sums in G fixed segments per column, the segments in order, / count
__global__ __launch_bounds__(kMomThreads) void moments_finish_kernel(const nlam_moments_t p, int nslot, double count) {
    __shared__ double seg[2 * kMomThreads];
    const int F = p.nvars, C2 = 2 * F, G = max(1, kMomThreads / C2), seglen = (nslot + G - 1) / G;
    const long o = blockIdx.x;
    const double* src = p.workspace + o * nslot * C2;
    for (int u = threadIdx.x; u < C2 * G; u += kMomThreads) {
        const int g = u / C2, j = u - g * C2;
        const int c1 = min(nslot, (g + 1) * seglen);
        double v = 0.0;
        for (int c = g * seglen; c < c1; ++c) v += src[(long)c * C2 + j];
        seg[u] = v;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < C2; j += kMomThreads) {
        double v = 0.0;
        for (int g = 0; g < G; ++g) v += seg[g * C2 + j];
        v = v / count;
        if (j < F) p.out_mean[o * F + j] = v;
        else p.out_sq[o * F + (j - F)] = v;
    }
}

// nlam_window_moments and nlam_window_moments_q16: every check, then the partial sums over `ser` and the finish
template <typename T>
int32_t moments_launch(const nlam_moments_t* p, const Series<T>& ser, hipStream_t stream) {
    if (p == nullptr || ser.base == nullptr || p->workspace == nullptr || p->out_mean == nullptr || p->out_sq == nullptr)
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
    const double count = (double)(p->step > 0 ? p->nrows / p->step - 1 : p->nrows) * p->nodes;
    if (p->step > 0)
        hipLaunchKernelGGL((moments_partials_kernel<true, T>), dim3((unsigned)blocks), dim3(kMomThreads), 0, stream, *p, ser,
                           (long)n_flat, sp.span, sp.nslot);
    else
        hipLaunchKernelGGL((moments_partials_kernel<false, T>), dim3((unsigned)blocks), dim3(kMomThreads), 0, stream, *p, ser,
                           (long)n_flat, sp.span, sp.nslot);
    hipLaunchKernelGGL(moments_finish_kernel, dim3((unsigned)n_out), dim3(kMomThreads), 0, stream, *p, sp.nslot, count);
    return (int32_t)hipGetLastError();
}

}  // namespace

extern "C" {

int64_t nlam_moments_workspace_doubles(int32_t nodes, int32_t nvars, int64_t count, int32_t step) {
    if (nodes < 1 || nvars < 1 || nvars > NLAM_MOMENTS_MAX_VARS || count < 1 || step < 0) return NLAM_EINVAL;
    const MomSplit sp = mom_split(nodes, nvars);
    return count * (step > 0 ? step : 1) * sp.nslot * 2L * nvars;
}

int32_t nlam_window_moments(const nlam_moments_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_window_moments");
    return moments_launch(p, Series<float>{p != nullptr ? p->series : nullptr, nullptr, nullptr}, (hipStream_t)hip_stream);
}

int32_t nlam_window_moments_q16(const nlam_moments_t* p, const int16_t* series, const float* scale, const float* offset,
                                void* hip_stream) {
    NLAM_RANGE("nlam_window_moments_q16");
    if (scale == nullptr || offset == nullptr) return NLAM_EINVAL;
    return moments_launch(p, Series<int16_t>{series, scale, offset}, (hipStream_t)hip_stream);
}

}  // extern "C"
