// The resident series as the data kernels read them: one set of row loops over fp32 and packed int16 series, and the window
// batches built on them.
//
// A series is read through Series<T>: T = float as it is, T = int16_t decoded with its per-feature tables,
//   x = fadd(fmul((float)q, scale[f]), offset[f])      two separately rounded fp32 operations
// Standardisation, where asked for, follows on that value (IEEE sub, then div): the two affine maps are never folded, so a
// packed series gives the bits of an fp32 series holding the decoded values.  A quad is one 16-byte load of floats or one
// 8-byte load of codes where the block starts on such a boundary, element by element otherwise (strides are counted in
// elements, so a packed block may start on any 2-byte boundary).
//   series_state_row    one contiguous (nodes x d) block -> fp32
//   series_forcing_row  one (nodes x d_forcing * window) row of windowed forcing: per node (window x d_forcing) -> (d_forcing x
//                       window); the (nodes x d_forcing) block of a window slot comes from a functor
//   mom_load            one quad of a moments row, decoded with the lane's own four (scale, offset) pairs
// The statistics come through a small accessor, so each kernel keeps their source: StatsGlobal (the batch kernels: global
// tables, standardised or not at run time) or StatsLds (the forecast kernels: the float2 table of fc_stage_stats).
// These helpers serve slice 1 (the forecast kernels, nlam_forecast.inc) and slice 5 (the window batches below, the moments of
// nlam_stats.inc); the including #if of nlam_hip.hip names both.

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

template <typename T>
struct Series {
    const T* base;
    const float* scale;    // T = int16_t only
    const float* offset;
};

// The argument struct of a launch over series of element types ST, FT: PACKED -- PLAIN plus the nlam_q16_src_t `q` -- only where
// one of them is packed, so that the float instantiations keep the argument block of an fp32 kernel (a longer block moves the
// implicit arguments a 64-byte line further out, which showed in a 6 us kernel).
template <typename ST, typename FT, typename PLAIN, typename PACKED>
using SeriesArgs = std::conditional_t<std::is_same_v<ST, float> && std::is_same_v<FT, float>, PLAIN, PACKED>;

// the state / forcing series of a launch with argument struct `a`: the packed one of a.q, or the float pointer of the parameters
template <typename T, typename A>
__device__ __forceinline__ Series<T> state_series(const float* f32, const A& a) {
    if constexpr (std::is_same_v<T, float>) return {f32, nullptr, nullptr};
    else return {a.q.state, a.q.state_scale, a.q.state_offset};
}
template <typename T, typename A>
__device__ __forceinline__ Series<T> forcing_series(const float* f32, const A& a) {
    if constexpr (std::is_same_v<T, float>) return {f32, nullptr, nullptr};
    else return {a.q.forcing, a.q.forcing_scale, a.q.forcing_offset};
}

// f(T{}) with T the element type of a series that is packed or not
template <typename F>
int32_t pick_elem(bool packed, F&& f) {
    return packed ? f(int16_t{}) : f(float{});
}

template <typename T>
constexpr size_t kQuadAlign = 4 * sizeof(T) - 1;   // 16 bytes of floats, 8 bytes of codes

// kAhead: series_forcing_row asks for the pair ahead of the element (an LDS read in front of the global load) or behind it (two
// more global loads), as the kernels of each kind always did: with this the fp32 forecast kernels are instruction for instruction
// what they were before the row loops were shared, and the batch kernels within a few scalar instructions of it.
struct StatsGlobal {
    static constexpr bool kAhead = false;
    const float* __restrict__ mean;   // NULL: the values are not standardised
    const float* __restrict__ std;
    __device__ __forceinline__ bool on() const { return mean != nullptr; }
    __device__ __forceinline__ float2 at(unsigned f) const { return make_float2(mean[f], std[f]); }
};

struct StatsLds {
    static constexpr bool kAhead = true;
    const float2* tab;   // (mean, std) per feature
    __device__ __forceinline__ bool on() const { return true; }
    __device__ __forceinline__ float2 at(unsigned f) const { return tab[f]; }
};

template <typename STATS>
__device__ __forceinline__ float standardised(float x, const STATS& st, unsigned f) {
    const float2 ms = st.at(f);
    return __fdiv_rn(__fsub_rn(x, ms.x), ms.y);
}

template <typename T, typename STATS>
__device__ __forceinline__ void series_state_row(const Series<T>& s, const T* __restrict__ src, float* __restrict__ dst, const STATS st,
                                                 unsigned per, unsigned d, unsigned tid, unsigned nthr) {
    const bool stdz = st.on();
    const bool vec = (per & 3u) == 0 && (reinterpret_cast<size_t>(src) & kQuadAlign<T>) == 0 && (reinterpret_cast<size_t>(dst) & 15) == 0;
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
                v[k] = standardised(v[k], st, f);
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

// Four consecutive floats of the output per thread and 32-bit index arithmetic: one division per four elements, the feature /
// window counters advance incrementally (64-bit divisions per element made the first version run at a tenth of the HBM rate).
// Consecutive lanes write consecutive floats; their reads walk `window` contiguous streams.
template <typename T, typename STATS, typename SLOT>
__device__ __forceinline__ void series_forcing_row(const Series<T>& s, float* __restrict__ dst, const STATS st, unsigned nodes,
                                                   unsigned df, unsigned W, unsigned tid, unsigned nthr, SLOT slot) {
    const unsigned fw = df * W;
    const unsigned per_out = nodes * fw;
    const bool stdz = st.on();
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
                float2 ms = {0.f, 1.f};
                if (STATS::kAhead && stdz) ms = st.at(fi);
                if constexpr (std::is_same_v<T, float>) x = slot(w)[(long)n * df + fi];
                else x = q16_decode(slot(w)[(long)n * df + fi], s.scale[fi], s.offset[fi]);
                if (!STATS::kAhead && stdz) ms = st.at(fi);
                if (stdz) x = __fdiv_rn(__fsub_rn(x, ms.x), ms.y);
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

// quad e .. e + 3 of a row (entries at or beyond e1 read as 0, or as code 0, and are not counted by the caller); `vec`: the row
// starts on a quad boundary (kQuadAlign)
template <typename T>
__device__ __forceinline__ f32x4 mom_load(const T* row, long e, long e1, bool vec, const float (&sc)[4], const float (&of)[4]) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (std::is_same_v<T, float>) {
        if (vec && e + 3 < e1) return *reinterpret_cast<const f32x4*>(row + e);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < e1) v[k] = row[e + k];
    } else {
        int16_t c[4] = {0, 0, 0, 0};
        if (vec && e + 3 < e1) {
            q16_load4(row + e, c);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e + k < e1) c[k] = row[e + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = q16_decode(c[k], sc[k], of[k]);
    }
    return v;
}

}  // namespace

#if NLAM_IN_TU(5)
namespace {

// nlam_window_batch: blockIdx.z = sample of the batch, blockIdx.y = row: 0 .. 1 + ar_steps -> one (nodes x d_state) block of
// the state series, then ar_steps rows of windowed forcing.  Every time index is clamped into the series.
__global__ __launch_bounds__(256) void window_batch_kernel(const nlam_window_t p) {
    const int b = blockIdx.z;
    const long i = p.sample_idx[b];
    const int past = p.num_past_forcing_steps, fut = p.num_future_forcing_steps;
    const long last = p.n_times - 1;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
    const int nstate_rows = 2 + p.ar_steps;
    if ((int)blockIdx.y < nstate_rows) {
        const int r = blockIdx.y;
        const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
        const long t = min(max(i + max(0, past - 2) + r, 0L), last);
        float* dst = r < 2 ? p.init_states + ((long)b * 2 + r) * per : p.target_states + ((long)b * p.ar_steps + (r - 2)) * per;
        series_state_row(Series<float>{}, p.state + t * (long)per, dst, StatsGlobal{p.state_mean, p.state_std}, per,
                         (unsigned)p.d_state, tid, nthr);
        if (r == 2 && p.target_times != nullptr && blockIdx.x == 0 && (int)threadIdx.x < p.ar_steps) {
            // without time stamps the (clamped, like the data) time INDEX of every target step is reported
            const long tt = min(max(i + max(2, past) + (long)threadIdx.x, 0L), last);
            p.target_times[(long)b * p.ar_steps + threadIdx.x] = p.times != nullptr ? p.times[tt] : tt;
        }
    } else {
        if (p.d_forcing == 0) return;
        const int step = (int)blockIdx.y - nstate_rows;
        const unsigned W = past + fut + 1, df = p.d_forcing;
        const long per_in = (long)p.nodes * df;
        const long t0 = i + max(2, past) + step - past;   // time of window slot 0
        const unsigned per_out = (unsigned)p.nodes * (df * W);
        float* dst = p.forcing_windowed + ((long)b * p.ar_steps + step) * per_out;
        series_forcing_row(Series<float>{}, dst, StatsGlobal{p.forcing_mean, p.forcing_std}, (unsigned)p.nodes, df, W, tid, nthr,
                           [&](unsigned w) { return p.forcing + min(max(t0 + (long)w, 0L), last) * per_in; });
    }
}

// nlam_window_batch_ens / _q16: window_batch_kernel's launch shape over strided series, each fp32 (ST / FT = float) or packed.
// The flat index is clamped and split into (sample, member) once per workgroup; every (sample, member, step) block is
// contiguous, the window slots stride_step elements apart.  n_flat = base_len * members (computed and checked by the launcher).
struct WindowSeriesArgs {
    nlam_window_ens_t p;
    long n_flat;
};
struct WindowPackedArgs : WindowSeriesArgs {
    nlam_q16_src_t q;
};

template <typename ST, typename FT>
__global__ __launch_bounds__(256) void window_batch_series_kernel(const SeriesArgs<ST, FT, WindowSeriesArgs, WindowPackedArgs> a) {
    const nlam_window_ens_t& p = a.p;
    const int b = blockIdx.z;
    const long idx = min(max(p.sample_idx[b], 0L), a.n_flat - 1);
    const long s = idx / p.members, m = idx - s * p.members;
    const int past = p.num_past_forcing_steps, fut = p.num_future_forcing_steps;
    const int off = max(2, past);
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
    const int nstate_rows = 2 + p.ar_steps;
    if ((int)blockIdx.y < nstate_rows) {
        const int r = blockIdx.y;
        const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
        const long j = max(0, past - 2) + r;
        const Series<ST> ser = state_series<ST>(p.state, a);
        const ST* src = ser.base + s * p.state_stride_sample + j * p.state_stride_step + m * p.state_stride_member;
        float* dst = r < 2 ? p.init_states + ((long)b * 2 + r) * per : p.target_states + ((long)b * p.ar_steps + (r - 2)) * per;
        series_state_row(ser, src, dst, StatsGlobal{p.state_mean, p.state_std}, per, (unsigned)p.d_state, tid, nthr);
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
        const Series<FT> ser = forcing_series<FT>(p.forcing, a);
        const FT* src0 = ser.base + s * p.forcing_stride_sample + (long)(off + step - past) * sw + m * p.forcing_stride_member;
        const unsigned per_out = (unsigned)p.nodes * (df * W);
        float* dst = p.forcing_windowed + ((long)b * p.ar_steps + step) * per_out;
        series_forcing_row(ser, dst, StatsGlobal{p.forcing_mean, p.forcing_std}, (unsigned)p.nodes, df, W, tid, nthr,
                           [&](unsigned w) { return src0 + (long)w * sw; });
    }
}

// one row of a window launch (blockIdx.y): four elements per thread, two rounds; 32-bit offsets inside a row
int32_t window_grid(int batch, int nodes, int d_state, int d_forcing, int ar_steps, long window, dim3* grid) {
    const long e_state = (long)nodes * d_state;
    const long e_forc = (long)nodes * d_forcing * window;
    if (e_state >= (1L << 31) || e_forc >= (1L << 31) || batch > 65535) return NLAM_EUNSUP;
    long blocks = ((e_state > e_forc ? e_state : e_forc) + 2047) / 2048;
    if (blocks < 1) blocks = 1;
    if (blocks > 512) blocks = 512;
    *grid = dim3((int)blocks, 2 + ar_steps + (d_forcing > 0 ? ar_steps : 0), batch);
    return 0;
}

// nlam_window_batch_ens and nlam_window_batch_q16: every check, then the instantiation of the two element types.  `src` names
// the packed series; one without any reads both through the float pointers of `p`.
int32_t window_series_launch(const nlam_window_ens_t* p, const nlam_q16_src_t* src, hipStream_t stream) {
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
    if (p->state_mean != nullptr && p->d_forcing > 0 && p->forcing_mean == nullptr) return NLAM_EINVAL;   // all or nothing, as the reference's hook
    const int32_t past = p->num_past_forcing_steps, fut = p->num_future_forcing_steps;
    const int64_t off = past > 2 ? past : 2;
    int64_t base_len;
    if (p->is_forecast) {
        if ((p->times == nullptr) != (p->elapsed == nullptr)) return NLAM_EINVAL;   // a valid time needs both stamps
        if (p->state_steps < off + p->ar_steps) return NLAM_EINVAL;                 // lead-time axis too short (weather_dataset.py:147-160)
        if (p->d_forcing > 0 && p->forcing_steps < off + p->ar_steps + fut) return NLAM_EINVAL;   // (:162-180)
        base_len = p->n_times;
    } else {
        if (p->elapsed != nullptr) return NLAM_EINVAL;
        base_len = nlam_window_len(p->n_times, p->d_forcing > 0 ? p->n_times : -1, p->ar_steps, past, fut);
        if (base_len < 1) return NLAM_EINVAL;   // the series is shorter than one sample
    }
    if (p->batch == 0 || p->nodes == 0) return 0;
    dim3 grid;
    if (const int32_t rc = window_grid(p->batch, p->nodes, p->d_state, p->d_forcing, p->ar_steps, (long)past + fut + 1, &grid)) return rc;
    WindowPackedArgs a;
    a.p = *p;
    a.n_flat = (long)(base_len * p->members);
    a.q = *src;
    return pick_elem(src->state != nullptr, [&](auto st) {
        return pick_elem(p->d_forcing > 0 && src->forcing != nullptr, [&](auto ft) {
            using A = SeriesArgs<decltype(st), decltype(ft), WindowSeriesArgs, WindowPackedArgs>;
            return launch<window_batch_series_kernel<decltype(st), decltype(ft)>>(grid, dim3(256), 0, stream, static_cast<const A&>(a));
        });
    });
}

}  // namespace

extern "C" {

int64_t nlam_window_len(int64_t n_state_times, int64_t n_forcing_times, int32_t ar_steps, int32_t past, int32_t future) {
    const int64_t window = (int64_t)(past > 2 ? past : 2) + ar_steps + future;
    int64_t n = n_state_times - window + 1;
    if (n_forcing_times >= 0 && n_forcing_times - window + 1 < n) n = n_forcing_times - window + 1;
    return n > 0 ? n : 0;
}

int32_t nlam_window_batch(const nlam_window_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_window_batch");
    if (p == nullptr || p->state == nullptr || p->sample_idx == nullptr || p->init_states == nullptr || p->target_states == nullptr)
        return NLAM_EINVAL;
    if (p->batch < 0 || p->nodes < 0 || p->d_state < 1 || p->d_forcing < 0 || p->ar_steps < 1 || p->ar_steps > 256 ||
        p->num_past_forcing_steps < 0 || p->num_future_forcing_steps < 0 || p->n_times < 1)
        return NLAM_EINVAL;
    if (p->d_forcing > 0 && (p->forcing == nullptr || p->forcing_windowed == nullptr)) return NLAM_EINVAL;
    if ((p->state_mean == nullptr) != (p->state_std == nullptr) || (p->forcing_mean == nullptr) != (p->forcing_std == nullptr)) return NLAM_EINVAL;
    if (p->state_mean != nullptr && p->d_forcing > 0 && p->forcing_mean == nullptr) return NLAM_EINVAL;   // all or nothing, as the reference's hook
    if (nlam_window_len(p->n_times, p->d_forcing > 0 ? p->n_times : -1, p->ar_steps, p->num_past_forcing_steps, p->num_future_forcing_steps) < 1)
        return NLAM_EINVAL;   // the series is shorter than one sample
    if (p->batch == 0 || p->nodes == 0) return 0;
    dim3 grid;
    if (const int32_t rc = window_grid(p->batch, p->nodes, p->d_state, p->d_forcing, p->ar_steps,
                                       (long)p->num_past_forcing_steps + p->num_future_forcing_steps + 1, &grid))
        return rc;
    hipLaunchKernelGGL(window_batch_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, *p);
    return (int32_t)hipGetLastError();
}

int32_t nlam_window_batch_ens(const nlam_window_ens_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_window_batch_ens");
    const nlam_q16_src_t fp32 = {};   // no packed series
    return window_series_launch(p, &fp32, (hipStream_t)hip_stream);
}

int32_t nlam_window_batch_q16(const nlam_window_ens_t* p, const nlam_q16_src_t* src, void* hip_stream) {
    NLAM_RANGE("nlam_window_batch_q16");
    return window_series_launch(p, src, (hipStream_t)hip_stream);
}

}  // extern "C"
#endif
