// nlam_forecast_init / _head / _tail / _finish: a forecast of any length as replays of ONE recorded AR step.
//
// A captured launch keeps its pointers, so what depends on the lead time is addressed on the device: `start` holds each
// forecast's time index t0, `lead` the number k of lead times already produced.  Per replay
//   head    this lead's standardised forcing window and boundary truth, cut from the resident series (the row loops of
//           nlam_series.inc, which window_batch_kernel runs too: the same bits)
//   (the network, recorded between the two)
//   tail    one pass per element: step_tail_pred -- the function of step_tail_ext_fwd_kernel, so the new state has the bits of
//           nlam_step_tail_ext_fwd(target = NULL) --, the in-place rotation prev_prev <- prev <- new, slot k of the physical
//           outputs, the valid time, and (VERIFY) the workgroup's per-variable sums of w * d^2 and w * |d|
//   finish  one workgroup: the partial sums in a fixed order into sq / ab [b][k][f], then ++*lead.  ONE thread reads the counter
//           and writes it; head and tail only read it, so no launch races with its own readers.
// All three do nothing once *lead >= max_lead: a replay too many writes nothing.
// nlam_forecast_init_strided / _head_strided are init and head over forecast-type and ensemble series: the same row loops, the
// (sample, member, row) block found with nlam_window_ens_t's strides from a flat sample index read on the device.
// nlam_forecast_init_q16 / _head_q16 launch the same two kernel templates with int16_t for every packed series (the strided
// entries launch the float instantiations); all of them stage (mean, std) in LDS.
// HBM-bound: a workgroup of the tail owns (batch item, chunk of whole nodes), a multiple of 4 nodes, so a chunk starts on a
// 16-byte boundary whenever its batch item does; 16-byte accesses where every operand of the chunk is aligned (DESIGN 4.17's
// rule), single elements otherwise and on a chunk's last partial quad.  The per-variable tables -- StepTailTables plus (std, mean)
// of the state -- are staged in LDS once per workgroup.  Included from nlam_hip.hip inside NLAM_IN_TU(1).

namespace {

constexpr int kFcChunkElems = 4096;   // elements per workgroup of the tail (whole nodes, a multiple of 4 of them)

__host__ __device__ __forceinline__ int fc_chunk_nodes(int nvars) {
    const int n = ((kFcChunkElems / nvars + 3) / 4) * 4;
    return n < 4 ? 4 : n;
}
__host__ __device__ __forceinline__ int fc_nchunks(int nodes, int nvars) { return (nodes + fc_chunk_nodes(nvars) - 1) / fc_chunk_nodes(nvars); }
// floats of StepTailTables in front of the forecast tail's own tables (28 bytes per variable, rounded to 16 bytes)
__host__ __device__ __forceinline__ int fc_tab_floats(int nvars) { return (7 * nvars + 3) & ~3; }

struct ForecastTailArgs {
    StepTailExtArgs t;   // dstd, dmean, clamp_lo, clamp_hi, nvars and the mode bits: what StepTailTables stages
    nlam_forecast_t p;
};

__device__ __forceinline__ long fc_clamp_time(long t, long last) { return min(max(t, 0L), last); }

// (mean, std) of `d` variables into LDS
__device__ __forceinline__ const float2* fc_stage_stats(const float* mean, const float* std, int d) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* const tab = reinterpret_cast<float2*>(smem);
    for (int v = threadIdx.x; v < d; v += blockDim.x) tab[v] = make_float2(mean[v], std[v]);
    __syncthreads();
    return tab;
}

// The strided source of nlam_forecast_init_strided / _head_strided: nlam_window_ens_t's addressing.  The flat sample index is
// read on the device, clamped into [0, n_flat) and split into (sample, member) once per workgroup.
struct ForecastSrcArgs {
    nlam_forecast_t p;
    nlam_forecast_src_t s;
    long n_flat;   // base_len * members at ar_steps = max_lead (computed and checked by the entry point)
};

struct FcSample {
    long s, m;
};

__device__ __forceinline__ FcSample fc_sample(const ForecastSrcArgs& a, int b) {
    const long idx = min(max(a.s.sample_idx[b], 0L), a.n_flat - 1);
    const long s = idx / a.s.members;
    return FcSample{s, idx - s * a.s.members};
}

// the contiguous (nodes x d) block of row j of (sample, member): forecast data clamps the lead-time row into [0, steps), analysis
// data the time index s + j into [0, n_times) (there stride_sample == stride_step)
template <typename T>
__device__ __forceinline__ const T* fc_src_block(const T* base, long stride_sample, long stride_step, long stride_member,
                                                 const nlam_forecast_src_t& c, int steps, FcSample i, long j) {
    if (c.is_forecast) return base + i.s * stride_sample + fc_clamp_time(j, steps - 1) * stride_step + i.m * stride_member;
    return base + fc_clamp_time(i.s + j, c.n_times - 1) * stride_step + i.m * stride_member;
}

// a strided source with a packed series (nlam_forecast_init_q16 / _head_q16): the instantiations that decode take this one
struct ForecastPackedArgs : ForecastSrcArgs {
    nlam_q16_src_t q;
};

// blockIdx.z = forecast of the batch, blockIdx.y = 0: prev_prev (time t0 - 1), 1: prev (time t0); the counter starts at 0
__global__ __launch_bounds__(256) void forecast_init_kernel(const nlam_forecast_t p) {
    const StatsLds stats{fc_stage_stats(p.state_mean, p.state_std, p.d_state)};
    const int b = blockIdx.z, r = blockIdx.y;
    const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
    const long t = fc_clamp_time(p.start[b] - 1 + r, p.n_times - 1);
    series_state_row(Series<float>{}, p.state + t * (long)per, (r == 0 ? p.prev_prev : p.prev) + (long)b * per, stats, per,
                     (unsigned)p.d_state, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    if (blockIdx.x == 0 && r == 0 && b == 0 && threadIdx.x == 0) *p.lead = 0;
}

// blockIdx.z = forecast of the batch, blockIdx.y = 0: the boundary truth (state at t0 + k + 1), 1: the forcing window of that time
__global__ __launch_bounds__(256) void forecast_head_kernel(const nlam_forecast_t p) {
    const int k = *p.lead;
    if (k >= p.max_lead) return;   // the same in every thread of the grid, ahead of every barrier
    const bool forc = blockIdx.y == 1;
    const StatsLds stats{forc ? fc_stage_stats(p.forcing_mean, p.forcing_std, p.d_forcing)
                              : fc_stage_stats(p.state_mean, p.state_std, p.d_state)};
    const int b = blockIdx.z;
    const long last = p.n_times - 1;
    const long tv = p.start[b] + k + 1;   // the valid time of this lead
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
    if (!forc) {
        const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
        series_state_row(Series<float>{}, p.state + fc_clamp_time(tv, last) * (long)per, p.truth + (long)b * per, stats, per,
                         (unsigned)p.d_state, tid, nthr);
        return;
    }
    const int past = p.num_past_forcing_steps;
    const unsigned W = past + p.num_future_forcing_steps + 1, df = p.d_forcing;
    const long per_in = (long)p.nodes * df;
    const long t0 = tv - past;   // time of window slot 0
    series_forcing_row(Series<float>{}, p.forcing_windowed + (long)b * p.nodes * (df * W), stats, (unsigned)p.nodes, df, W, tid, nthr,
                       [&](unsigned w) { return p.forcing + fc_clamp_time(t0 + (long)w, last) * per_in; });
}

// forecast_init_kernel over a strided source, fp32 (ST = float) or packed: rows off - 2 and off - 1 of the sample
template <typename ST>
__global__ __launch_bounds__(256) void forecast_init_strided_kernel(const SeriesArgs<ST, float, ForecastSrcArgs, ForecastPackedArgs> g) {
    const nlam_forecast_t& p = g.p;
    const nlam_forecast_src_t& c = g.s;
    const StatsLds stats{fc_stage_stats(p.state_mean, p.state_std, p.d_state)};
    const int b = blockIdx.z, r = blockIdx.y;
    const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
    const long j = max(2, p.num_past_forcing_steps) - 2 + r;
    const Series<ST> ser = state_series<ST>(c.state, g);
    const ST* src = fc_src_block(ser.base, c.state_stride_sample, c.state_stride_step, c.state_stride_member, c, c.state_steps,
                                 fc_sample(g, b), j);
    series_state_row(ser, src, (r == 0 ? p.prev_prev : p.prev) + (long)b * per, stats, per, (unsigned)p.d_state,
                     blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
    if (blockIdx.x == 0 && r == 0 && b == 0 && threadIdx.x == 0) *p.lead = 0;
}

// forecast_head_kernel over a strided source: the truth is row off + k, window slot w of the forcing row off + k - past + w
template <typename ST, typename FT>
__global__ __launch_bounds__(256) void forecast_head_strided_kernel(const SeriesArgs<ST, FT, ForecastSrcArgs, ForecastPackedArgs> g) {
    const nlam_forecast_t& p = g.p;
    const nlam_forecast_src_t& c = g.s;
    const int k = *p.lead;
    if (k >= p.max_lead) return;   // the same in every thread of the grid, ahead of every barrier
    const bool forc = blockIdx.y == 1;
    const StatsLds stats{forc ? fc_stage_stats(p.forcing_mean, p.forcing_std, p.d_forcing)
                              : fc_stage_stats(p.state_mean, p.state_std, p.d_state)};
    const int b = blockIdx.z;
    const FcSample i = fc_sample(g, b);
    const int past = p.num_past_forcing_steps;
    const long jv = max(2, past) + k;   // the row of this lead
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
    if (!forc) {
        const unsigned per = (unsigned)p.nodes * (unsigned)p.d_state;
        const Series<ST> ser = state_series<ST>(c.state, g);
        const ST* src = fc_src_block(ser.base, c.state_stride_sample, c.state_stride_step, c.state_stride_member, c, c.state_steps, i, jv);
        series_state_row(ser, src, p.truth + (long)b * per, stats, per, (unsigned)p.d_state, tid, nthr);
        return;
    }
    const unsigned W = past + p.num_future_forcing_steps + 1, df = p.d_forcing;
    const Series<FT> ser = forcing_series<FT>(c.forcing, g);
    series_forcing_row(ser, p.forcing_windowed + (long)b * p.nodes * (df * W), stats, (unsigned)p.nodes, df, W, tid, nthr, [&](unsigned w) {
        return fc_src_block(ser.base, c.forcing_stride_sample, c.forcing_stride_step, c.forcing_stride_member, c, c.forcing_steps, i,
                            jv - past + (long)w);
    });
}

// blockIdx.y = forecast of the batch, blockIdx.x = chunk of fc_chunk_nodes nodes.  LDS: StepTailTables, (std, mean) of the state,
// and with VERIFY the chunk's weighted errors [2][chunk elements], which 2 F threads then add per variable in node order.
template <bool HAS_CLAMP, bool HAS_STD, bool VERIFY>
__global__ __launch_bounds__(256) void forecast_tail_kernel(const ForecastTailArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const nlam_forecast_t& p = a.p;
    const int k = *p.lead;
    if (k >= p.max_lead) return;   // the same in every thread of the grid, ahead of every barrier
    const StepTailTables<NLAM_LOSS_MSE, HAS_CLAMP, HAS_STD> tab(a.t);
    const int F = p.d_state, N = p.nodes, ld = p.delta_ld;
    float2* const phys = reinterpret_cast<float2*>(smem + fc_tab_floats(F));
    float* const tile = reinterpret_cast<float*>(phys + F);
    for (int v = threadIdx.x; v < F; v += blockDim.x) phys[v] = make_float2(p.state_std[v], p.state_mean[v]);
    __syncthreads();
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int cn = fc_chunk_nodes(F);
    const int n0 = chunk * cn, n1 = min(N, n0 + cn);
    const int cnt = (n1 - n0) * F, tstride = cn * F;
    const long base = ((long)b * N + n0) * F;
    const long obase = (((long)b * p.max_lead + k) * N + n0) * F;
    float* const prev = p.prev + base;
    float* const pprev = p.prev_prev + base;
    const float* const truth = p.truth + base;
    const float* const delta = p.delta + ((long)b * N + n0) * ld;
    float* const out = p.out_state + obase;
    float* const ostd = HAS_STD ? p.out_std + obase : nullptr;
    const float* __restrict__ bmask = p.bmask;
    const float* __restrict__ row_weight = p.row_weight;
    const bool vec = ((reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(pprev) | reinterpret_cast<uintptr_t>(truth) |
                       reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ostd) |
                       (HAS_STD ? 0 : reinterpret_cast<uintptr_t>(delta))) & 15) == 0;
    for (int e = 4 * threadIdx.x; e < cnt; e += 4 * blockDim.x) {
        const unsigned row = (unsigned)e / (unsigned)F;
        int f = e - (int)row * F, n = n0 + (int)row;
        const bool quad = vec && e + 3 < cnt;
        f32x4 pr = {0.f, 0.f, 0.f, 0.f}, tr = {0.f, 0.f, 0.f, 0.f}, dl = {0.f, 0.f, 0.f, 0.f}, raw = {0.f, 0.f, 0.f, 0.f};
        if (quad) {
            pr = *reinterpret_cast<const f32x4*>(prev + e);
            tr = *reinterpret_cast<const f32x4*>(truth + e);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (e + c < cnt) {
                    pr[c] = prev[e + c];
                    tr[c] = truth[e + c];
                }
        }
        if (!HAS_STD && quad) {
            dl = *reinterpret_cast<const f32x4*>(delta + e);
        } else {   // with a std head the delta rows are twice as long: a quad's eight values one by one
            long di = (long)row * ld + f;
            int fd = f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (e + c < cnt) {
                    dl[c] = delta[di];
                    if constexpr (HAS_STD) raw[c] = delta[di + F];
                }
                ++di;
                if (++fd == F) {
                    fd = 0;
                    di += ld - F;
                }
            }
        }
        f32x4 nv, ov, sv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const bool live = e + c < cnt;
            const int nn = live ? n : n0;   // a dead lane of the last quad reads a valid node
            const float nw = step_tail_pred<HAS_CLAMP>(tab, dl[c], pr[c], tr[c], bmask[nn], f);
            const float2 ph = phys[f];
            nv[c] = nw;
            ov[c] = nw * ph.x + ph.y;
            if constexpr (HAS_STD) sv[c] = softplus_fwd(raw[c]) * ph.x;
            if constexpr (VERIFY) {
                if (live) {
                    const float w = row_weight[nn];
                    const float d = nw - tr[c];
                    tile[e + c] = w != 0.f ? w * (d * d) : 0.f;
                    tile[tstride + e + c] = w != 0.f ? w * fabsf(d) : 0.f;
                }
            }
            if (++f == F) {
                f = 0;
                ++n;
            }
        }
        if (quad) {
            *reinterpret_cast<f32x4*>(pprev + e) = pr;
            *reinterpret_cast<f32x4*>(prev + e) = nv;
            *reinterpret_cast<f32x4*>(out + e) = ov;
            if constexpr (HAS_STD) *reinterpret_cast<f32x4*>(ostd + e) = sv;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (e + c < cnt) {
                    pprev[e + c] = pr[c];
                    prev[e + c] = nv[c];
                    out[e + c] = ov[c];
                    if constexpr (HAS_STD) ostd[e + c] = sv[c];
                }
        }
    }
    if (chunk == 0 && threadIdx.x == 0 && p.valid_times != nullptr) {
        const long tv = fc_clamp_time(p.start[b] + k + 1, p.n_times - 1);
        p.valid_times[(long)b * p.max_lead + k] = p.times != nullptr ? p.times[tv] : tv;
    }
    if constexpr (VERIFY) {
        __syncthreads();
        float* const ws = p.workspace + ((long)b * gridDim.x + chunk) * (2 * F);
        for (int j = threadIdx.x; j < 2 * F; j += blockDim.x) {   // j = q * F + f: the chunk's sum of variable f, in node order
            const int q = j / F, fj = j - q * F;
            const float* col = tile + q * tstride + fj;
            float v = 0.f;
            for (int r = 0; r < n1 - n0; ++r) v += col[r * F];
            ws[j] = v;
        }
    }
}

// one workgroup.  nchunks > 0: lane -> one of the batch * 2 F sums, the four waves split the chunks, combined in wave order.
__global__ __launch_bounds__(256) void forecast_finish_kernel(const nlam_forecast_t p, int nchunks) {
    __shared__ int ks;
    __shared__ float red[4][64];
    if (threadIdx.x == 0) ks = *p.lead;
    __syncthreads();
    const int k = ks;
    if (k >= p.max_lead) return;
    if (nchunks > 0) {
        const int F = p.d_state, W2 = 2 * F, M = p.batch * W2;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int per = (nchunks + 3) / 4, c0 = wave * per, c1 = min(nchunks, c0 + per);
        for (int m0 = 0; m0 < M; m0 += 64) {
            const int m = m0 + lane;
            const int b = m / W2, j = m - b * W2;
            float v = 0.f;
            if (m < M) {
                const float* src = p.workspace + (long)b * nchunks * W2 + j;
#pragma unroll 8
                for (int c = c0; c < c1; ++c) v += src[(long)c * W2];
            }
            red[wave][lane] = v;
            __syncthreads();
            if (wave == 0 && m < M) {
                const int q = j / F, f = j - q * F;
                float* const dst = q == 0 ? p.sq : p.ab;
                if (dst != nullptr) dst[((long)b * p.max_lead + k) * F + f] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) *p.lead = k + 1;
}

enum { kFcInit, kFcHead, kFcTail, kFcFinish };

bool fc_verifies(const nlam_forecast_t* p) { return p->sq != nullptr || p->ab != nullptr; }

// every check before any launch
int32_t forecast_check(const nlam_forecast_t* p, int which) {
    if (p == nullptr || p->lead == nullptr) return NLAM_EINVAL;
    if (p->n_times < 1 || p->nodes < 1 || p->d_state < 1 || p->d_forcing < 0 || p->batch < 1 || p->max_lead < 1 ||
        p->num_past_forcing_steps < 0 || p->num_future_forcing_steps < 0)
        return NLAM_EINVAL;
    if (p->d_state > NLAM_LOSS_MAX_VARS || p->d_forcing > NLAM_LOSS_MAX_VARS || p->batch > 65535) return NLAM_EUNSUP;
    const long window = (long)p->num_past_forcing_steps + p->num_future_forcing_steps + 1;
    if ((long)p->nodes * p->d_state >= (1L << 31) || (long)p->nodes * p->d_forcing * window >= (1L << 31)) return NLAM_EUNSUP;
    if (which != kFcFinish) {
        if (p->state == nullptr || p->start == nullptr || p->state_mean == nullptr || p->state_std == nullptr) return NLAM_EINVAL;
        if (p->d_forcing > 0 && (p->forcing == nullptr || p->forcing_mean == nullptr || p->forcing_std == nullptr)) return NLAM_EINVAL;
    }
    if (which == kFcInit && (p->prev == nullptr || p->prev_prev == nullptr)) return NLAM_EINVAL;
    if (which == kFcHead && (p->truth == nullptr || (p->d_forcing > 0 && p->forcing_windowed == nullptr))) return NLAM_EINVAL;
    if (which == kFcTail) {
        if (p->delta == nullptr || p->prev == nullptr || p->prev_prev == nullptr || p->truth == nullptr || p->bmask == nullptr ||
            p->out_state == nullptr)
            return NLAM_EINVAL;
        const bool has_std = p->delta_ld == 2 * p->d_state;
        if ((p->delta_ld != p->d_state && !has_std) || has_std != (p->out_std != nullptr)) return NLAM_EINVAL;
        if (p->clamp_mode_host != nullptr) {
            if (p->clamp_lo == nullptr || p->clamp_hi == nullptr) return NLAM_EINVAL;
            for (int v = 0; v < p->d_state; ++v)
                if (p->clamp_mode_host[v] < NLAM_CLAMP_NONE || p->clamp_mode_host[v] > NLAM_CLAMP_UPPER) return NLAM_EINVAL;
        }
    }
    if ((which == kFcTail || which == kFcFinish) && fc_verifies(p)) {
        if (p->d_state > NLAM_EVAL_MAX_VARS) return NLAM_EUNSUP;
        if (p->workspace == nullptr || (which == kFcTail && p->row_weight == nullptr)) return NLAM_EINVAL;
        if (p->workspace_floats < (long)p->batch * fc_nchunks(p->nodes, p->d_state) * 2 * p->d_state) return NLAM_EINVAL;
    }
    return 0;
}

// the checks of a strided source, and the launch arguments: the series, the sample indices and n_times of `p` are replaced by the
// source's, so that forecast_check sees what the kernels read
int32_t forecast_src_check(const nlam_forecast_t* p, const nlam_forecast_src_t* s, int which, ForecastSrcArgs* a) {
    if (p == nullptr || s == nullptr) return NLAM_EINVAL;
    a->p = *p;
    a->s = *s;
    a->p.state = s->state;
    a->p.forcing = s->forcing;
    a->p.start = s->sample_idx;
    a->p.n_times = s->n_times;
    if (const int32_t rc = forecast_check(&a->p, which)) return rc;
    if (s->members < 1 || (s->is_forecast != 0 && s->is_forecast != 1)) return NLAM_EINVAL;
    if (s->state_stride_sample < 0 || s->state_stride_step < 0 || s->state_stride_member < 0 || s->forcing_stride_sample < 0 ||
        s->forcing_stride_step < 0 || s->forcing_stride_member < 0)
        return NLAM_EINVAL;
    const int64_t off = p->num_past_forcing_steps > 2 ? p->num_past_forcing_steps : 2;
    int64_t base_len;
    if (s->is_forecast) {
        if (s->state_steps < off + p->max_lead) return NLAM_EINVAL;   // lead-time axis too short
        if (p->d_forcing > 0 && s->forcing_steps < off + p->max_lead + p->num_future_forcing_steps) return NLAM_EINVAL;
        base_len = s->n_times;
    } else {
        if (s->state_stride_sample != s->state_stride_step || (p->d_forcing > 0 && s->forcing_stride_sample != s->forcing_stride_step))
            return NLAM_EINVAL;   // one time axis
        base_len = nlam_window_len(s->n_times, -1, p->max_lead, p->num_past_forcing_steps, p->num_future_forcing_steps);
        if (base_len < 1) base_len = 1;   // too short a series: the time clamp keeps every read inside it
    }
    a->n_flat = (long)(base_len * s->members);
    return 0;
}

// workgroups of a (nodes x row) block of `elems` floats: four elements per thread, two rounds
int fc_row_blocks(long elems) {
    const long blocks = (elems + 2047) / 2048;
    return (int)(blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks));
}

// grid and dynamic LDS of an init / a head launch: two state rows, or the truth row and the forcing row, per forecast
struct FcRowShape {
    dim3 grid;
    size_t lds;   // the (mean, std) table of the widest row
};

FcRowShape fc_init_shape(const nlam_forecast_t& p) {
    return {dim3(fc_row_blocks((long)p.nodes * p.d_state), 2, p.batch), (size_t)p.d_state * sizeof(float2)};
}

FcRowShape fc_head_shape(const nlam_forecast_t& p) {
    const long window = (long)p.num_past_forcing_steps + p.num_future_forcing_steps + 1;
    const long e_state = (long)p.nodes * p.d_state, e_forc = (long)p.nodes * p.d_forcing * window;
    const int wide = p.d_state > p.d_forcing ? p.d_state : p.d_forcing;
    return {dim3(fc_row_blocks(e_state > e_forc ? e_state : e_forc), p.d_forcing > 0 ? 2 : 1, p.batch), (size_t)wide * sizeof(float2)};
}

// forecast_src_check with the packed source in place of the float series: a packed series stands in for the float pointer the
// shared checks ask for (no kernel of the pair reads it through that pointer)
int32_t forecast_q16_check(const nlam_forecast_t* p, const nlam_forecast_src_t* s, const nlam_q16_src_t* q, int which,
                           ForecastPackedArgs* g) {
    if (p == nullptr || s == nullptr || q == nullptr) return NLAM_EINVAL;
    if (const int32_t rc = q16_src_check(q, s->state, s->forcing, p->d_forcing)) return rc;
    nlam_forecast_src_t s2 = *s;
    if (q->state != nullptr) s2.state = reinterpret_cast<const float*>(q->state);
    if (p->d_forcing > 0 && q->forcing != nullptr) s2.forcing = reinterpret_cast<const float*>(q->forcing);
    if (const int32_t rc = forecast_src_check(p, &s2, which, g)) return rc;
    g->s = *s;
    g->q = *q;
    return 0;
}

// the strided launches, fp32 (g.q names no series: the float instantiations take the ForecastSrcArgs in front of it) or packed
int32_t forecast_init_series(const ForecastPackedArgs& g, hipStream_t stream) {
    const FcRowShape sh = fc_init_shape(g.p);
    return pick_elem(g.q.state != nullptr, [&](auto st) {
        using A = SeriesArgs<decltype(st), float, ForecastSrcArgs, ForecastPackedArgs>;
        return launch<forecast_init_strided_kernel<decltype(st)>>(sh.grid, dim3(256), sh.lds, stream, static_cast<const A&>(g));
    });
}

int32_t forecast_head_series(const ForecastPackedArgs& g, hipStream_t stream) {
    const FcRowShape sh = fc_head_shape(g.p);
    return pick_elem(g.q.state != nullptr, [&](auto st) {
        return pick_elem(g.p.d_forcing > 0 && g.q.forcing != nullptr, [&](auto ft) {
            using A = SeriesArgs<decltype(st), decltype(ft), ForecastSrcArgs, ForecastPackedArgs>;
            return launch<forecast_head_strided_kernel<decltype(st), decltype(ft)>>(sh.grid, dim3(256), sh.lds, stream,
                                                                                   static_cast<const A&>(g));
        });
    });
}

}  // namespace

extern "C" {

int32_t nlam_forecast_init(const nlam_forecast_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_forecast_init");
    if (const int32_t rc = forecast_check(p, kFcInit)) return rc;
    const FcRowShape sh = fc_init_shape(*p);
    return launch<forecast_init_kernel>(sh.grid, dim3(256), sh.lds, (hipStream_t)hip_stream, *p);
}

int32_t nlam_forecast_head(const nlam_forecast_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_forecast_head");
    if (const int32_t rc = forecast_check(p, kFcHead)) return rc;
    const FcRowShape sh = fc_head_shape(*p);
    return launch<forecast_head_kernel>(sh.grid, dim3(256), sh.lds, (hipStream_t)hip_stream, *p);
}

int32_t nlam_forecast_init_strided(const nlam_forecast_t* p, const nlam_forecast_src_t* src, void* hip_stream) {
    NLAM_RANGE("nlam_forecast_init_strided");
    ForecastPackedArgs g = {};
    if (const int32_t rc = forecast_src_check(p, src, kFcInit, &g)) return rc;
    return forecast_init_series(g, (hipStream_t)hip_stream);
}

int32_t nlam_forecast_head_strided(const nlam_forecast_t* p, const nlam_forecast_src_t* src, void* hip_stream) {
    NLAM_RANGE("nlam_forecast_head_strided");
    ForecastPackedArgs g = {};
    if (const int32_t rc = forecast_src_check(p, src, kFcHead, &g)) return rc;
    return forecast_head_series(g, (hipStream_t)hip_stream);
}

int32_t nlam_forecast_init_q16(const nlam_forecast_t* p, const nlam_forecast_src_t* src, const nlam_q16_src_t* packed,
                               void* hip_stream) {
    NLAM_RANGE("nlam_forecast_init_q16");
    ForecastPackedArgs g;
    if (const int32_t rc = forecast_q16_check(p, src, packed, kFcInit, &g)) return rc;
    return forecast_init_series(g, (hipStream_t)hip_stream);
}

int32_t nlam_forecast_head_q16(const nlam_forecast_t* p, const nlam_forecast_src_t* src, const nlam_q16_src_t* packed,
                               void* hip_stream) {
    NLAM_RANGE("nlam_forecast_head_q16");
    ForecastPackedArgs g;
    if (const int32_t rc = forecast_q16_check(p, src, packed, kFcHead, &g)) return rc;
    return forecast_head_series(g, (hipStream_t)hip_stream);
}

int32_t nlam_forecast_tail(const nlam_forecast_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_forecast_tail");
    if (const int32_t rc = forecast_check(p, kFcTail)) return rc;
    ForecastTailArgs a;
    memset(&a.t, 0, sizeof(a.t));
    a.p = *p;
    a.t.p.dstd = p->dstd;
    a.t.p.dmean = p->dmean;
    a.t.p.clamp_lo = p->clamp_lo;
    a.t.p.clamp_hi = p->clamp_hi;
    a.t.p.nvars = p->d_state;
    bool clamp = false;
    if (p->clamp_mode_host != nullptr)
        for (int v = 0; v < p->d_state; ++v) {
            a.t.mode_bits[v >> 4] |= (uint32_t)p->clamp_mode_host[v] << (2 * (v & 15));
            clamp |= p->clamp_mode_host[v] != NLAM_CLAMP_NONE;
        }
    const bool has_std = p->out_std != nullptr, verify = fc_verifies(p);
    const int F = p->d_state;
    const size_t lds = ((size_t)fc_tab_floats(F) + 2 * (size_t)F + (verify ? 2 * (size_t)fc_chunk_nodes(F) * F : 0)) * sizeof(float);
    const dim3 grid(fc_nchunks(p->nodes, F), p->batch);
    const hipStream_t stream = (hipStream_t)hip_stream;
    return pick_bool(clamp, [&](auto hc) {
        return pick_bool(has_std, [&](auto hs) {
            return pick_bool(verify, [&](auto vf) { return launch<forecast_tail_kernel<hc, hs, vf>>(grid, dim3(256), lds, stream, a); });
        });
    });
}

int32_t nlam_forecast_finish(const nlam_forecast_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_forecast_finish");
    if (const int32_t rc = forecast_check(p, kFcFinish)) return rc;
    const int nchunks = fc_verifies(p) ? fc_nchunks(p->nodes, p->d_state) : 0;
    hipLaunchKernelGGL(forecast_finish_kernel, dim3(1), dim3(nchunks > 0 ? 256 : 64), 0, (hipStream_t)hip_stream, *p, nchunks);
    return (int32_t)hipGetLastError();
}

int64_t nlam_forecast_workspace_floats(int32_t batch, int32_t nodes, int32_t nvars) {
    if (batch < 1 || nodes < 1 || nvars < 1) return NLAM_EINVAL;
    if (nvars > NLAM_EVAL_MAX_VARS) return NLAM_EUNSUP;
    return (int64_t)batch * fc_nchunks(nodes, nvars) * 2 * nvars;
}

}  // extern "C"
