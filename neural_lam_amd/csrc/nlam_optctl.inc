// Optimizer controls decided on the device (nlam_grad_sumsq, nlam_adamw_step_controlled): the global norm of the flat
// gradient, the clip coefficient, the learning rate of a closed-form schedule and the skip of a non-finite step, by kernels
// that sit in front of the AdamW update inside the captured step.  No launch argument depends on the step.
//
//   grad_sumsq_kernel     one pass over the gradient with 16-byte loads; fp64 from the first element (two fp64 operations per
//                         fp32 element are far below what the stream delivers), lanes -> wave -> workgroup in a fixed order,
//                         one fp64 partial per workgroup.  No atomics: the same buffer gives the same bits on every run.
//   adamw_control_kernel  one wave: the partials in a fixed order, norm = grad_scale * sqrt(sum), the finiteness test, the
//                         resident step count and bias corrections (adamw_prep_kernel's expressions), the schedule in fp64
//                         rounded once, torch's clip coefficient; everything the update needs goes to a block of
//                         NLAM_OPTCTL_WORDS words that the host may read later.
//   adamw_ctl_kernel      adamw_kernel's arithmetic with lr and the clip coefficient read from that block; returns before
//                         touching anything when the skip flag is up.
// Gradient accumulation over K micro-batches (nlam_accum_begin, nlam_adamw_step_accum): the same launches, each gated by a
// block of NLAM_ACCUM_WORDS words on the device, so one recorded step serves every micro-step of a window.
//   accum_begin_kernel          the zero of the flat gradient in front of the step: only when word 0 (the index of the
//                               micro-batch) is 0; 16-byte stores on the aligned interior, single elements around it.
//   grad_sumsq_accum_kernel     grad_sumsq_kernel's body; every workgroup returns unless word 0 is K - 1.
//   adamw_control_accum_kernel  adds the micro-batch loss to the window's sum and either holds (advance word 0, raise the
//                               hold flag) or closes the window and decides as adamw_control_kernel does (one shared body).
//   adamw_ctl_accum_kernel      adamw_ctl_kernel's body behind the hold flag and the skip flag.
// The moving average of the weights (nlam_adamw_step_controlled_ema) is a template flag of adamw_ctl_body and its two kernels:
// behind the same gates, from the parameter value the launch holds (EmaArg / ema_one in nlam_hip.hip).  flat_swap_kernel
// exchanges weights and average in place (nlam_flat_swap), head / tail as accum_begin_kernel.
// Included from nlam_hip.hip inside NLAM_IN_TU(5).

namespace {

constexpr int kSumsqThreads = 256;
constexpr int kSumsqQuads = 4;   // 16-byte loads in flight per lane

__host__ __device__ inline int sumsq_blocks(long n) {
    const long per_wg = 4L * kSumsqThreads * kSumsqQuads;
    const long need = n < 1 ? 1 : (n + per_wg - 1) / per_wg;
    return (int)(need < kMaxGridBlocks ? need : kMaxGridBlocks);
}

// butterfly: every lane ends with the same sum, added in an order that depends on nothing but the lane numbers
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void grad_sumsq_body(const float* g, long n, double* partials) {
    __shared__ double red[kSumsqThreads / 64];
    const int tid = threadIdx.x;
    // elements in front of the first 16-byte boundary and behind the last whole quad: lanes 0-2 / 3-5 of workgroup 0
    long head = (long)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2);
    if (head > n) head = n;
    const long nq = (n - head) >> 2;
    const long tail0 = head + 4 * nq;
    const f32x4* q = reinterpret_cast<const f32x4*>(g + head);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const long stride = (long)gridDim.x * kSumsqThreads;
    long i = (long)blockIdx.x * kSumsqThreads + tid;
    for (; i + (kSumsqQuads - 1) * stride < nq; i += kSumsqQuads * stride) {
        f32x4 v[kSumsqQuads];
#pragma unroll
        for (int u = 0; u < kSumsqQuads; ++u) v[u] = q[i + u * stride];
#pragma unroll
        for (int u = 0; u < kSumsqQuads; ++u) {
            const double x0 = (double)v[u][0], x1 = (double)v[u][1], x2 = (double)v[u][2], x3 = (double)v[u][3];
            a0 = fma(x0, x0, a0);
            a1 = fma(x1, x1, a1);
            a2 = fma(x2, x2, a2);
            a3 = fma(x3, x3, a3);
        }
    }
    for (; i < nq; i += stride) {
        const f32x4 v = q[i];
        const double x0 = (double)v[0], x1 = (double)v[1], x2 = (double)v[2], x3 = (double)v[3];
        a0 = fma(x0, x0, a0);
        a1 = fma(x1, x1, a1);
        a2 = fma(x2, x2, a2);
        a3 = fma(x3, x3, a3);
    }
    if (blockIdx.x == 0) {
        if (tid < head) {
            const double x = (double)g[tid];
            a0 = fma(x, x, a0);
        } else if (tid >= 3 && tail0 + (tid - 3) < n && tid < 6) {
            const double x = (double)g[tail0 + (tid - 3)];
            a0 = fma(x, x, a0);
        }
    }
    const double w = wave_sum_f64((a0 + a1) + (a2 + a3));
    if ((tid & 63) == 0) red[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        double s = red[0];
#pragma unroll
        for (int k = 1; k < kSumsqThreads / 64; ++k) s += red[k];
        partials[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kSumsqThreads) void grad_sumsq_kernel(const float* g, long n, double* partials) {
    grad_sumsq_body(g, n, partials);
}

// the norm is wanted on the micro-step that closes a window only (accum[0] is uniform: the whole grid takes one side)
__global__ __launch_bounds__(kSumsqThreads) void grad_sumsq_accum_kernel(const float* g, long n, double* partials, const int32_t* accum,
                                                                         int last) {
    if (accum[0] != last) return;
    grad_sumsq_body(g, n, partials);
}

// the partials in a fixed order, by one wave: lane l adds l, l + 64, ... in order, then the butterfly
__device__ __forceinline__ double partials_sum(const double* partials, int nparts) {
    double s = 0.0;
    for (int k = (int)(threadIdx.x & 63); k < nparts; k += 64) s += partials[k];
    return wave_sum_f64(s);
}

__global__ __launch_bounds__(64) void grad_norm_finish_kernel(const double* partials, int nparts, float scale, float* norm) {
    const double s = partials_sum(partials, nparts);
    if (threadIdx.x == 0) norm[0] = (float)((double)scale * sqrt(s));
}

// f(s) of the header: LambdaLR's factor for the update that follows s earlier ones
__device__ __forceinline__ double schedule_factor(int kind, long s, long W, long T, double r) {
    if (s < W) return (double)(s + 1) / (double)W;
    if (kind == NLAM_SCHED_CONSTANT) return 1.0;
    const long span = T - W > 1 ? T - W : 1;
    double p = (double)(s - W) / (double)span;
    if (p > 1.0) p = 1.0;
    if (kind == NLAM_SCHED_WARMUP_COSINE) return r + (1.0 - r) * 0.5 * (1.0 + cos(3.14159265358979323846 * p));
    return r + (1.0 - r) * (1.0 - p);
}

struct OptCtlArgs {
    const double* partials;
    int32_t* step_count;
    float* bias_corr;
    float* ctl_f;      // the control block as floats: [0] lr_t, [1] clip coefficient, [2] norm
    int32_t* ctl_i;    // and as words: [3] skip flag, [4] skipped steps
    int nparts;
    float lr, b1, b2, grad_scale, max_norm, min_ratio;
    int kind, warmup, total, skip_nonfinite;
};

// lane 0 of the control wave, with the sum of the partials: everything the update launch reads
__device__ __forceinline__ void optctl_decide(const OptCtlArgs a, double sum) {
    const float norm = (float)((double)a.grad_scale * sqrt(sum));
    const bool finite = fabsf(norm) <= 3.402823466e+38f;   // false for inf and nan
    a.ctl_f[2] = norm;
    if (a.skip_nonfinite && !finite) {
        a.ctl_f[1] = 0.f;
        a.ctl_i[3] = 1;
        a.ctl_i[4] = a.ctl_i[4] + 1;
        return;
    }
    const int t = *a.step_count + 1;
    *a.step_count = t;
    a.bias_corr[0] = 1.f - powf(a.b1, (float)t);
    a.bias_corr[1] = sqrtf(1.f - powf(a.b2, (float)t));
    float lr_t = a.lr;
    if (a.kind != NLAM_SCHED_NONE)
        lr_t = (float)((double)a.lr * schedule_factor(a.kind, (long)t - 1, a.warmup, a.total, (double)a.min_ratio));
    float coef = 1.f;
    if (a.max_norm > 0.f) {
        const float c = a.max_norm / (norm + 1e-6f);   // torch.nn.utils.clip_grad_norm_
        coef = c < 1.f ? c : 1.f;
    }
    a.ctl_f[0] = lr_t;
    a.ctl_f[1] = coef;
    a.ctl_i[3] = 0;
}

__global__ __launch_bounds__(64) void adamw_control_kernel(const OptCtlArgs a) {
    const double sum = partials_sum(a.partials, a.nparts);
    if (threadIdx.x != 0) return;
    optctl_decide(a, sum);
}

// acc: the NLAM_ACCUM_WORDS block ([0] micro-batch index, [1] hold flag, [2] running loss sum, [3] mean loss of the last
// closed window).  The loss is added in fp32 in call order, from 0 at the first micro-batch of a window.  A window that is
// not complete holds: word 0 advances, the flag goes up, the control block keeps the last closed window's values.  The last
// micro-batch closes the window -- also when the decision below is to skip, so that the next gated zero clears the gradient.
__global__ __launch_bounds__(64) void adamw_control_accum_kernel(const OptCtlArgs a, int32_t* acc, const float* loss, int steps) {
    const int k = acc[0];
    const bool closing = k == steps - 1;
    double sum = 0.0;
    if (closing) sum = partials_sum(a.partials, a.nparts);   // (the partials are stale on a holding micro-step)
    if (threadIdx.x != 0) return;
    float* acc_f = reinterpret_cast<float*>(acc);
    const float run = (k == 0 ? 0.f : acc_f[2]) + (loss != nullptr ? loss[0] : 0.f);
    acc_f[2] = run;
    if (!closing) {
        acc[0] = k + 1;
        acc[1] = 1;
        return;
    }
    acc[0] = 0;
    acc[1] = 0;
    acc_f[3] = run / (float)steps;
    optctl_decide(a, sum);
}

// (adamw_ctl_one, one element of the update, sits in nlam_hip.hip: adamw_kernel shares it)
// nq quads from 16-byte aligned bases, then the n - 4 nq elements behind them
// (first / stride: the caller's (long)blockIdx.x * blockDim.x + threadIdx.x and (long)gridDim.x * blockDim.x)
template <bool EMA>
__device__ __forceinline__ void adamw_ctl_body(float* param, const float* grad, float* m, float* v, long n, long nq, float b1, float b2,
                                               float eps, float wd, float gscale, const float* bias_corr, const float* ctl_f,
                                               long first, long stride, const EmaArg<EMA> ea) {
    int mode = kEmaOff;
    f32x4* e4 = nullptr;
    if constexpr (EMA) {
        mode = ema_mode(ea);
        e4 = reinterpret_cast<f32x4*>(ea.ema);
    }
    const float lr = ctl_f[0], coef = ctl_f[1];
    const float bc1 = bias_corr[0], bc2_sqrt = bias_corr[1];
    const float decay = fmaf(-lr, wd, 1.f), step = lr / bc1;   // torch.optim.AdamW: decoupled decay first
    f32x4* p4 = reinterpret_cast<f32x4*>(param);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(grad);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    for (long i = first; i < nq; i += stride) {
        f32x4 pv = p4[i], mo = m4[i], vo = v4[i];
        const f32x4 gr = g4[i];
        f32x4 avg = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EMA) {
            if (mode == kEmaLerp) avg = e4[i];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pv[k], mk = mo[k], vk = vo[k];
            adamw_ctl_one(pk, gr[k], mk, vk, decay, step, b1, b2, eps, bc2_sqrt, gscale, coef);
            pv[k] = pk;
            mo[k] = mk;
            vo[k] = vk;
        }
        m4[i] = mo;
        v4[i] = vo;
        p4[i] = pv;
        if constexpr (EMA) {
            if (mode == kEmaLerp) {
#pragma unroll
                for (int k = 0; k < 4; ++k) avg[k] = ema_one(avg[k], pv[k], ea.w);
                e4[i] = avg;
            } else if (mode == kEmaCopy) {
                e4[i] = pv;
            }
        }
    }
    for (long idx = 4 * nq + first; idx < n; idx += stride) {
        float pk = param[idx], mk = m[idx], vk = v[idx];
        float avg = 0.f;
        if constexpr (EMA) {
            if (mode == kEmaLerp) avg = ea.ema[idx];
        }
        adamw_ctl_one(pk, grad[idx], mk, vk, decay, step, b1, b2, eps, bc2_sqrt, gscale, coef);
        m[idx] = mk;
        v[idx] = vk;
        param[idx] = pk;
        if constexpr (EMA) {
            if (mode == kEmaLerp)
                ea.ema[idx] = ema_one(avg, pk, ea.w);
            else if (mode == kEmaCopy)
                ea.ema[idx] = pk;
        }
    }
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamw_ctl_kernel(float* param, const float* grad, float* m, float* v, long n, long nq, float b1,
                                                        float b2, float eps, float wd, float gscale, const float* bias_corr,
                                                        const float* ctl_f, const int32_t* ctl_i, const EmaArg<EMA> ea) {
    if (ctl_i[3] != 0) return;   // a non-finite step: parameters and moments (and the average) stay as they are
    adamw_ctl_body<EMA>(param, grad, m, v, n, nq, b1, b2, eps, wd, gscale, bias_corr, ctl_f,
                        (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, ea);
}

// ... and while a window is open (hold flag acc[1]) nothing is touched either
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_ctl_accum_kernel(float* param, const float* grad, float* m, float* v, long n, long nq,
                                                              float b1, float b2, float eps, float wd, float gscale,
                                                              const float* bias_corr, const float* ctl_f, const int32_t* ctl_i,
                                                              const int32_t* acc, const EmaArg<EMA> ea) {
    if (acc[1] != 0 || ctl_i[3] != 0) return;
    adamw_ctl_body<EMA>(param, grad, m, v, n, nq, b1, b2, eps, wd, gscale, bias_corr, ctl_f,
                        (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x, ea);
}

constexpr int kSwapThreads = 256;
constexpr int kSwapMaxBlocks = 256 * 8;   // adamw_ctl_kernel's cap

// a <-> b.  `head` elements in front of the first address that is 16-byte aligned in both buffers (the host passes n when
// there is none: the two sit at different offsets within 16 bytes), nq quads behind it, the rest one by one.  Every element
// is read and written by one lane only, so the exchange needs no ordering between lanes.
__global__ __launch_bounds__(kSwapThreads) void flat_swap_kernel(float* a, float* b, long n, long head, long nq) {
    const long first = (long)blockIdx.x * kSwapThreads + threadIdx.x, stride = (long)gridDim.x * kSwapThreads;
    f32x4* a4 = reinterpret_cast<f32x4*>(a + head);
    f32x4* b4 = reinterpret_cast<f32x4*>(b + head);
    for (long i = first; i < nq; i += stride) {
        const f32x4 x = a4[i], y = b4[i];
        a4[i] = y;
        b4[i] = x;
    }
    const long tail0 = head + 4 * nq;
    for (long k = first; k < head + (n - tail0); k += stride) {   // the elements around the quads
        const long idx = k < head ? k : tail0 + (k - head);
        const float x = a[idx], y = b[idx];
        a[idx] = y;
        b[idx] = x;
    }
}

constexpr int kZeroThreads = 256;
constexpr int kZeroMaxBlocks = 256 * 8;   // adamw_ctl_kernel's cap

// The gated memset of the flat gradient.  head / tail as in grad_sumsq_kernel: the elements in front of the first 16-byte
// boundary and behind the last whole quad go one by one (lanes 0-2 / 3-5 of workgroup 0), the quads between them with one
// 16-byte store each, grid-stride.
__global__ __launch_bounds__(kZeroThreads) void accum_begin_kernel(float* g, long n, const int32_t* accum) {
    if (accum[0] != 0) return;   // inside a window: the gradient keeps accumulating
    const int tid = threadIdx.x;
    long head = (long)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2);
    if (head > n) head = n;
    const long nq = (n - head) >> 2;
    const long tail0 = head + 4 * nq;
    f32x4* q = reinterpret_cast<f32x4*>(g + head);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const long stride = (long)gridDim.x * kZeroThreads;
    for (long i = (long)blockIdx.x * kZeroThreads + tid; i < nq; i += stride) q[i] = zero;
    if (blockIdx.x == 0) {
        if (tid < head)
            g[tid] = 0.f;
        else if (tid >= 3 && tid < 6 && tail0 + (tid - 3) < n)
            g[tail0 + (tid - 3)] = 0.f;
    }
}

int32_t sumsq_launch(const float* grad, int64_t n, double* partials, int64_t workspace_doubles, hipStream_t stream, int* nparts,
                     const int32_t* accum = nullptr, int last = 0) {
    if (grad == nullptr || partials == nullptr || n < 0) return NLAM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(grad) & 3) != 0 || (reinterpret_cast<uintptr_t>(partials) & 7) != 0) return NLAM_EINVAL;
    const int blocks = sumsq_blocks((long)n);
    if (workspace_doubles < blocks) return NLAM_EINVAL;
    if (accum == nullptr)
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(kSumsqThreads), 0, stream, grad, (long)n, partials);
    else
        hipLaunchKernelGGL(grad_sumsq_accum_kernel, dim3(blocks), dim3(kSumsqThreads), 0, stream, grad, (long)n, partials, accum, last);
    *nparts = blocks;
    return (int32_t)hipGetLastError();
}

inline bool accum_valid(const nlam_accum_t* a) {
    return a != nullptr && a->accum != nullptr && a->steps >= 1 && (reinterpret_cast<uintptr_t>(a->accum) & 3) == 0 &&
           (reinterpret_cast<uintptr_t>(a->loss) & 3) == 0;
}

// the three launches of nlam_adamw_step_controlled; with `acc` each of them behind its gate; EMA: the update launch also
// keeps the moving average `e`
template <bool EMA>
int32_t optctl_launch(const nlam_optctl_t* p, const nlam_accum_t* acc, hipStream_t stream, const nlam_ema_t* e = nullptr) {
    if (p == nullptr || p->param == nullptr || p->grad == nullptr || p->exp_avg == nullptr || p->exp_avg_sq == nullptr ||
        p->step_count_dev == nullptr || p->bias_corr_dev == nullptr || p->control == nullptr || p->n < 0)
        return NLAM_EINVAL;
    if (p->schedule < NLAM_SCHED_NONE || p->schedule > NLAM_SCHED_WARMUP_LINEAR || p->warmup_steps < 0 || p->total_steps < 0 ||
        !(p->min_ratio >= 0.f && p->min_ratio <= 1.f) || p->max_grad_norm != p->max_grad_norm)
        return NLAM_EINVAL;
    if (p->schedule == NLAM_SCHED_NONE && p->warmup_steps != 0) return NLAM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(p->control) & 3) != 0) return NLAM_EINVAL;
    EmaArg<EMA> ea;
    if constexpr (EMA) {
        if (!ema_valid(e)) return NLAM_EINVAL;
        ea = ema_arg(e, p->step_count_dev);
    }
    int nparts = 0;
    if (acc == nullptr) {
        if (const int32_t rc = sumsq_launch(p->grad, p->n, p->partials, p->partials_doubles, stream, &nparts)) return rc;
    } else {
        if (const int32_t rc = sumsq_launch(p->grad, p->n, p->partials, p->partials_doubles, stream, &nparts, acc->accum, acc->steps - 1))
            return rc;
    }
    OptCtlArgs a;
    a.partials = p->partials;
    a.step_count = p->step_count_dev;
    a.bias_corr = p->bias_corr_dev;
    a.ctl_f = reinterpret_cast<float*>(p->control);
    a.ctl_i = reinterpret_cast<int32_t*>(p->control);
    a.nparts = nparts;
    a.lr = p->lr, a.b1 = p->beta1, a.b2 = p->beta2, a.grad_scale = p->grad_scale;
    a.max_norm = p->max_grad_norm, a.min_ratio = p->min_ratio;
    a.kind = p->schedule, a.warmup = p->warmup_steps, a.total = p->total_steps, a.skip_nonfinite = p->skip_nonfinite != 0;
    if (acc == nullptr)
        hipLaunchKernelGGL(adamw_control_kernel, dim3(1), dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL(adamw_control_accum_kernel, dim3(1), dim3(64), 0, stream, a, acc->accum, acc->loss, (int)acc->steps);
    if (p->n == 0) return (int32_t)hipGetLastError();
    // quads only where all four buffers (five with the average) sit on a 16-byte boundary (the flat buffers do); element by
    // element otherwise
    uintptr_t bits = reinterpret_cast<uintptr_t>(p->param) | reinterpret_cast<uintptr_t>(p->grad) |
                     reinterpret_cast<uintptr_t>(p->exp_avg) | reinterpret_cast<uintptr_t>(p->exp_avg_sq);
    if constexpr (EMA) bits |= reinterpret_cast<uintptr_t>(e->ema);
    const long nq = (bits & 15) == 0 ? (long)(p->n >> 2) : 0L;
    const long work = nq > 0 ? nq : (long)p->n;
    long blocks = (work + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (acc == nullptr)
        hipLaunchKernelGGL(adamw_ctl_kernel<EMA>, dim3((int)blocks), dim3(256), 0, stream, p->param, p->grad, p->exp_avg, p->exp_avg_sq,
                           (long)p->n, nq, p->beta1, p->beta2, p->eps, p->weight_decay, p->grad_scale, (const float*)p->bias_corr_dev,
                           (const float*)a.ctl_f, (const int32_t*)a.ctl_i, ea);
    else
        hipLaunchKernelGGL(adamw_ctl_accum_kernel<EMA>, dim3((int)blocks), dim3(256), 0, stream, p->param, p->grad, p->exp_avg,
                           p->exp_avg_sq, (long)p->n, nq, p->beta1, p->beta2, p->eps, p->weight_decay, p->grad_scale,
                           (const float*)p->bias_corr_dev, (const float*)a.ctl_f, (const int32_t*)a.ctl_i,
                           (const int32_t*)acc->accum, ea);
    return (int32_t)hipGetLastError();
}

}  // namespace

extern "C" {

int64_t nlam_grad_sumsq_workspace_doubles(int64_t n) {
    if (n < 0) return NLAM_EINVAL;
    return sumsq_blocks((long)n);
}

int32_t nlam_grad_sumsq(const float* grad, int64_t n, double* partials, int64_t workspace_doubles, float scale, float* norm,
                        void* hip_stream) {
    NLAM_RANGE("nlam_grad_sumsq");
    const hipStream_t stream = (hipStream_t)hip_stream;
    int nparts = 0;
    if (const int32_t rc = sumsq_launch(grad, n, partials, workspace_doubles, stream, &nparts)) return rc;
    if (norm == nullptr) return 0;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(64), 0, stream, (const double*)partials, nparts, scale, norm);
    return (int32_t)hipGetLastError();
}

int32_t nlam_adamw_step_controlled(const nlam_optctl_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_adamw_step_controlled");
    return optctl_launch<false>(p, nullptr, (hipStream_t)hip_stream);
}

int32_t nlam_adamw_step_accum(const nlam_optctl_t* p, const nlam_accum_t* a, void* hip_stream) {
    NLAM_RANGE("nlam_adamw_step_accum");
    if (!accum_valid(a)) return NLAM_EINVAL;
    return optctl_launch<false>(p, a, (hipStream_t)hip_stream);
}

int32_t nlam_adamw_step_controlled_ema(const nlam_optctl_t* p, const nlam_accum_t* a, const nlam_ema_t* e, void* hip_stream) {
    NLAM_RANGE("nlam_adamw_step_controlled_ema");
    if (a != nullptr && !accum_valid(a)) return NLAM_EINVAL;
    if (!ema_valid(e)) return NLAM_EINVAL;   // (in front of optctl_launch's own checks: nothing is launched)
    return optctl_launch<true>(p, a, (hipStream_t)hip_stream, e);
}

int32_t nlam_flat_swap(float* a, float* b, int64_t n, void* hip_stream) {
    NLAM_RANGE("nlam_flat_swap");
    if (a == nullptr || b == nullptr || n < 0) return NLAM_EINVAL;
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
    if ((ua & 3) != 0 || (ub & 3) != 0) return NLAM_EINVAL;
    if (n == 0 || a == b) return 0;
    long head = (long)n, nq = 0;
    if ((ua & 15) == (ub & 15)) {   // a common 16-byte grid: quads between the first boundary and the last whole quad
        head = (long)(((16 - (ua & 15)) & 15) >> 2);
        if (head > (long)n) head = (long)n;
        nq = ((long)n - head) >> 2;
    }
    const long work = nq > (long)n - 4 * nq ? nq : (long)n - 4 * nq;
    long blocks = (work + kSwapThreads - 1) / kSwapThreads;
    blocks = blocks < 1 ? 1 : (blocks > kSwapMaxBlocks ? kSwapMaxBlocks : blocks);
    hipLaunchKernelGGL(flat_swap_kernel, dim3((int)blocks), dim3(kSwapThreads), 0, (hipStream_t)hip_stream, a, b, (long)n, head, nq);
    return (int32_t)hipGetLastError();
}

int32_t nlam_accum_begin(float* grad, int64_t n, const int32_t* accum, void* hip_stream) {
    NLAM_RANGE("nlam_accum_begin");
    if (grad == nullptr || accum == nullptr || n < 0) return NLAM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(grad) & 3) != 0 || (reinterpret_cast<uintptr_t>(accum) & 3) != 0) return NLAM_EINVAL;
    if (n == 0) return 0;
    long blocks = ((long)(n >> 2) + kZeroThreads - 1) / kZeroThreads;
    blocks = blocks < 1 ? 1 : (blocks > kZeroMaxBlocks ? kZeroMaxBlocks : blocks);
    hipLaunchKernelGGL(accum_begin_kernel, dim3((int)blocks), dim3(kZeroThreads), 0, (hipStream_t)hip_stream, grad, (long)n, accum);
    return (int32_t)hipGetLastError();
}

}  // extern "C"
