// nlam_gemm.inc -- the tiled-GEMM MLP family: nlam_mlp_fwd_gemm / nlam_mlp_bwd_gemm for any width (above all the widths above
// kMaxWide = 512 that the fused kernels of nlam_wide.inc / nlam_wbf.inc do not instantiate).  Included from nlam_hip.hip inside
// NLAM_IN_TU(6).
//
// The fused kernels keep a whole row of the hidden layer in registers / LDS; above 512 columns that does not fit, so this family
// runs an MLP launch as a short chain of kernels over HBM-resident intermediates (all of them capturable: no host
// synchronisation, no allocation -- the intermediates live in the caller's `wpack` scratch):
//   forward   z1 = [gathered sources] W1^T + b1            gemm_kernel (A gathered / concatenated on load)
//             z2 = act(z1) W2^T + b2                        gemm_kernel (SiLU applied on load: silu(z1) is never stored)
//             LayerNorm, residuals, out / scatter          ln_fwd_rows_kernel (one wave per row)
//             segment aggregation                          tile_segsum_kernel (the tile schedule's receivers, CSR order)
//   backward  g = g_out + g_aggr[receiver] (x inv_deg), dz2 = LayerNorm backward      ln_bwd_rows_kernel
//             dz1 = (dz2 W2) * silu'(z1)                    gemm_kernel (W2 read as (k, n))
//             dX  = dz1 W1 (+ residual gradients), per source scattered (dmode 1), tile-row order (2) or staged for the
//                   segment sum (3)                         gemm_kernel (W1 read as (k, n)) + tile_segsum_kernel
//             db1, db2, dgamma, dbeta partial rows         colsum_partials_kernel (fixed row blocks, fixed order)
// Every reduction but one has a fixed order: the results are bit-identical run to run.  The exception are tile lists with
// NLAM_TILE_SPLIT tiles (the one-pass split mode): tile_segsum_kernel adds each piece of such a receiver with atomicAdd, in no
// fixed order, into a destination the CALLER must have zeroed -- `aggr` in the forward and every dmode-3 `dsrc` in the backward
// (ops.py allocates both with torch.zeros on that path).  The virtual split + nlam_split_combine keeps the fixed order.
//
// gemm_kernel: 128 x 128 output tiles, 256 threads (2 x 2 waves of 64 x 64), K staged through LDS in steps of 32 (fp32,
// register-prefetched one step ahead), products on v_mfma_f32_32x32x16_bf16 with each operand split into NS bf16 terms and
// fp32 accumulation (split8 / MFMA_BF16 of the split-bf16 kernels).  NS = 3 (fp32-class) serves NLAM_F_MM_BF16X3 and ALSO the
// fp32 (matrix bits 0) and two-term (NLAM_F_MM_BF16X2) modes: this family has no fp32-MFMA or two-term kernels; NS = 1 serves
// NLAM_F_MM_BF16X1 (bf16 autocast).  Weights are read in nn.Linear layout, no packing step.  Any width >= 1: loads and stores
// are predicated per element (sources of 2-3 columns, widths that are no multiple of 32).

namespace {

constexpr int kGemmBM = 128;
constexpr int kGemmBN = 128;
constexpr int kGemmBK = 32;
constexpr int kGemmLd = kGemmBK + 4;   // LDS row stride (floats): 16-byte aligned rows for the fragment reads
constexpr int kGemmThreads = 256;
constexpr int kGemmPartBlocks = 256;   // row blocks of the (db1, db2, dgamma, dbeta) partial sums

enum { kEpiBias = 0, kEpiDsilu = 1, kEpiScatter = 2 };

// element s of a 3-array kernel argument by selects: a per-lane index into the argument struct would copy it to scratch
template <class T>
__device__ __forceinline__ T sel3(const T (&a)[NLAM_MAX_SRC], int s) {
    return s == 0 ? a[0] : (s == 1 ? a[1] : a[2]);
}

struct GemmArgs {
    // A operand: row R of (M = batch * rows) is the concatenation of up to three (gathered) source rows
    int M, K, rows, nsrc, silu_a;
    const float* sptr[NLAM_MAX_SRC];
    const int32_t* sidx[NLAM_MAX_SRC];
    long sbstride[NLAM_MAX_SRC];
    int swidth[NLAM_MAX_SRC];
    int scol0[NLAM_MAX_SRC + 1];
    // B operand: nn = 0: W[n * ldw + k] (z = x W^T), nn = 1: W[k * ldw + n] (dx = dz W)
    const float* W;
    long ldw;
    int N;
    // epilogue
    int epi, no_act;
    const float* bias;   // kEpiBias: C = acc + bias
    float* C;            // kEpiBias / kEpiDsilu: (M, N) rows, row stride N
    const float* z;      // kEpiDsilu: C = acc * silu'(z) (z: (M, N) rows)
    // kEpiScatter: column n of source s goes to dst[s] + b * dbstride[s] + (didx[s] ? didx[s][r] : r) * width_s + (n - col0_s)
    float* dst[NLAM_MAX_SRC];
    long dbstride[NLAM_MAX_SRC];
    const int32_t* didx[NLAM_MAX_SRC];
    int dcol0[NLAM_MAX_SRC + 1];
    int ndst;
    // residual gradients: source 0 += g_out[b, out_idx[r]] (NLAM_F_ADD_SRC0), source 1 += gm[R] (NLAM_F_ADD_SRC1)
    const float* g_out;
    const int32_t* out_idx;
    long out_bstride;
    const float* gm;
};

template <int NS, int NN>
__global__ __launch_bounds__(kGemmThreads) void gemm_kernel(const GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[kGemmBM * kGemmLd];
    __shared__ __attribute__((aligned(16))) float Bs[kGemmBN * kGemmLd];
    __shared__ long roff[NLAM_MAX_SRC][kGemmBM];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * kGemmBN;
    const int m0 = blockIdx.y * kGemmBM;

    // per tile row and source: element offset of the (gathered) source row, -1 past the last row
    if (tid < kGemmBM) {
        const int R = m0 + tid;
        const bool ok = R < g.M;
        const int b = ok ? R / g.rows : 0, r = ok ? R - b * g.rows : 0;
#pragma unroll
        for (int s = 0; s < NLAM_MAX_SRC; ++s) {
            long o = -1;
            if (ok && s < g.nsrc) o = (long)b * g.sbstride[s] + (long)(g.sidx[s] != nullptr ? g.sidx[s][r] : r) * g.swidth[s];
            roff[s][tid] = o;
        }
    }
    __syncthreads();

    float ra[16], rb[16];
    const int kq = tid & 31, r0 = tid >> 5;   // A (and NT B): column kq of rows r0 + 8 i
    const int nq = tid & 127, k0b = tid >> 7;  // NN B: column nq of k rows k0b + 2 i
    auto load_step = [&](int k0) {
        const int k = k0 + kq;
        int s = 0;
        if (g.nsrc > 1 && k >= g.scol0[1]) s = 1;
        if (g.nsrc > 2 && k >= g.scol0[2]) s = 2;
        const float* sp = sel3(g.sptr, s) + (k - (s == 0 ? 0 : (s == 1 ? g.scol0[1] : g.scol0[2])));
        const bool kin = k < g.K;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long o = roff[s][r0 + 8 * i];
            float v = 0.f;
            if (kin && o >= 0) {
                v = sp[o];
                if (g.silu_a) v = silu_f(v);
            }
            ra[i] = v;
        }
        if (NN == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int n = n0 + r0 + 8 * i;
                rb[i] = (kin && n < g.N) ? g.W[(long)n * g.ldw + k] : 0.f;
            }
        } else {
            const int n = n0 + nq;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int kk = k0 + k0b + 2 * i;
                rb[i] = (kk < g.K && n < g.N) ? g.W[(long)kk * g.ldw + n] : 0.f;
            }
        }
    };
    auto store_step = [&]() {
#pragma unroll
        for (int i = 0; i < 16; ++i) As[(r0 + 8 * i) * kGemmLd + kq] = ra[i];
        if (NN == 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) Bs[(r0 + 8 * i) * kGemmLd + kq] = rb[i];
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) Bs[nq * kGemmLd + k0b + 2 * i] = rb[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int j = lane & 31, hi = lane >> 5;
    const int nk = (g.K + kGemmBK - 1) / kGemmBK;
    load_step(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();   // every wave is done with the previous step's tiles
        store_step();
        __syncthreads();
        if (kt + 1 < nk) load_step((kt + 1) * kGemmBK);   // next step's loads in flight under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < kGemmBK / 16; ++kk) {
            // every term of the step in its own registers before the first MFMA (see mma_split_lds)
            BfFrag<NS> fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float* ap = &As[(wm * 64 + i * 32 + j) * kGemmLd + kk * 16 + 8 * hi];
                const float* bp = &Bs[(wn * 64 + i * 32 + j) * kGemmLd + kk * 16 + 8 * hi];
                const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap), a1 = *reinterpret_cast<const f32x4*>(ap + 4);
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
                float xa[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                float xb[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
                fa[i] = split8<NS>(xa);
                fb[i] = split8<NS>(xb);
            }
#pragma unroll
            for (int ord = NS - 1; ord >= 0; --ord)
#pragma unroll
                for (int pa = 0; pa <= ord; ++pa)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int jb = 0; jb < 2; ++jb) acc[i][jb] = MFMA_BF16(fa[i].t[pa], fb[jb].t[ord - pa], acc[i][jb]);
        }
    }

    // ---- epilogue: lane (j, hi) holds column j of rows 8 q + 4 hi + c of each 32 x 32 block ----
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) {
        const int n = n0 + wn * 64 + jb * 32 + j;
        if (n >= g.N) continue;
        int s = 0;   // kEpiScatter: the source this column belongs to
        if (g.epi == kEpiScatter) {
            if (g.ndst > 1 && n >= g.dcol0[1]) s = 1;
            if (g.ndst > 2 && n >= g.dcol0[2]) s = 2;
        }
        const float bias = g.epi == kEpiBias && g.bias != nullptr ? g.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int R = m0 + wm * 64 + i * 32 + 8 * q + 4 * hi + c;
                    if (R >= g.M) continue;
                    const float v = acc[i][jb][4 * q + c];
                    if (g.epi == kEpiBias) {
                        g.C[(long)R * g.N + n] = v + bias;
                    } else if (g.epi == kEpiDsilu) {
                        g.C[(long)R * g.N + n] = g.no_act ? v : v * silu_grad_f(g.z[(long)R * g.N + n]);
                    } else {
                        float* d = sel3(g.dst, s);
                        if (d == nullptr) continue;
                        const int b = R / g.rows, r = R - b * g.rows;
                        const int cs = s == 0 ? 0 : (s == 1 ? g.dcol0[1] : g.dcol0[2]);
                        const int ce = s == 0 ? g.dcol0[1] : (s == 1 ? g.dcol0[2] : g.dcol0[3]);
                        const int w = ce - cs, c0 = n - cs;
                        const int32_t* di = sel3(g.didx, s);
                        float x = v;
                        if (s == 0 && g.g_out != nullptr)
                            x += g.g_out[(long)b * g.out_bstride + (long)(g.out_idx != nullptr ? g.out_idx[r] : r) * w + c0];
                        if (s == 1 && g.gm != nullptr) x += g.gm[(long)R * w + c0];
                        d[(long)b * sel3(g.dbstride, s) + (long)(di != nullptr ? di[r] : r) * w + c0] = x;
                    }
                }
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per row: LayerNorm (two-pass mean / variance), affine, msg = y [+ src1 row], aggregation staging (msg back into
// `z`), out row = msg [+ src0 row] (through out_idx), xhat / rstd for the backward.
__global__ __launch_bounds__(256) void ln_fwd_rows_kernel(const nlam_mlp_fwd_t p, float* z, int keep_msg) {
    const int lane = threadIdx.x & 63;
    const long M = (long)p.batch * p.rows;
    const long R = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (R >= M) return;
    const int d = p.dout;
    const int b = (int)(R / p.rows), r = (int)(R - (long)b * p.rows);
    float* zr = z + R * d;
    float mean = 0.f, rstd = 1.f;
    const bool ln = p.ln_w != nullptr;
    if (ln) {
        float s = 0.f;
        for (int c = lane; c < d; c += 64) s += zr[c];
        mean = wave_sum(s) / (float)d;
        float s2 = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float t = zr[c] - mean;
            s2 += t * t;
        }
        rstd = rsqrtf(wave_sum(s2) / (float)d + p.eps);
        if (p.rstd != nullptr && lane == 0) p.rstd[R] = rstd;
    }
    const bool add0 = (p.flags & NLAM_F_ADD_SRC0) != 0, add1 = (p.flags & NLAM_F_ADD_SRC1) != 0;
    const float* s0 = add0 ? p.src[0].ptr + (long)b * p.src[0].bstride + (long)(p.src[0].idx != nullptr ? p.src[0].idx[r] : r) * p.src[0].width : nullptr;
    const float* s1 = add1 ? p.src[1].ptr + (long)b * p.src[1].bstride + (long)(p.src[1].idx != nullptr ? p.src[1].idx[r] : r) * p.src[1].width : nullptr;
    float* orow = p.out != nullptr ? p.out + (long)b * p.out_bstride + (long)(p.out_idx != nullptr ? p.out_idx[r] : r) * d : nullptr;
    for (int c = lane; c < d; c += 64) {
        float v = zr[c];
        if (ln) {
            const float xh = (v - mean) * rstd;
            if (p.xhat != nullptr) p.xhat[R * d + c] = xh;
            v = xh * p.ln_w[c] + (p.ln_b != nullptr ? p.ln_b[c] : 0.f);
        }
        if (add1) v += s1[c];
        if (keep_msg) zr[c] = v;
        if (orow != nullptr) orow[c] = add0 ? v + s0[c] : v;
    }
}

// One wave per row: g = g_out[out_idx] + g_aggr[receiver] (x inv_deg for the mean), dz2 = LayerNorm backward of g (g itself
// without LayerNorm); gm (if set) keeps g for the residual gradient of source 1 and the dgamma / dbeta partial sums.
__global__ __launch_bounds__(256) void ln_bwd_rows_kernel(const nlam_mlp_bwd_t p, float* dz2, float* gm) {
    const int lane = threadIdx.x & 63;
    const long M = (long)p.batch * p.rows;
    const long R = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (R >= M) return;
    const int d = p.dout;
    const int b = (int)(R / p.rows), r = (int)(R - (long)b * p.rows);
    const float* go = p.g_out != nullptr ? p.g_out + (long)b * p.out_bstride + (long)(p.out_idx != nullptr ? p.out_idx[r] : r) * d : nullptr;
    const float* ga = nullptr;
    float gs = 1.f;
    if (p.g_aggr != nullptr) {
        const int sg = p.seg_of_row[r];
        ga = p.g_aggr + ((long)b * p.nseg_total + sg) * d;
        if (p.flags & NLAM_F_MEAN) gs = p.inv_deg[sg];
    }
    auto grad = [&](int c) { return (go != nullptr ? go[c] : 0.f) + (ga != nullptr ? ga[c] * gs : 0.f); };
    if (p.ln_w != nullptr) {
        const float rstd = p.rstd[R];
        const float* xh = p.xhat + R * d;
        float s1 = 0.f, s2 = 0.f;
        for (int c = lane; c < d; c += 64) {
            const float gx = grad(c) * p.ln_w[c];
            s1 += gx;
            s2 += gx * xh[c];
        }
        const float m1 = wave_sum(s1) / (float)d, m2 = wave_sum(s2) / (float)d;
        for (int c = lane; c < d; c += 64) {
            const float gv = grad(c);
            if (gm != nullptr) gm[R * d + c] = gv;
            dz2[R * d + c] = rstd * (gv * p.ln_w[c] - m1 - xh[c] * m2);
        }
    } else {
        for (int c = lane; c < d; c += 64) {
            const float gv = grad(c);
            if (gm != nullptr) gm[R * d + c] = gv;
            dz2[R * d + c] = gv;
        }
    }
}

// Segment sums over the tile schedule's receivers (as tile_segment_reduce of the fused kernels): for every tile and batch
// item, out[b, s] = scale[s] * sum_{q in rowptr[s] .. rowptr[s+1]} in[b * rows + q], rows in CSR order.  A tile flagged
// NLAM_TILE_SPLIT (the one-pass split mode of graph.build_tile_schedule) is ONE piece of its receiver: it sums its own rows
// row0 .. row0 + nrows and adds that partial sum atomically.  Segments without rows (and every segment of a launch without
// rows) are written as zeros.
__global__ __launch_bounds__(256) void tile_segsum_kernel(const nlam_tile_t* tiles, int rows, const float* in, const int32_t* rowptr,
                                                          const float* scale, float* out, long out_bstride, int w) {
    const int b = blockIdx.y;
    const TileInfo t = get_tile(tiles, blockIdx.x, rows);
    const float* ib = in + (long)b * rows * w;
    float* ob = out + (long)b * out_bstride;
    for (int s = t.seg0; s < t.seg0 + t.nseg; ++s) {
        const int q0 = t.split ? t.row0 : rowptr[s], q1 = t.split ? t.row0 + t.nrows : rowptr[s + 1];
        const float sc = scale != nullptr ? scale[s] : 1.f;
        for (int c = threadIdx.x; c < w; c += blockDim.x) {
            float acc = 0.f;
            for (int q = q0; q < q1; ++q) acc += ib[(long)q * w + c];
            if (t.split)
                atomicAdd(&ob[(long)s * w + c], acc * sc);
            else
                ob[(long)s * w + c] = acc * sc;
        }
    }
}

// vec_partials rows: workgroup k sums rows [k * span, (k + 1) * span) of dz1 (db1), dz2 (db2), gm * xhat (dgamma), gm (dbeta)
// in row order; columns past a width are zeros.
__global__ __launch_bounds__(256) void colsum_partials_kernel(const float* dz1, const float* dz2, const float* gm, const float* xhat,
                                                              long M, long span, int hid, int dout, float* vp, int vs) {
    const long R0 = (long)blockIdx.x * span;
    const long R1 = R0 + span < M ? R0 + span : M;
    float* o = vp + (long)blockIdx.x * 4 * vs;
    for (int c = threadIdx.x; c < vs; c += blockDim.x) {
        float a1 = 0.f, a2 = 0.f, ag = 0.f, ab = 0.f;
        for (long R = R0; R < R1; ++R) {
            if (c < hid) a1 += dz1[R * hid + c];
            if (c < dout) {
                a2 += dz2[R * dout + c];
                if (gm != nullptr) {
                    const float gv = gm[R * dout + c];
                    ab += gv;
                    if (xhat != nullptr) ag += gv * xhat[R * dout + c];
                }
            }
        }
        o[c] = a1;
        o[vs + c] = a2;
        o[2 * vs + c] = ag;
        o[3 * vs + c] = ab;
    }
}

int gemm_terms(uint32_t flags) { return ((flags & NLAM_F_MM_MASK) >> NLAM_F_MM_SHIFT) == 1 ? 1 : 3; }

int32_t gemm_launch(const GemmArgs& g, int ns, int nn, hipStream_t stream) {
    if (g.M == 0 || g.N == 0) return 0;
    const dim3 grid((g.N + kGemmBN - 1) / kGemmBN, (g.M + kGemmBM - 1) / kGemmBM);
    if (grid.y > 65535) return NLAM_EUNSUP;
    void (*kern)(const GemmArgs) = ns == 1 ? (nn ? gemm_kernel<1, 1> : gemm_kernel<1, 0>) : (nn ? gemm_kernel<3, 1> : gemm_kernel<3, 0>);
    hipLaunchKernelGGL(kern, grid, dim3(kGemmThreads), 0, stream, g);
    return (int32_t)hipGetLastError();
}

int32_t segsum_launch(const nlam_tile_t* tiles, int ntiles, int batch, int rows, const float* in, const int32_t* rowptr, const float* scale,
                      float* out, long out_bstride, int w, hipStream_t stream) {
    if (ntiles == 0 || batch == 0) return 0;
    hipLaunchKernelGGL(tile_segsum_kernel, dim3(ntiles, batch), dim3(w >= 256 ? 256 : 64), 0, stream, tiles, rows, in, rowptr, scale, out,
                       out_bstride, w);
    return (int32_t)hipGetLastError();
}

int gemm_kin(const nlam_src_t* src, int nsrc) {
    int k = 0;
    for (int s = 0; s < nsrc; ++s) k += src[s].width;
    return k;
}

// flags this family does not serve (factorised edge MLP, bf16 storage, in-kernel weight gradients, rollout accumulation)
constexpr uint32_t kGemmUnsup = NLAM_F_PRE_ADD | NLAM_F_LEAF_WGRAD | NLAM_F_STORE_BF16 | NLAM_F_ACC_DSRC0;

int32_t gemm_check_common(const nlam_src_t* src, int nsrc, int batch, int rows, int ntiles, int hid, int dout, int ldw1,
                          const float* W1, const float* W2, uint32_t flags) {
    if (nsrc < 1 || nsrc > NLAM_MAX_SRC || batch < 1 || rows < 0 || ntiles < 0 || hid < 1 || dout < 1) return NLAM_EINVAL;
    if (W1 == nullptr || W2 == nullptr) return NLAM_EINVAL;
    long kin = 0;
    for (int s = 0; s < nsrc; ++s) {
        if (src[s].ptr == nullptr || src[s].width < 1 || src[s].bstride < 0) return NLAM_EINVAL;
        kin += src[s].width;
    }
    if (kin > (1L << 30) || (ldw1 != 0 && ldw1 < kin)) return NLAM_EINVAL;
    if ((flags & NLAM_F_ADD_SRC0) && src[0].width != dout) return NLAM_EINVAL;
    if ((flags & NLAM_F_ADD_SRC1) && (nsrc < 2 || src[1].width != dout)) return NLAM_EINVAL;
    if (flags & kGemmUnsup) return NLAM_EUNSUP;
    if ((long)batch * rows > (long)65535 * kGemmBM) return NLAM_EUNSUP;
    return 0;
}

int32_t fwd_gemm_check(const nlam_mlp_fwd_t* p) {
    if (p == nullptr) return NLAM_EINVAL;
    if (const int32_t rc = gemm_check_common(p->src, p->nsrc, p->batch, p->rows, p->ntiles, p->hid, p->dout, p->ldw1, p->W1, p->W2, p->flags))
        return rc;
    if (p->b1 == nullptr || p->b2 == nullptr) return NLAM_EINVAL;
    if (p->ln_w == nullptr && (p->xhat != nullptr || p->ln_b != nullptr)) return NLAM_EINVAL;
    if (p->aggr != nullptr && (p->rowptr == nullptr || p->nseg_total < 1 || ((p->flags & NLAM_F_MEAN) && p->inv_deg == nullptr)))
        return NLAM_EINVAL;
    if (p->ncat != 0) return NLAM_EUNSUP;
    return 0;
}

int32_t bwd_gemm_check(const nlam_mlp_bwd_t* p) {
    if (p == nullptr) return NLAM_EINVAL;
    if (const int32_t rc = gemm_check_common(p->src, p->nsrc, p->batch, p->rows, p->ntiles, p->hid, p->dout, p->ldw1, p->W1, p->W2, p->flags))
        return rc;
    if (p->z1 == nullptr || p->dz1 == nullptr || p->dz2 == nullptr) return NLAM_EINVAL;
    if (p->dz2_ld != 0 && p->dz2_ld != p->dout) return NLAM_EINVAL;
    if (p->ln_w != nullptr && (p->xhat == nullptr || p->rstd == nullptr)) return NLAM_EINVAL;
    if (p->g_aggr != nullptr && (p->seg_of_row == nullptr || p->nseg_total < 1 || ((p->flags & NLAM_F_MEAN) && p->inv_deg == nullptr)))
        return NLAM_EINVAL;
    for (int s = 0; s < p->nsrc; ++s) {
        const int m = p->dmode[s];
        if (m < 0 || m > 3 || (m != 0 && p->dsrc[s] == nullptr)) return NLAM_EINVAL;
        if (m == 3 && p->rowptr == nullptr) return NLAM_EINVAL;
    }
    if (p->vec_partials != nullptr && (p->vec_partials_rows < kGemmPartBlocks || p->vec_stride < p->hid || p->vec_stride < p->dout))
        return NLAM_EINVAL;
    return 0;
}

int64_t fwd_gemm_ws(const nlam_mlp_fwd_t* p) {
    const long M = (long)p->batch * p->rows;
    return M * p->dout + (p->z1 == nullptr ? M * p->hid : 0);
}

bool bwd_gemm_needs_gm(const nlam_mlp_bwd_t* p) { return p->ln_w != nullptr || (p->flags & NLAM_F_ADD_SRC1); }

int64_t bwd_gemm_ws(const nlam_mlp_bwd_t* p) {
    const long M = (long)p->batch * p->rows;
    int64_t n = bwd_gemm_needs_gm(p) ? M * p->dout : 0;
    for (int s = 0; s < p->nsrc; ++s)
        if (p->dmode[s] == 3) n += M * p->src[s].width;
    return n;
}

}  // namespace

extern "C" {

int64_t nlam_mlp_fwd_gemm_workspace_floats(const nlam_mlp_fwd_t* p) {
    if (const int32_t rc = fwd_gemm_check(p)) return rc;
    return fwd_gemm_ws(p);
}

int64_t nlam_mlp_bwd_gemm_workspace_floats(const nlam_mlp_bwd_t* p) {
    if (const int32_t rc = bwd_gemm_check(p)) return rc;
    return bwd_gemm_ws(p);
}

int32_t nlam_mlp_bwd_gemm_blocks(const nlam_mlp_bwd_t* p) {
    (void)p;
    return kGemmPartBlocks;
}

int32_t nlam_mlp_fwd_gemm(const nlam_mlp_fwd_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_mlp_fwd_gemm");
    if (const int32_t rc = fwd_gemm_check(p)) return rc;
    const int64_t need = fwd_gemm_ws(p);
    if (need > 0 && (p->wpack == nullptr || p->wpack_floats < need)) return NLAM_EINVAL;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const long M = (long)p->batch * p->rows;
    const bool aggr = p->aggr != nullptr;
    const int ntiles = p->tiles != nullptr ? p->ntiles : (p->rows + 31) / 32;
    if (M == 0)   // no rows: receivers covered by the tile schedule still get their (zero) aggregate
        return aggr ? segsum_launch(p->tiles, ntiles, p->batch, p->rows, p->wpack, p->rowptr, nullptr, p->aggr,
                                    (long)p->nseg_total * p->dout, p->dout, stream)
                    : 0;
    const int ns = gemm_terms(p->flags);
    const int kin = gemm_kin(p->src, p->nsrc);
    float* msg = p->wpack;
    float* z1 = p->z1 != nullptr ? p->z1 : p->wpack + M * p->dout;

    GemmArgs g = {};
    g.M = (int)M;
    g.rows = p->rows;
    g.K = kin;
    g.nsrc = p->nsrc;
    int col = 0;
    for (int s = 0; s < p->nsrc; ++s) {
        g.sptr[s] = p->src[s].ptr;
        g.sidx[s] = p->src[s].idx;
        g.sbstride[s] = p->src[s].bstride;
        g.swidth[s] = p->src[s].width;
        g.scol0[s] = col;
        col += p->src[s].width;
    }
    g.scol0[p->nsrc] = col;
    g.W = p->W1;
    g.ldw = p->ldw1 != 0 ? p->ldw1 : kin;
    g.N = p->hid;
    g.epi = kEpiBias;
    g.bias = p->b1;
    g.C = z1;
    int32_t rc = gemm_launch(g, ns, 0, stream);
    if (rc != 0) return rc;

    GemmArgs h = {};   // z2 = act(z1) W2^T + b2, into the message buffer
    h.M = (int)M;
    h.rows = p->rows;
    h.K = p->hid;
    h.nsrc = 1;
    h.silu_a = (p->flags & NLAM_F_NO_ACT) ? 0 : 1;
    h.sptr[0] = z1;
    h.sbstride[0] = (long)p->rows * p->hid;
    h.swidth[0] = p->hid;
    h.scol0[1] = p->hid;
    h.W = p->W2;
    h.ldw = p->hid;
    h.N = p->dout;
    h.epi = kEpiBias;
    h.bias = p->b2;
    h.C = msg;
    if ((rc = gemm_launch(h, ns, 0, stream)) != 0) return rc;

    hipLaunchKernelGGL(ln_fwd_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, *p, msg, aggr ? 1 : 0);
    if ((rc = (int32_t)hipGetLastError()) != 0) return rc;
    if (aggr) {
        rc = segsum_launch(p->tiles, ntiles, p->batch, p->rows, msg, p->rowptr, (p->flags & NLAM_F_MEAN) ? p->inv_deg : nullptr, p->aggr,
                           (long)p->nseg_total * p->dout, p->dout, stream);
    }
    return rc;
}

int32_t nlam_mlp_bwd_gemm(const nlam_mlp_bwd_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_mlp_bwd_gemm");
    if (const int32_t rc = bwd_gemm_check(p)) return rc;
    const int64_t need = bwd_gemm_ws(p);
    if (need > 0 && (p->wpack == nullptr || p->wpack_floats < need)) return NLAM_EINVAL;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const long M = (long)p->batch * p->rows;
    const int ns = gemm_terms(p->flags);
    const int kin = gemm_kin(p->src, p->nsrc);
    float* gm = bwd_gemm_needs_gm(p) ? p->wpack : nullptr;
    float* tmp = p->wpack + (gm != nullptr ? M * p->dout : 0);
    int32_t rc = 0;
    if (M > 0) {
        hipLaunchKernelGGL(ln_bwd_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream, *p, p->dz2, gm);
        if ((rc = (int32_t)hipGetLastError()) != 0) return rc;

        GemmArgs h = {};   // dz1 = (dz2 W2) * silu'(z1)
        h.M = (int)M;
        h.rows = p->rows;
        h.K = p->dout;
        h.nsrc = 1;
        h.sptr[0] = p->dz2;
        h.sbstride[0] = (long)p->rows * p->dout;
        h.swidth[0] = p->dout;
        h.scol0[1] = p->dout;
        h.W = p->W2;
        h.ldw = p->hid;
        h.N = p->hid;
        h.epi = kEpiDsilu;
        h.no_act = (p->flags & NLAM_F_NO_ACT) ? 1 : 0;
        h.z = p->z1;
        h.C = p->dz1;
        if ((rc = gemm_launch(h, ns, 1, stream)) != 0) return rc;
    }

    bool any = false;
    GemmArgs g = {};   // dX = dz1 W1 (+ residual gradients), per source
    g.M = (int)M;
    g.rows = p->rows;
    g.K = p->hid;
    g.nsrc = 1;
    g.sptr[0] = p->dz1;
    g.sbstride[0] = (long)p->rows * p->hid;
    g.swidth[0] = p->hid;
    g.scol0[1] = p->hid;
    g.W = p->W1;
    g.ldw = p->ldw1 != 0 ? p->ldw1 : kin;
    g.N = kin;
    g.epi = kEpiScatter;
    g.ndst = p->nsrc;
    float* stage[NLAM_MAX_SRC] = {nullptr, nullptr, nullptr};
    bool staged[NLAM_MAX_SRC] = {false, false, false};   // dmode 3: segment-summed below (also without rows: zeros)
    int col = 0;
    for (int s = 0; s < p->nsrc; ++s) {
        const int w = p->src[s].width;
        g.dcol0[s] = col;
        col += w;
        const int m = p->dmode[s];
        if (m == 0) continue;
        any = true;
        if (m == 1) {
            g.dst[s] = p->dsrc[s];
            g.dbstride[s] = p->dsrc_bstride[s];
            g.didx[s] = p->src[s].idx;
        } else if (m == 2) {
            g.dst[s] = p->dsrc[s];
            g.dbstride[s] = p->dsrc_bstride[s];
        } else {
            stage[s] = tmp;
            staged[s] = true;
            tmp += M * w;
            g.dst[s] = stage[s];
            g.dbstride[s] = (long)p->rows * w;
        }
    }
    g.dcol0[p->nsrc] = col;
    if ((p->flags & NLAM_F_ADD_SRC0) && p->g_out != nullptr) {
        g.g_out = p->g_out;
        g.out_idx = p->out_idx;
        g.out_bstride = p->out_bstride;
    }
    if (p->flags & NLAM_F_ADD_SRC1) g.gm = gm;
    if (any && M > 0 && (rc = gemm_launch(g, ns, 1, stream)) != 0) return rc;
    const int ntiles = p->tiles != nullptr ? p->ntiles : (p->rows + 31) / 32;
    for (int s = 0; s < p->nsrc; ++s)
        if (staged[s] &&
            (rc = segsum_launch(p->tiles, ntiles, p->batch, p->rows, stage[s], p->rowptr, nullptr, p->dsrc[s], p->dsrc_bstride[s],
                                p->src[s].width, stream)) != 0)
            return rc;

    if (p->vec_partials != nullptr) {
        const long span = (M + kGemmPartBlocks - 1) / kGemmPartBlocks;
        hipLaunchKernelGGL(colsum_partials_kernel, dim3(kGemmPartBlocks), dim3(256), 0, stream, p->dz1, p->dz2, gm,
                           p->ln_w != nullptr ? p->xhat : nullptr, M, span, p->hid, p->dout, p->vec_partials, p->vec_stride);
        rc = (int32_t)hipGetLastError();
    }
    return rc;
}

}  // extern "C"
