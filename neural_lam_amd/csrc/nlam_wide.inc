// nlam_wide.inc -- workgroup-cooperative kernels for hidden / output widths in (64, 512].
// Included inside the anonymous namespace of nlam_hip.hip (shares its helpers).
//
// Why a second kernel family: at d > 64 a single wave can no longer hold a 32-row
// tile of the whole MLP in registers (d/2 accumulators per GEMM) and the weights no
// longer fit the CU's 160 KB of LDS (W1 alone is 192 KB at d = 128).  So
//  * a *workgroup* (NWV waves) owns the 32-row tile; the waves split the FEATURE
//    dimension block-cyclically: wave w owns the 32-feature blocks w, w + NWV, ...
//    (FB of them) of whatever the current GEMM produces;
//  * weights stay in HBM/L2 in the packed A-operand order (one coalesced 1-KiB
//    dwordx4 load per wave = the A operands of four MFMAs), written once per launch by
//    pack_a_kernel; every weight element is used by exactly one wave of the
//    workgroup, so staging it in LDS would buy nothing.  The A stream is prefetched one
//    "quad" (32 K-columns = 16 MFMAs per block) ahead, across phase and tile boundaries;
//  * what the waves *share* are the B operands: the gathered input rows (staged in
//    K-chunks of 128 columns, double buffered) and the 32 x d hidden tile between the
//    two GEMMs; both live in LDS with a (width + 4) row stride = conflict-free
//    ds_read_b128 for the chunk layout of mma_chunk;
//  * LayerNorm row statistics cross the waves through a tiny LDS array, column sums
//    (bias / LN-affine gradients) are taken with thread = column from the shared tiles.
// The tile schedule (whole receivers per tile), the parameter structs and the output
// modes are exactly those of the narrow kernels.

constexpr int kWideKC = 128;          // K columns per staged chunk
constexpr int kXS = kWideKC + 4;      // staged-input row stride (floats)
constexpr int kMaxWide = 512;

struct pack_job_t {
    const float* W;
    long ldm, ldk;      // A[m][k] = W[m * ldm + k * ldk]
    int M, MB, Kw;      // real rows, 32-row blocks, real K columns
    int T, t0;          // K-groups per block row of the destination, first group of this job
    float* dst;
};
struct pack_jobs_t {
    pack_job_t job[4];
    int njobs;
};

#if NLAM_IN_TU(3)   // no template: emitted where it is defined, so only in the slice of launch_pack
// dst[((mb * T + t0 + t) * 64 + lane) * 4 + c] = A[mb*32 + (lane & 31)][8t + 4(lane >> 5) + c]
// for t < round_up(ceil(Kw / 8), 4); zero outside M x Kw.
__global__ void pack_a_kernel(const pack_jobs_t jobs) {
    if ((int)blockIdx.y >= jobs.njobs) return;
    const pack_job_t jb = jobs.job[blockIdx.y];
    const int ng = round_up((jb.Kw + 7) >> 3, 4);
    const long total = (long)jb.MB * ng * 64;
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(s & 63);
        const long rest = s >> 6;
        const int t = (int)(rest % ng);
        const int mb = (int)(rest / ng);
        const int m = mb * 32 + (lane & 31);
        const int kb = 8 * t + 4 * (lane >> 5);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < jb.M) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (kb + c < jb.Kw) v[c] = jb.W[(long)m * jb.ldm + (long)(kb + c) * jb.ldk];
        }
        *reinterpret_cast<f32x4*>(&jb.dst[(((size_t)mb * jb.T + jb.t0 + t) * 64 + lane) * 4]) = v;
    }
}
#endif

template <typename P>
__device__ __forceinline__ nlam_src_t get_src(const P& p, int s) {
    return s == 0 ? p.src[0] : (s == 1 ? p.src[1] : p.src[2]);
}

// A operands of one quad (4 K-groups) for the wave's FB blocks
template <int FB>
struct AQuad {
    f32x4 a[4][FB];
};

struct APhase {
    const float* A;   // packed matrix
    int T;            // K-groups per block row
    int nblk;         // 32-row blocks it has
};

template <int NWV, int FB>
__device__ __forceinline__ void load_aquad(AQuad<FB>& r, const APhase ph, int q, int wave, int lane) {
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
        const int blk = wave + fb * NWV;
        if (blk < ph.nblk) {
            const float* base = ph.A + (((size_t)blk * ph.T + 4 * q) * 64 + lane) * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g) r.a[g][fb] = *reinterpret_cast<const f32x4*>(base + g * 256);
        }
    }
}

// 16 MFMAs per owned block: acc[fb] += A(quad) . x(quad)
template <int NWV, int FB>
__device__ __forceinline__ void mma_aquad(f32x16 (&acc)[FB], const AQuad<FB>& r, const f32x4 (&x)[4], int nblk, int wave) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                if (wave + fb * NWV < nblk) acc[fb] = MFMA32(r.a[g][fb][c], x[g][c], acc[fb]);
            }
        }
    }
}

// B operands of quad q from a shared LDS tile with row stride S
__device__ __forceinline__ void load_xquad(f32x4 (&x)[4], const float* tile, int S, int q, int j, int hi) {
#pragma unroll
    for (int g = 0; g < 4; ++g) x[g] = *reinterpret_cast<const f32x4*>(&tile[j * S + 8 * (4 * q + g) + 4 * hi]);
}

template <int FB>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[FB]) {
#pragma unroll
    for (int fb = 0; fb < FB; ++fb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[fb][r] = 0.f;
}

// guarded 4-float parameter fetch (bias / gamma / beta) for columns [c0, c0 + 4)
__device__ __forceinline__ f32x4 load_vec4(const float* v, int n, int c0, float fill) {
    f32x4 r = {fill, fill, fill, fill};
    if (v != nullptr) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c0 + c < n) r[c] = v[c0 + c];
    }
    return r;
}

// Segment-sum a shared 32 x w tile over the tile's receivers with all NT threads
// (thread -> (receiver, column), consecutive threads = consecutive columns).
__device__ __forceinline__ void coop_segment_reduce(const float* tile, int S, const TileInfo& tl, const int32_t* rowptr,
                                                    const float* inv_deg, float* out_b, int w, int tid, int NT) {
    const int total = tl.nseg * w;
    for (int idx = tid; idx < total; idx += NT) {
        const int sg = idx / w;
        const int c = idx - sg * w;
        const int r = tl.seg0 + sg;
        int lo = 0, hi_ = tl.nrows;
        if (!tl.split) {
            lo = rowptr[r] - tl.row0;
            hi_ = rowptr[r + 1] - tl.row0;
        }
        float s = 0.f;
        for (int q = lo; q < hi_; ++q) s += tile[q * S + c];
        if (inv_deg != nullptr) s *= inv_deg[r];
        float* dst = out_b + (size_t)r * w + c;
        if (tl.split)
            atomicAdd(dst, s);
        else
            *dst = s;
    }
}

__device__ __forceinline__ float tile_colsum32(const float* tile, int S, int c) {
    float s = 0.f;
#pragma unroll 8
    for (int q = 0; q < 32; ++q) s += tile[q * S + c];
    return s;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// (the body takes the workgroup's index and count within ITS launch: a grouped launch -- several MLPs of one shape in one grid,
// mlp_fwd_wide_group_kernel -- binds every workgroup to one member)
template <int NWV, int FB>
__device__ __forceinline__ void mlp_fwd_wide_body(const nlam_mlp_fwd_t& p, const int bid, const int nb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NT = NWV * 64;
    constexpr int SI = (32 * (kWideKC / 4) + NT - 1) / NT;   // staged float4 per thread per chunk

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hi = lane >> 5;

    const int HBT = (p.hid + 31) >> 5, OBT = (p.dout + 31) >> 5;
    const int WS = (HBT > OBT ? HBT : OBT) * 32 + 4;
    int NQ1 = 0;
    for (int s = 0; s < p.nsrc; ++s) NQ1 += (get_src(p, s).width + 31) >> 5;
    const APhase ph1 = {p.wpack, NQ1 * 4, HBT};
    const APhase ph2 = {p.wpack + (size_t)HBT * NQ1 * 1024, HBT * 4, OBT};

    float* X = smem;                                     // 2 x 32 x kXS
    float* H = X + 2 * 32 * kXS;                         // 32 x WS   (hidden tile, later message tile)
    float* red = H + 32 * WS;                            // 2 x NWV x 32
    int* ridx = reinterpret_cast<int*>(red + 2 * NWV * 32);  // NLAM_MAX_SRC x 32 gathered row ids (-1 = no row)

    const bool has_ln = p.ln_w != nullptr;
    const float inv_dout = 1.f / (float)p.dout;

    AQuad<FB> an;
    load_aquad<NWV, FB>(an, ph1, 0, wave, lane);

    const long total_tiles = (long)p.ntiles * p.batch;
    for (long gt = bid; gt < total_tiles; gt += nb) {
        const int b = (int)(gt / p.ntiles);
        const int ti = (int)(gt % p.ntiles);
        const TileInfo tl = get_tile(p.tiles, ti, p.rows);
        const bool valid = j < tl.nrows;
        const int prow = tl.row0 + j;

        // ---- gathered row ids of the tile ----
        if (tid < NLAM_MAX_SRC * 32) {
            const int s = tid >> 5, r = tid & 31;
            int v = -1;
            if (s < p.nsrc && r < tl.nrows) {
                const nlam_src_t S = get_src(p, s);
                v = S.idx != nullptr ? S.idx[tl.row0 + r] : tl.row0 + r;
            }
            ridx[tid] = v;
        }
        __syncthreads();

        auto stage_load = [&](int s, int c0, f32x4(&v)[SI]) {
            const nlam_src_t S = get_src(p, s);
            const int nc = min(kWideKC, S.width - c0);
            const int nvp = ((nc + 31) >> 5) * 8;          // float4 slots per row incl. zero padding to the quad
            const bool vec_ok = (S.width & 3) == 0;
#pragma unroll
            for (int k = 0; k < SI; ++k) {
                const int item = tid + k * NT;
                f32x4 val = {0.f, 0.f, 0.f, 0.f};
                if (item < 32 * nvp) {
                    const int r = item / nvp, q = item - r * nvp;
                    const int rid = ridx[s * 32 + r];
                    if (rid >= 0 && 4 * q < nc) {
                        const float* row = S.ptr + (long)b * S.bstride + (long)rid * S.width + c0 + 4 * q;
                        if (vec_ok) {
                            val = *reinterpret_cast<const f32x4*>(row);
                        } else {
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                if (4 * q + c < nc) val[c] = row[c];
                        }
                    }
                }
                v[k] = val;
            }
        };
        auto stage_store = [&](float* Xb, int s, int c0, const f32x4(&v)[SI]) {
            const nlam_src_t S = get_src(p, s);
            const int nc = min(kWideKC, S.width - c0);
            const int nvp = ((nc + 31) >> 5) * 8;
#pragma unroll
            for (int k = 0; k < SI; ++k) {
                const int item = tid + k * NT;
                if (item < 32 * nvp) {
                    const int r = item / nvp, q = item - r * nvp;
                    *reinterpret_cast<f32x4*>(&Xb[r * kXS + 4 * q]) = v[k];
                }
            }
        };

        // ---- GEMM1 over the staged chunks ----
        f32x16 acc[FB];
        zero_acc<FB>(acc);
        f32x4 sv[SI];
        int cs = 0, cc0 = 0, buf = 0, q = 0;
        stage_load(0, 0, sv);
        stage_store(X, 0, 0, sv);
        __syncthreads();
        while (cs < p.nsrc) {
            const int wcur = get_src(p, cs).width;
            int ns = cs, nc0 = cc0 + kWideKC;
            if (nc0 >= wcur) {
                ns = cs + 1;
                nc0 = 0;
            }
            const bool has_next = ns < p.nsrc;
            if (has_next) stage_load(ns, nc0, sv);
            const int nq = (min(kWideKC, wcur - cc0) + 31) >> 5;
            const float* Xb = X + buf * 32 * kXS;
            for (int ql = 0; ql < nq; ++ql) {
                const AQuad<FB> ac = an;
                if (q + 1 < NQ1)
                    load_aquad<NWV, FB>(an, ph1, q + 1, wave, lane);
                else
                    load_aquad<NWV, FB>(an, ph2, 0, wave, lane);
                f32x4 x[4];
                load_xquad(x, Xb, kXS, ql, j, hi);
                mma_aquad<NWV, FB>(acc, ac, x, HBT, wave);
                ++q;
            }
            if (has_next) stage_store(X + (buf ^ 1) * 32 * kXS, ns, nc0, sv);
            __syncthreads();
            buf ^= 1;
            cs = ns;
            cc0 = nc0;
        }

        // ---- bias, save pre-activation, SiLU -> shared hidden tile ----
        {
            float* z1row = p.z1 != nullptr ? p.z1 + ((size_t)b * p.rows + prow) * p.hid : nullptr;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < HBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        const int c0 = 8 * t + 4 * hi;
                        const f32x4 z = acc_chunk(acc[fb], tt) + load_vec4(p.b1, p.hid, c0, 0.f);
                        if (z1row != nullptr) store_chunk(z1row, p.hid, t, hi, valid, z);
                        f32x4 h;
#pragma unroll
                        for (int c = 0; c < 4; ++c) h[c] = (p.flags & NLAM_F_NO_ACT) ? z[c] : silu_f(z[c]);
                        *reinterpret_cast<f32x4*>(&H[j * WS + c0]) = h;
                    }
                }
            }
        }
        __syncthreads();

        // ---- GEMM2 from the hidden tile ----
        zero_acc<FB>(acc);
        for (int q2 = 0; q2 < HBT; ++q2) {
            const AQuad<FB> ac = an;
            if (q2 + 1 < HBT)
                load_aquad<NWV, FB>(an, ph2, q2 + 1, wave, lane);
            else
                load_aquad<NWV, FB>(an, ph1, 0, wave, lane);   // first quad of the next tile
            f32x4 x[4];
            load_xquad(x, H, WS, q2, j, hi);
            mma_aquad<NWV, FB>(acc, ac, x, OBT, wave);
        }

        // ---- bias 2 + LayerNorm over the real dout features (row statistics across the waves) ----
        float sum = 0.f;
#pragma unroll
        for (int fb = 0; fb < FB; ++fb) {
            const int blk = wave + fb * NWV;
            if (blk < OBT) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int c0 = 8 * (blk * 4 + tt) + 4 * hi;
                    const f32x4 bias = load_vec4(p.b2, p.dout, c0, 0.f);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float v = acc[fb][4 * tt + c] + bias[c];
                        acc[fb][4 * tt + c] = v;
                        sum += (c0 + c < p.dout) ? v : 0.f;
                    }
                }
            }
        }
        if (has_ln) {
            sum = row_allreduce(sum);
            if (hi == 0) red[wave * 32 + j] = sum;
            __syncthreads();   // also: every wave is done reading the hidden tile
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < NWV; ++w) tot += red[w * 32 + j];
            const float mean = tot * inv_dout;
            float sq = 0.f;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < OBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int c0 = 8 * (blk * 4 + tt) + 4 * hi;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float dlt = acc[fb][4 * tt + c] - mean;
                            acc[fb][4 * tt + c] = dlt;
                            sq += (c0 + c < p.dout) ? dlt * dlt : 0.f;
                        }
                    }
                }
            }
            sq = row_allreduce(sq);
            if (hi == 0) red[(NWV + wave) * 32 + j] = sq;
            __syncthreads();
            float tot2 = 0.f;
#pragma unroll
            for (int w = 0; w < NWV; ++w) tot2 += red[(NWV + w) * 32 + j];
            const float rstd = rsqrtf(tot2 * inv_dout + p.eps);
            if (p.rstd != nullptr && valid && hi == 0 && wave == 0) p.rstd[(size_t)b * p.rows + prow] = rstd;
            float* xrow = p.xhat != nullptr ? p.xhat + ((size_t)b * p.rows + prow) * p.dout : nullptr;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < OBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        const int c0 = 8 * t + 4 * hi;
                        f32x4 xh;
#pragma unroll
                        for (int c = 0; c < 4; ++c) xh[c] = acc[fb][4 * tt + c] * rstd;
                        if (xrow != nullptr) store_chunk(xrow, p.dout, t, hi, valid, xh);
                        const f32x4 g = load_vec4(p.ln_w, p.dout, c0, 1.f);
                        const f32x4 be = load_vec4(p.ln_b, p.dout, c0, 0.f);
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[fb][4 * tt + c] = xh[c] * g[c] + be[c];
                    }
                }
            }
        } else {
            __syncthreads();   // every wave is done reading the hidden tile (it becomes the message tile)
        }

        // ---- msg = mlp [+ src1]; aggregate; out = msg [+ src0] ----
        {
            const float* srow0 = nullptr;
            const float* srow1 = nullptr;
            if (valid) {
                srow0 = p.src[0].ptr + (long)b * p.src[0].bstride + (long)ridx[j] * p.src[0].width;
                if (p.nsrc > 1) srow1 = p.src[1].ptr + (long)b * p.src[1].bstride + (long)ridx[32 + j] * p.src[1].width;
            }
            float* orow = nullptr;
            if (p.out != nullptr && valid) {
                const long oidx = p.out_idx != nullptr ? p.out_idx[prow] : prow;
                orow = p.out + (long)b * p.out_bstride + oidx * (long)p.dout;
            }
            // all residual chunks of the row are requested before its first store (a load behind a store waits for the
            // store's acknowledgement: interleaved they were FB x 4 such round trips per tile)
            const bool add0 = (p.flags & NLAM_F_ADD_SRC0) != 0 && orow != nullptr;
            const bool add1 = (p.flags & NLAM_F_ADD_SRC1) != 0;
            f32x4 res0[FB][4], res1[FB][4];
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    res0[fb][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    res1[fb][tt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (blk < OBT) {
                        if (add1) res1[fb][tt] = load_chunk(srow1, p.dout, blk * 4 + tt, hi, valid);
                        if (add0) res0[fb][tt] = load_chunk(srow0, p.dout, blk * 4 + tt, hi, valid);
                    }
                }
            }
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < OBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        f32x4 m = acc_chunk(acc[fb], tt) + res1[fb][tt];
                        if (p.aggr != nullptr) {
                            if (!valid) m = f32x4{0.f, 0.f, 0.f, 0.f};
                            *reinterpret_cast<f32x4*>(&H[j * WS + 8 * t + 4 * hi]) = m;
                        }
                        if (orow != nullptr) store_chunk(orow, p.dout, t, hi, valid, m + res0[fb][tt]);
                    }
                }
            }
        }
        if (p.aggr != nullptr) {
            __syncthreads();
            coop_segment_reduce(H, WS, tl, p.rowptr, (p.flags & NLAM_F_MEAN) ? p.inv_deg : nullptr,
                                p.aggr + (size_t)b * p.nseg_total * p.dout, p.dout, tid, NT);
        }
        __syncthreads();   // tile end: X / H / ridx are reused by the next tile
    }
}

template <int NWV, int FB>
__global__ __launch_bounds__(NWV * 64) void mlp_fwd_wide_kernel(const nlam_mlp_fwd_t p) {
    mlp_fwd_wide_body<NWV, FB>(p, xcd_slot((int)blockIdx.x, (int)gridDim.x), (int)gridDim.x);
}

// Grouped launch (nlam_mlp_fwd_group with wide members): the chunks of a SplitMLPs layer (hi_lam_parallel.py:127-143) are
// 3 .. 206 tiles each -- a launch apiece leaves most of the chip idle for one tile's latency; one grid runs them side by side.
struct fwd_wide_group_t {
    nlam_mlp_fwd_t g[NLAM_MAX_GROUP];
    int n;
    int first[NLAM_MAX_GROUP + 1];   // first workgroup of each member; first[n] = grid size
};
template <int NWV, int FB>
__global__ __launch_bounds__(NWV * 64) void mlp_fwd_wide_group_kernel(const fwd_wide_group_t G) {
    int gi = 0;
#pragma unroll
    for (int k = 1; k < NLAM_MAX_GROUP; ++k)
        if (k < G.n && (int)blockIdx.x >= G.first[k]) gi = k;
    mlp_fwd_wide_body<NWV, FB>(G.g[gi], (int)blockIdx.x - G.first[gi], G.first[gi + 1] - G.first[gi]);
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <int NWV, int FB>
__device__ __forceinline__ void mlp_bwd_wide_body(const nlam_mlp_bwd_t& p, const int bid, const int nb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NT = NWV * 64;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hi = lane >> 5;

    const int HBT = (p.hid + 31) >> 5, OBT = (p.dout + 31) >> 5;
    int maxb = HBT > OBT ? HBT : OBT;
    // phases of the A stream: dh = W2^T dz2, then one per source with a data gradient
    const APhase ph0 = {p.wpack, OBT * 4, HBT};
    APhase phs[NLAM_MAX_SRC];
    bool act[NLAM_MAX_SRC];
    {
        size_t off = (size_t)HBT * OBT * 1024;
#pragma unroll
        for (int s = 0; s < NLAM_MAX_SRC; ++s) {
            act[s] = s < p.nsrc && p.dmode[s] != 0;
            const int SB = (p.src[s].width + 31) >> 5;
            phs[s] = {p.wpack + off, HBT * 4, SB};
            if (act[s]) {
                off += (size_t)SB * HBT * 1024;
                if (p.dmode[s] == 3 && SB > maxb) maxb = SB;
            }
        }
    }
    // first phase at or after source s0 (wraps to the next tile's phase 0)
    auto phase_from = [&](int s0) {
        APhase nxt = ph0;
        if (s0 <= 2 && act[2]) nxt = phs[2];
        if (s0 <= 1 && act[1]) nxt = phs[1];
        if (s0 <= 0 && act[0]) nxt = phs[0];
        return nxt;
    };
    const int WS = maxb * 32 + 4;
    float* T0 = smem;                     // 32 x WS
    float* T1 = T0 + 32 * WS;             // 32 x WS
    float* red = T1 + 32 * WS;            // 2 x NWV x 32

    const bool has_ln = p.ln_w != nullptr;
    const float inv_dout = 1.f / (float)p.dout;

    // thread = column accumulators of db1, db2, dgamma, dbeta
    float acc_db1 = 0.f, acc_db2 = 0.f, acc_dg = 0.f, acc_dbt = 0.f;

    AQuad<FB> an;
    load_aquad<NWV, FB>(an, ph0, 0, wave, lane);

    const long total_tiles = (long)p.ntiles * p.batch;
    for (long gt = bid; gt < total_tiles; gt += nb) {
        const int b = (int)(gt / p.ntiles);
        const int ti = (int)(gt % p.ntiles);
        const TileInfo tl = get_tile(p.tiles, ti, p.rows);
        const bool valid = j < tl.nrows;
        const int prow = tl.row0 + j;
        const size_t srow_id = (size_t)b * p.rows + prow;

        const float* grow = nullptr;
        if (p.g_out != nullptr && valid) {
            const long oidx = p.out_idx != nullptr ? p.out_idx[prow] : prow;
            grow = p.g_out + (long)b * p.out_bstride + oidx * (long)p.dout;
        }
        const float* garow = nullptr;
        float gscale = 1.f;
        if (p.g_aggr != nullptr && valid) {
            const int sg = p.seg_of_row[prow];
            garow = p.g_aggr + ((size_t)b * p.nseg_total + sg) * p.dout;
            if (p.flags & NLAM_F_MEAN) gscale = p.inv_deg[sg];
        }
        auto dmsg_chunk = [&](int t) {
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (grow != nullptr) g += load_chunk(grow, p.dout, t, hi, true);
            if (garow != nullptr) g += load_chunk(garow, p.dout, t, hi, true) * gscale;
            return g;
        };
        const float* xrow = (has_ln && valid) ? p.xhat + srow_id * p.dout : nullptr;
        const float rstd = (has_ln && valid) ? p.rstd[srow_id] : 0.f;

        // ---- phase A: dmsg, LayerNorm backward, dz2 ----
        f32x16 dz[FB];
        zero_acc<FB>(dz);
        // z1 of the tile (used behind the dh GEMM of phase B): requested now, ahead of every store of this tile
        f32x4 zq[FB][4];
        {
            const float* zrow = valid ? p.z1 + srow_id * p.hid : nullptr;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
                    zq[fb][tt] = load_chunk(zrow, p.hid, (wave + fb * NWV) * 4 + tt, hi, valid && wave + fb * NWV < HBT);
        }
        if (has_ln) {
            f32x4 xh[FB][4];
            float m1 = 0.f, m2 = 0.f;
            // requests first (each load_chunk is a branch the scheduler does not move code across: with the arithmetic in
            // between, every chunk's four loads were waited for before the next chunk's were issued)
            f32x4 gq[FB][4], aq[FB][4], gmq[FB][4];
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int t = blk * 4 + tt;
                    gq[fb][tt] = load_chunk(grow, p.dout, t, hi, blk < OBT && grow != nullptr);
                    aq[fb][tt] = load_chunk(garow, p.dout, t, hi, blk < OBT && garow != nullptr);
                    xh[fb][tt] = load_chunk(xrow, p.dout, t, hi, blk < OBT && valid);
                    gmq[fb][tt] = load_vec4(p.ln_w, p.dout, blk < OBT ? 8 * t + 4 * hi : p.dout, 0.f);
                }
            }
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < OBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        const int c0 = 8 * t + 4 * hi;
                        const f32x4 g = gq[fb][tt] + aq[fb][tt] * gscale;
                        const f32x4 gm = gmq[fb][tt];
                        *reinterpret_cast<f32x4*>(&T0[j * WS + c0]) = g;
                        *reinterpret_cast<f32x4*>(&T1[j * WS + c0]) = g * xh[fb][tt];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float gy = g[c] * gm[c];
                            dz[fb][4 * tt + c] = gy;
                            m1 += gy;
                            m2 += gy * xh[fb][tt][c];
                        }
                    }
                }
            }
            m1 = row_allreduce(m1);
            m2 = row_allreduce(m2);
            if (hi == 0) {
                red[wave * 32 + j] = m1;
                red[(NWV + wave) * 32 + j] = m2;
            }
            __syncthreads();
            if (tid < p.dout) {
                acc_dbt += tile_colsum32(T0, WS, tid);
                acc_dg += tile_colsum32(T1, WS, tid);
            }
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int w = 0; w < NWV; ++w) {
                t1 += red[w * 32 + j];
                t2 += red[(NWV + w) * 32 + j];
            }
            t1 *= inv_dout;
            t2 *= inv_dout;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < OBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int c0 = 8 * (blk * 4 + tt) + 4 * hi;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float v = rstd * (dz[fb][4 * tt + c] - t1 - xh[fb][tt][c] * t2);
                            dz[fb][4 * tt + c] = (valid && c0 + c < p.dout) ? v : 0.f;
                        }
                    }
                }
            }
            __syncthreads();   // column sums of T0 / T1 are done
        } else {
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < OBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const f32x4 g = dmsg_chunk(blk * 4 + tt);   // (no LayerNorm: output_map only -- left chunk by chunk)
#pragma unroll
                        for (int c = 0; c < 4; ++c) dz[fb][4 * tt + c] = g[c];
                    }
                }
            }
        }
        {
            float* drow = p.dz2 != nullptr ? p.dz2 + srow_id * p.dout : nullptr;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < OBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        const f32x4 v = acc_chunk(dz[fb], tt);
                        if (drow != nullptr) store_chunk(drow, p.dout, t, hi, valid, v);
                        *reinterpret_cast<f32x4*>(&T0[j * WS + 8 * t + 4 * hi]) = v;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < p.dout) acc_db2 += tile_colsum32(T0, WS, tid);

        // ---- phase B: dh = W2^T dz2 ; dz1 = dh * silu'(z1) ----
        zero_acc<FB>(dz);
        for (int q = 0; q < OBT; ++q) {
            const AQuad<FB> ac = an;
            if (q + 1 < OBT)
                load_aquad<NWV, FB>(an, ph0, q + 1, wave, lane);
            else
                load_aquad<NWV, FB>(an, phase_from(0), 0, wave, lane);
            f32x4 x[4];
            load_xquad(x, T0, WS, q, j, hi);
            mma_aquad<NWV, FB>(dz, ac, x, HBT, wave);
        }
        {
            float* drow = p.dz1 != nullptr ? p.dz1 + srow_id * p.hid : nullptr;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < HBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        const f32x4 z = zq[fb][tt];
                        f32x4 v;
#pragma unroll
                        for (int c = 0; c < 4; ++c) v[c] = valid ? dz[fb][4 * tt + c] * ((p.flags & NLAM_F_NO_ACT) ? 1.f : silu_grad_f(z[c])) : 0.f;
                        if (drow != nullptr) store_chunk(drow, p.hid, t, hi, valid, v);
                        *reinterpret_cast<f32x4*>(&T1[j * WS + 8 * t + 4 * hi]) = v;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < p.hid) acc_db1 += tile_colsum32(T1, WS, tid);

        // ---- phase C: dx_s = W1_s^T dz1 per source ----
#pragma unroll
        for (int s = 0; s < NLAM_MAX_SRC; ++s) {
            if (!act[s]) continue;
            const nlam_src_t S = p.src[s];
            const int mode = p.dmode[s];
            float* dbase = p.dsrc[s];
            const long dbstride = p.dsrc_bstride[s];
            const int w = S.width;
            const int SB = phs[s].nblk;
            zero_acc<FB>(dz);
            for (int q = 0; q < HBT; ++q) {
                const AQuad<FB> ac = an;
                if (q + 1 < HBT)
                    load_aquad<NWV, FB>(an, phs[s], q + 1, wave, lane);
                else
                    load_aquad<NWV, FB>(an, phase_from(s + 1), 0, wave, lane);
                f32x4 x[4];
                load_xquad(x, T1, WS, q, j, hi);
                mma_aquad<NWV, FB>(dz, ac, x, SB, wave);
            }
            const bool add_gout = (s == 0) && (p.flags & NLAM_F_ADD_SRC0) && p.g_out != nullptr;
            const bool add_gmsg = (s == 1) && (p.flags & NLAM_F_ADD_SRC1);
            float* drow = nullptr;
            if (valid) {
                if (mode == 1) {
                    const long ridx = S.idx != nullptr ? S.idx[prow] : prow;
                    drow = dbase + (long)b * dbstride + ridx * (long)w;
                } else if (mode == 2) {
                    drow = dbase + srow_id * w;
                }
            }
            f32x4 rs[FB][4];   // residual terms: every load of the row ahead of its first store
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    f32x4 r = {0.f, 0.f, 0.f, 0.f};
                    if (blk < SB) {
                        if (add_gout && grow != nullptr) r += load_chunk(grow, p.dout, blk * 4 + tt, hi, true);
                        if (add_gmsg) r += dmsg_chunk(blk * 4 + tt);
                    }
                    rs[fb][tt] = r;
                }
            }
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = wave + fb * NWV;
                if (blk < SB) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        f32x4 v = acc_chunk(dz[fb], tt) + rs[fb][tt];
                        if (mode == 3) {
                            if (!valid) v = f32x4{0.f, 0.f, 0.f, 0.f};
                            *reinterpret_cast<f32x4*>(&T0[j * WS + 8 * t + 4 * hi]) = v;
                        } else {
                            store_chunk(drow, w, t, hi, valid, v);
                        }
                    }
                }
            }
            if (mode == 3) {
                __syncthreads();
                coop_segment_reduce(T0, WS, tl, p.rowptr, nullptr, dbase + (long)b * dbstride, w, tid, NT);
                __syncthreads();
            }
        }
        __syncthreads();   // tile end: T0 / T1 are rewritten by the next tile
    }

    if (p.vec_partials != nullptr) {
        float* vp = p.vec_partials + (size_t)bid * 4 * p.vec_stride;
        for (int c = tid; c < p.vec_stride; c += NT) {
            const bool mine = c == tid;
            vp[0 * p.vec_stride + c] = (mine && c < p.hid) ? acc_db1 : 0.f;
            vp[1 * p.vec_stride + c] = (mine && c < p.dout) ? acc_db2 : 0.f;
            vp[2 * p.vec_stride + c] = (mine && c < p.dout) ? acc_dg : 0.f;
            vp[3 * p.vec_stride + c] = (mine && c < p.dout) ? acc_dbt : 0.f;
        }
    }
}

template <int NWV, int FB>
__global__ __launch_bounds__(NWV * 64) void mlp_bwd_wide_kernel(const nlam_mlp_bwd_t p) {
    mlp_bwd_wide_body<NWV, FB>(p, xcd_slot((int)blockIdx.x, (int)gridDim.x), (int)gridDim.x);
}

struct bwd_wide_group_t {
    nlam_mlp_bwd_t g[NLAM_MAX_GROUP];
    int n;
    int first[NLAM_MAX_GROUP + 1];
};
template <int NWV, int FB>
__global__ __launch_bounds__(NWV * 64) void mlp_bwd_wide_group_kernel(const bwd_wide_group_t G) {
    int gi = 0;
#pragma unroll
    for (int k = 1; k < NLAM_MAX_GROUP; ++k)
        if (k < G.n && (int)blockIdx.x >= G.first[k]) gi = k;
    mlp_bwd_wide_body<NWV, FB>(G.g[gi], (int)blockIdx.x - G.first[gi], G.first[gi + 1] - G.first[gi]);
}

// ---------------------------------------------------------------------------
// weight gradients, windowed:  C[m][n] = sum_rows A[row][m] * B[row][n]
// grid = (row slices, 128 x 128 output windows); 4 waves, each a 2 x 2 set of 32 x 32
// blocks.  Same LDS-DMA double-buffered row streaming as wgrad_dma_kernel.
// ---------------------------------------------------------------------------
constexpr int kWWin = 128;
constexpr int kWWTile = kWgradRows * kWWin;   // floats per [32][128] LDS tile

template <bool SILU>
__global__ __launch_bounds__(kWgradThreads) void wgrad_wide_kernel(const nlam_wgrad_t p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // 2 x (A tile + B tile)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 31, hi = lane >> 5;

    // decode the output window
    const int mwins = (p.m + kWWin - 1) / kWWin;
    const int mw = blockIdx.y % mwins;
    int nwi = blockIdx.y / mwins;
    int s_sel = 0, off = 0;
    for (int s = 0; s < p.nsrc; ++s) {
        const int w = get_src(p, s).width;
        const int nws = (w + kWWin - 1) / kWWin;
        if (nwi < nws) {
            s_sel = s;
            break;
        }
        nwi -= nws;
        off += w;
    }
    const nlam_src_t S = get_src(p, s_sel);
    const int m0 = mw * kWWin, mcols = min(kWWin, p.m - m0);
    const int n0 = nwi * kWWin, ncols = min(kWWin, S.width - n0);
    const int gcol0 = off + n0;

    const int mb2 = (wave >> 1) * 2, nb2 = (wave & 1) * 2;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
    const bool act_m[2] = {mb2 * 32 < mcols, (mb2 + 1) * 32 < mcols};
    const bool act_n[2] = {nb2 * 32 < ncols, (nb2 + 1) * 32 < ncols};

    const int chunks_per_batch = (p.rows + kWgradRows - 1) / kWgradRows;
    const long total_chunks = (long)chunks_per_batch * p.batch;
    const int lrow = lane >> 5, lcol = (lane & 31) << 2;

    // gather indices one chunk ahead of the LDS-DMA that uses them (as in wgrad_dma_kernel)
    auto load_idx = [&](long ch, int(&ix)[4]) {
        const int r0 = (int)(ch % chunks_per_batch) * kWgradRows;
        const int nr = min(kWgradRows, p.rows - r0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = 2 * (wave * 4 + k) + lrow;
            const int prow = r0 + (r < nr ? r : 0);
            ix[k] = (r < nr && S.idx != nullptr) ? S.idx[prow] : prow;
        }
    };
    auto issue = [&](long ch, int buf, const int(&ix)[4]) {
        const int b = (int)(ch / chunks_per_batch);
        const int r0 = (int)(ch % chunks_per_batch) * kWgradRows;
        const int nr = min(kWgradRows, p.rows - r0);
        float* At = smem + (size_t)buf * 2 * kWWTile;
        float* Bt = At + kWWTile;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int pr = wave * 4 + k;          // row pair
            const int r = 2 * pr + lrow;
            const bool rv = r < nr;
            const long prow = r0 + (rv ? r : 0);
            {
                const float* src = (rv && lcol < mcols) ? p.A + ((size_t)b * p.rows + prow) * p.m + m0 + lcol : g_zero16;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(At + pr * 2 * kWWin), 16, 0, 0);
            }
            {
                const float* src = g_zero16;
                if (rv && lcol < ncols) src = S.ptr + (long)b * S.bstride + (long)ix[k] * S.width + n0 + lcol;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(Bt + pr * 2 * kWWin), 16, 0, 0);
            }
        }
    };

    long ch = blockIdx.x;
    int buf = 0;
    int ix[4];
    if (ch < total_chunks) {
        load_idx(ch, ix);
        issue(ch, 0, ix);
    }
    if (ch + gridDim.x < total_chunks) load_idx(ch + gridDim.x, ix);
    for (; ch < total_chunks; ch += gridDim.x) {
        __syncthreads();   // drains this wave's LDS-DMA; everyone is done reading buf ^ 1
        if (ch + gridDim.x < total_chunks) issue(ch + gridDim.x, buf ^ 1, ix);
        if (ch + 2 * (long)gridDim.x < total_chunks) load_idx(ch + 2 * (long)gridDim.x, ix);
        const float* At = smem + (size_t)buf * 2 * kWWTile;
        const float* Bt = At + kWWTile;
#pragma unroll 4
        for (int ks = 0; ks < kWgradRows / 2; ++ks) {
            const int ro = (2 * ks + hi) * kWWin;
            float a[2], bv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = At[ro + (mb2 + u) * 32 + i];
                bv[u] = Bt[ro + (nb2 + u) * 32 + i];
                if constexpr (SILU) bv[u] = silu_f(bv[u]);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v)
                    if (act_m[u] && act_n[v]) acc[u][v] = MFMA32(a[u], bv[v], acc[u][v]);
        }
        buf ^= 1;
    }
    float* P = p.partials + (size_t)blockIdx.x * p.m * p.n;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            if (act_m[u] && act_n[v]) {
                const int nl = (nb2 + v) * 32 + i;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ml = (mb2 + u) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (ml < mcols && nl < ncols) P[(size_t)(m0 + ml) * p.n + gcol0 + nl] = acc[u][v][r];
                }
            }
        }
}
