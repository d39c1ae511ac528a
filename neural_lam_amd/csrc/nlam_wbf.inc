// nlam_wbf.inc -- split-bf16 matrix path for hidden / output widths in (64, 512].
// Included inside the anonymous namespace of nlam_hip.hip after nlam_wide.inc.
//
// The fp32 workgroup-cooperative kernels of nlam_wide.inc give one 32-row tile to a
// workgroup, so every 32 rows stream the whole weight matrix out of L2 once.  That is
// fine at the fp32 MFMA rate; the bf16 matrix cores are 16x faster (2.7x with three
// split terms) and the packed split weights are 1.5x the bytes, so the same shape would
// need ~4x the L2 bandwidth the chip has.  This family therefore
//  * gives a workgroup of 8 waves NRT = RG * RT row tiles (a "super tile" of 64 to 256
//    rows).  The waves form an RG x FG grid: wave (rg, fg) owns the 32-feature blocks
//    fg, fg + FG, .. (FB of them) of the RT row tiles rg*RT .. rg*RT + RT - 1, so one
//    A (weight) fragment fetched from L2 feeds RT MFMAs per split product;
//  * keeps the weights in HBM/L2 already split into bf16 terms and in MFMA A-fragment
//    order (pack_bf_kernel, once per launch): one coalesced 1-KiB load per term, block
//    and K = 16 group, prefetched one group ahead;
//  * shares the B operands through LDS *in fragment order*: the gathered input rows are
//    split once by the staging threads (chunks of KG groups, double buffered), the hidden
//    tile is split by the wave that produced it; every B fetch is one linear,
//    conflict-free ds_read_b128 per term;
//  * runs GEMM2 + LayerNorm + outputs in passes of RTP row tiles per wave, because the
//    split hidden tile of a whole super tile (6 bytes per element at NS = 3) does not
//    fit the 160 KB of LDS at d >= 256; the input staging (dead after GEMM1) and the
//    hidden / message tiles (dead before the next super tile) share one LDS region.
// K order of GEMM2 is the slot permutation of the narrow split kernels (the hidden
// fragments are written straight from the accumulator layout).  Saved tensors (z1, xhat,
// rstd), the tile schedule and the output modes are those of the other forward kernels,
// so the backward kernels do not care which forward ran.

// launches with fewer super tiles than nlam_detail::wbf_min_supertiles (nlam_set_tuning, default 192) run on the fp32
// kernels of nlam_wide.inc

struct packbf_job_t {
    const float* W;
    long ldm, ldk;      // A[m][k] = W[m * ldm + k * ldk]
    int M, MB, Kw;      // real rows, 32-row blocks, real K columns
    int TK, g0, ng;     // K groups per block row of the destination, first group and group count of this job
    int perm2;          // slot-permuted K order (GEMM2)
    u32x4* dst;
};
struct packbf_jobs_t {
    packbf_job_t job[4];
    int njobs;
};

// dst[((mb * TK + g0 + g) * NS + term) * 64 + lane] = slots 0..7 of row mb*32 + (lane & 31) of group g
template <int NS>
__global__ void pack_bf_kernel(const packbf_jobs_t jobs) {
    if ((int)blockIdx.y >= jobs.njobs) return;
    const packbf_job_t jb = jobs.job[blockIdx.y];
    const long total = (long)jb.MB * jb.ng * 64;
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(s & 63);
        const long rest = s >> 6;
        const int g = (int)(rest % jb.ng);
        const int mb = (int)(rest / jb.ng);
        const int m = mb * 32 + (lane & 31);
        const int hi = lane >> 5;
        float x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = jb.perm2 ? 32 * (g >> 1) + 16 * (g & 1) + (q & 3) + 8 * (q >> 2) + 4 * hi : 16 * g + 8 * hi + q;
            x[q] = (m < jb.M && k < jb.Kw) ? jb.W[(long)m * jb.ldm + (long)k * jb.ldk] : 0.f;
        }
        const BfFrag<NS> f = split8<NS>(x);
#pragma unroll
        for (int pa = 0; pa < NS; ++pa) jb.dst[(((size_t)mb * jb.TK + jb.g0 + g) * NS + pa) * 64 + lane] = f.t[pa];
    }
}

template <int NS, int NW, int FG, int FB, int RT, int RTP>
struct WbfShape {
    static constexpr int NT = NW * 64;
    static constexpr int RG = NW / FG;
    static constexpr int NRT = RG * RT;                 // row tiles per workgroup (super tile)
    static constexpr int SL = (NS == 1 && NW == 8) ? 4 : 2;   // 8-float staging slots per thread and chunk (one term: a third
                                                        // of the LDS per K group, so chunks twice as long = half the barriers;
                                                        // the 4-wave shapes hold twice the accumulators per wave: two slots)
    static constexpr int KG = SL * NT / (NRT * 64);     // K = 16 groups per staged chunk
    static constexpr int SLOTS = NRT * KG * 64;         // 8-float staging slots per chunk
    static_assert(KG >= 2 && KG % 2 == 0, "chunks are walked two K groups at a time");
    static constexpr int NP = RT / RTP;                 // GEMM2 passes
    static constexpr int PT = RG * RTP;                 // row tiles per pass
    static_assert(RT % RTP == 0 && RT / RTP <= 4, "passes must tile the wave's row tiles");
    static_assert(FB * RT >= 2 && FB * RTP >= 2, "two accumulators must alternate (see mma_split_lds)");
};

// A fragments (all terms, the wave's FB blocks) of K group kg of a packed matrix with TK groups per block row
template <int NS, int FB>
struct AFrag {
    u32x4 a[NS][FB];
};

template <int NS, int FG, int FB>
__device__ __forceinline__ void load_afrag(AFrag<NS, FB>& r, const u32x4* A, int TK, int nblk, int kg, int fg, int lane) {
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
        int blk = fg + fb * FG;
        blk = blk < nblk ? blk : nblk - 1;   // waves beyond the matrix repeat its last block (results never leave)
        const u32x4* base = A + (((size_t)blk * TK + kg) * NS) * 64 + lane;
#pragma unroll
        for (int pa = 0; pa < NS; ++pa) r.a[pa][fb] = base[pa * 64];
    }
}

// Depth of the A-fragment register ring = K groups of weights in flight per wave.  The weights stream from L2 (~500-700 cycles
// under load); one group is FB x RT MFMAs of 32 cycles.  Three terms: a group is 6 FB RT MFMAs, two groups cover the latency.
// One term: 2 - 4 MFMAs per group, four groups in flight (K group counts of every phase are multiples of 4 then: the host
// sends odd block counts to the three-term kernels).
template <int NS, int FB>
struct WbfRing {
    static constexpr int D = (NS == 1 && FB <= 2) ? 4 : 2;   // four blocks per wave: 8 registers per group and block pair less to spare
};

// A fragments of K group g of the wave's FB blocks: base[fb] = the block's first fragment (uniform pointer; the lane is added
// here so that the address is scalar base + lane offset + immediate)
template <int NS, int FB>
__device__ __forceinline__ void load_aring(AFrag<NS, FB>& r, const u32x4* const (&base)[FB], int g, int lane) {
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
        const u32x4* q = base[fb] + (size_t)g * (NS * 64) + lane;
#pragma unroll
        for (int pa = 0; pa < NS; ++pa) r.a[pa][fb] = q[pa * 64];
    }
}

// acc[fb][r] += sum_{p+q<NS} A_p(fb) . B_q(r): accumulators innermost so consecutive MFMAs never chain
template <int NS, int FB, int NR>
__device__ __forceinline__ void mma_frags(f32x16 (&acc)[FB][NR], const AFrag<NS, FB>& A, const u32x4 (&B)[NS][NR]) {
#pragma unroll
    for (int ord = NS - 1; ord >= 0; --ord)
#pragma unroll
        for (int pa = 0; pa <= ord; ++pa)
#pragma unroll
            for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                for (int r = 0; r < NR; ++r) acc[fb][r] = MFMA_BF16(A.a[pa][fb], B[ord - pa][r], acc[fb][r]);
}


// ---------------------------------------------------------------------------
// bf16 storage of the tensors a layer saves for / hands to its own backward (NLAM_F_STORE_BF16; torch.autocast(bfloat16) only)
// ---------------------------------------------------------------------------
// Under Lightning's --precision bf16-mixed (train_model.py:163-168) the reference's nn.Linear outputs ARE bf16 tensors: the
// pre-activation z1 it saves, and the row gradients dz1 / dz2 its backward produces, have 8 significant bits.  The one-term
// kernels then keep z1, xhat, dz1 and dz2 in HBM as bf16: 2 KB less written and 2 KB less read per row and direction at d = 512
// (a quarter to a third of the algorithmic bytes of the forward, backward and weight-gradient launches).
// A 32 x 32 block in accumulator layout has 4 columns per lane and chunk (lane (j, hi): row j, columns 8 tt + 4 hi ..): pairs of
// chunks are exchanged between the half waves (v_permlane32_swap) so that every lane holds 8 CONSECUTIVE columns = one 16-byte
// access: lane (j, hi) covers columns c0 + 8 (2 pr + hi) .. + 7 of row j for pr = 0, 1.
typedef unsigned short bf16s_t;

__device__ __forceinline__ void store_block_bf16(bf16s_t* row, int c0, int hi, bool valid, const f32x16& v) {
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        float x[8];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // a = chunk 2 pr (low half: this row's columns +0..3, high half: +4..7), b = chunk 2 pr + 1; after the swap the low
            // half holds (a.low | b.low) ... see tools/probes/permlane_probe.hip
            // (element copies first: __builtin_bit_cast applied to a vector-element lvalue reads element 0 with this clang)
            const float fa = v[8 * pr + c], fb = v[8 * pr + 4 + c];
            const unsigned a = __builtin_bit_cast(unsigned, fa), b = __builtin_bit_cast(unsigned, fb);
            const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
            x[c] = __builtin_bit_cast(float, (unsigned)r[0]);
            x[4 + c] = __builtin_bit_cast(float, (unsigned)r[1]);
        }
        const BfFrag<1> f = split8<1>(x);
        if (valid) *reinterpret_cast<u32x4*>(row + c0 + 8 * (2 * pr + hi)) = f.t[0];
    }
}

// requests only (two 16-byte loads per block; an invalid row reads the zero buffer, so the loads stay unconditional) ...
__device__ __forceinline__ void load_block_bf16_raw(const bf16s_t* row, int c0, int hi, bool valid, u32x4 (&raw)[2]) {
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const bf16s_t* q = valid ? row + c0 + 8 * (2 * pr + hi) : reinterpret_cast<const bf16s_t*>(g_zero16);
        raw[pr] = *reinterpret_cast<const u32x4*>(q);
    }
}

// ... and the arithmetic: widen, swap the chunk pairs back into accumulator layout
__device__ __forceinline__ f32x16 block_from_bf16_raw(const u32x4 (&raw)[2]) {
    f32x16 v;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // columns 0..3 of the lane's eight are dwords 0, 1 (low / high half word), 4..7 dwords 2, 3
            const unsigned w0 = raw[pr][c >> 1], w1 = raw[pr][2 + (c >> 1)];
            const unsigned lo = (c & 1) ? (w0 & 0xffff0000u) : (w0 << 16);
            const unsigned up = (c & 1) ? (w1 & 0xffff0000u) : (w1 << 16);
            const auto r = __builtin_amdgcn_permlane32_swap(lo, up, false, false);
            v[8 * pr + c] = __builtin_bit_cast(float, (unsigned)r[0]);
            v[8 * pr + 4 + c] = __builtin_bit_cast(float, (unsigned)r[1]);
        }
    }
    return v;
}

template <int NS, int NW, int FG, int FB, int RT, int RTP, bool SBF = false, bool V4 = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void mlp_fwd_wbf_kernel(const nlam_mlp_fwd_t p) {
    static_assert(!SBF || NS == 1, "bf16 storage belongs to the one-term (autocast) kernels");
    using SH = WbfShape<NS, NW, FG, FB, RT, RTP>;
    constexpr int NT = SH::NT, RG = SH::RG, NRT = SH::NRT, KG = SH::KG, SL = SH::SL, NP = SH::NP, PT = SH::PT;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rg = wave / FG, fg = wave % FG;
    const int j = lane & 31, hi = lane >> 5;

    const int HBT = (p.hid + 31) >> 5, OBT = (p.dout + 31) >> 5;
    // NLAM_F_PRE_ADD (factorised edge MLP): only source 0 is staged and multiplied; sources 1.. are gathered rows of
    // width hid that initialise GEMM1's accumulators ((W1_j x)[sender] + (W1_i x)[receiver])
    const bool pre = (p.flags & NLAM_F_PRE_ADD) != 0;
    const int ngemm = pre ? 1 : p.nsrc;
    int TK1 = 0;
    for (int s = 0; s < ngemm; ++s) TK1 += ((get_src(p, s).width + 16 * KG - 1) / (16 * KG)) * KG;
    const int TK2 = 2 * HBT;
    const u32x4* A1 = reinterpret_cast<const u32x4*>(p.wpack);
    const u32x4* A2 = A1 + (size_t)HBT * TK1 * NS * 64;

    // LDS map
    u32x4* Xf = reinterpret_cast<u32x4*>(smem);                         // 2 x [NRT][KG][NS][64]
    constexpr size_t kXfVec = (size_t)NRT * KG * NS * 64;               // u32x4 per buffer
    // the staged input is dead once GEMM1 is done and the hidden / message tiles are dead before the next super tile
    // stages its first chunk: the two regions share their LDS
    u32x4* Hf = Xf;                                                     // [PT][TK2][NS][64]
    const size_t hf_vec = (size_t)PT * TK2 * NS * 64;
    size_t r0_vec = 2 * kXfVec;
    if (hf_vec > r0_vec) r0_vec = hf_vec;
    constexpr size_t kStgVec = (size_t)NW * 32 * kStgStride / 4;
    if (kStgVec > r0_vec) r0_vec = kStgVec;
    // round 6: no message tile.  The aggregation used to stage the pass's fp32 messages for all columns (32 x (dout + 4) floats
    // per row tile: 66 KB at d = 512, the largest LDS region of the kernel) and reduce them with a thread -> (receiver, column)
    // loop between two workgroup barriers; a wave now reduces each of ITS 32-column blocks over the tile's receivers through
    // a [32][36] block of its own (block_segment_reduce, as the narrow kernels and the backward do).  The blocks live at the
    // start of the hidden-fragment region, which is dead once every wave has left GEMM2 (the barrier in front of the epilogue)
    float* stg = reinterpret_cast<float*>(Hf) + (size_t)wave * 32 * kStgStride;            // NW x [32][36]
    float* red = reinterpret_cast<float*>(Xf + r0_vec);                                    // 2 x FG x PT*32
    int* ridx = reinterpret_cast<int*>(red + 2 * FG * PT * 32);         // NLAM_MAX_SRC x NRT*32 gathered row ids (-1 = no row)
    // b1 | b2 | gamma | beta, zero / one padded to whole blocks: the epilogues read them as broadcast b128 LDS loads
    // (as global loads they were four guarded dword loads per chunk, each a full L2 round trip in the critical path)
    const int DP = (HBT > OBT ? HBT : OBT) * 32;
    float* pvec = reinterpret_cast<float*>(ridx + NLAM_MAX_SRC * NRT * 32);   // 4 x DP
    int* rps = reinterpret_cast<int*>(pvec + 4 * DP);                         // NRT x 33 row pointers of the tiles' receivers
    float* scs = reinterpret_cast<float*>(rps + NRT * 33);                    // NRT x 32 their mean scales
    int* tds = reinterpret_cast<int*>(scs + NRT * 32);                        // NRT x (row0, nrows, seg0, nseg | split flag)
    auto lds_tile = [&](int k) {
        TileInfo t;
        t.row0 = tds[4 * k + 0];
        t.nrows = tds[4 * k + 1];
        t.seg0 = tds[4 * k + 2];
        t.split = (tds[4 * k + 3] & NLAM_TILE_SPLIT) != 0;
        t.nseg = tds[4 * k + 3] & ~NLAM_TILE_SPLIT;
        return t;
    };
    for (int c = tid; c < DP; c += NT) {
        pvec[c] = (p.b1 != nullptr && c < p.hid) ? p.b1[c] : 0.f;
        pvec[DP + c] = (p.b2 != nullptr && c < p.dout) ? p.b2[c] : 0.f;
        pvec[2 * DP + c] = (p.ln_w != nullptr && c < p.dout) ? p.ln_w[c] : 1.f;
        pvec[3 * DP + c] = (p.ln_b != nullptr && c < p.dout) ? p.ln_b[c] : 0.f;
    }

    const bool has_ln = p.ln_w != nullptr;
    constexpr bool sbf = SBF;   // NLAM_F_STORE_BF16: z1 / xhat leave as bf16 rows (compile time: a run-time branch around stores / loads
                                // makes the wait-counter pass drain the memory queue at its join)
    const float inv_dout = 1.f / (float)p.dout;
    const int spb = (p.ntiles + NRT - 1) / NRT;          // super tiles per batch element
    const long nsuper = (long)spb * p.batch;

    // A stream of a super tile: GEMM1 groups 0 .. TK1-1, then the TK2 groups of GEMM2 once per pass; it wraps into the next
    // super tile.  D groups are in flight in a register ring indexed at compile time (group g lives in ring[g % D]: every
    // phase has a multiple of D groups).  Addresses are a uniform base pointer per block (two per wave and matrix) + group
    // stride: the generic (phase, group) -> address function this replaces cost ~19 scalar instructions and three branches per
    // MFMA in the one-term kernels, and its dependent scalar chain delayed every fetch (round 4).
    constexpr int D = WbfRing<NS, FB>::D;
    static_assert(KG % D == 0, "a staged chunk is a whole number of ring revolutions");
    const u32x4* a1b[FB];
    const u32x4* a2b[FB];
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
        const int b1 = min(fg + fb * FG, HBT - 1), b2 = min(fg + fb * FG, OBT - 1);   // waves beyond the matrix repeat its last block
        a1b[fb] = A1 + (size_t)b1 * TK1 * NS * 64;
        a2b[fb] = A2 + (size_t)b2 * TK2 * NS * 64;
    }
    AFrag<NS, FB> ring[D];
#pragma unroll
    for (int u = 0; u < D; ++u) load_aring<NS, FB>(ring[u], a1b, u, lane);
    NLAM_T_DECL
    int t_ntiles_ = 0;

    for (long st = xcd_slot((int)blockIdx.x, (int)gridDim.x); st < nsuper; st += gridDim.x) {
        const int b = (int)(st / spb);
        const int t0 = (int)(st % spb) * NRT;

        // ---- gathered row ids of the super tile ----
        for (int idx = tid; idx < NLAM_MAX_SRC * NRT * 32; idx += NT) {
            const int s = idx / (NRT * 32), r = idx - s * (NRT * 32);
            const int ti = t0 + (r >> 5);
            int v = -1;
            if (s == 0 && (r & 31) == 0 && ti >= p.ntiles) {
                tds[4 * (r >> 5) + 0] = 0;
                tds[4 * (r >> 5) + 1] = 0;
                tds[4 * (r >> 5) + 2] = 0;
                tds[4 * (r >> 5) + 3] = 0;
            }
            if (s < p.nsrc && ti < p.ntiles) {
                const TileInfo tk = get_tile(p.tiles, ti, p.rows);
                if (s == 0 && (r & 31) == 0) {   // descriptor cache: later stages read it from LDS
                    tds[4 * (r >> 5) + 0] = tk.row0;
                    tds[4 * (r >> 5) + 1] = tk.nrows;
                    tds[4 * (r >> 5) + 2] = tk.seg0;
                    tds[4 * (r >> 5) + 3] = tk.nseg | (tk.split ? NLAM_TILE_SPLIT : 0);
                }
                if ((r & 31) < tk.nrows) {
                    const nlam_src_t S = get_src(p, s);
                    const int row = tk.row0 + (r & 31);
                    v = S.idx != nullptr ? S.idx[row] : row;
                }
            }
            ridx[idx] = v;
        }
        if (p.aggr != nullptr) {   // the tiles' CSR row pointers and scales, fetched with the row ids instead of inside the reduction
            for (int idx = tid; idx < NRT * 33; idx += NT) {
                const int k = idx / 33, l = idx - k * 33;
                const int ti = t0 + k;
                int rpv = 0;
                float sc = 1.f;
                if (ti < p.ntiles) {
                    const TileInfo tk = get_tile(p.tiles, ti, p.rows);
                    if (!tk.split && l <= tk.nseg) rpv = p.rowptr[tk.seg0 + l];
                    if (l < tk.nseg && (p.flags & NLAM_F_MEAN)) sc = p.inv_deg[tk.seg0 + l];
                }
                rps[idx] = rpv;
                if (l < 32) scs[k * 32 + l] = sc;
            }
        }
        __syncthreads();
        ++t_ntiles_;
        NLAM_T_MARK(0)

        // ---- staging: slot -> (row tile, K group, fragment lane) ----
        auto stage_load = [&](int s, int c0, f32x4(&v)[SL][2]) {
            const nlam_src_t S = get_src(p, s);
#pragma unroll
            for (int k = 0; k < SL; ++k) {
                const int slot = tid + k * NT;
                f32x4 lo = {0.f, 0.f, 0.f, 0.f}, up = {0.f, 0.f, 0.f, 0.f};
                if (slot < SH::SLOTS) {
                    const int ln = slot & 63, g = (slot >> 6) % KG, rt = slot / (64 * KG);
                    const int rid = ridx[s * (NRT * 32) + rt * 32 + (ln & 31)];
                    const int c = c0 + 16 * g + 8 * (ln >> 5);
                    if (rid >= 0 && c < S.width) {
                        const float* row = S.ptr + (long)b * S.bstride + (long)rid * S.width + c;
                        lo = *reinterpret_cast<const f32x4*>(row);
                        if (c + 4 < S.width) up = *reinterpret_cast<const f32x4*>(row + 4);
                    }
                }
                v[k][0] = lo;
                v[k][1] = up;
            }
        };
        auto stage_store = [&](u32x4* Xb, const f32x4(&v)[SL][2]) {
#pragma unroll
            for (int k = 0; k < SL; ++k) {
                const int slot = tid + k * NT;
                if (slot < SH::SLOTS) {
                    const int ln = slot & 63, gr = slot >> 6;   // gr = rt * KG + g
                    float x[8];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        x[c] = v[k][0][c];
                        x[4 + c] = v[k][1][c];
                    }
                    const BfFrag<NS> f = split8<NS>(x);
#pragma unroll
                    for (int pa = 0; pa < NS; ++pa) Xb[((size_t)gr * NS + pa) * 64 + ln] = f.t[pa];
                }
            }
        };

        // ---- GEMM1 over the staged chunks ----
        f32x16 acc1[FB][RT];
#pragma unroll
        for (int fb = 0; fb < FB; ++fb)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc1[fb][rt][r] = 0.f;
        if (pre) {
            // the addend rows ARE the initial accumulators (chunk layout = accumulator layout); their gathers are in
            // flight while the first chunk of source 0 is staged.  Requests first, sums afterwards (load_chunk is a branch: with
            // `acc += load` per chunk every chunk was waited for before the next request -- 32 serial round trips)
            // (FB * RT > 4 -- the 64-row 4-wave shape at d = 512: 128 accumulator registers -- has no room for a second full set:
            // the second addend is requested one row tile at a time behind the whole first one)
            constexpr int RT2 = (FB * RT > 4) ? 1 : RT;
            f32x16 add2[FB][RT2];
            auto request = [&](int k, int rt, f32x16(&dst)[FB]) {
                const bool have = k < p.nsrc;
                const nlam_src_t S = get_src(p, have ? k : 0);
                const int rid = have ? ridx[k * (NRT * 32) + (rg * RT + rt) * 32 + j] : -1;
                const float* row = rid >= 0 ? S.ptr + (long)b * S.bstride + (long)rid * S.width : nullptr;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const f32x4 a = load_chunk_v<V4>(row, p.hid, blk * 4 + tt, hi, rid >= 0 && blk < HBT);
#pragma unroll
                        for (int c = 0; c < 4; ++c) dst[fb][4 * tt + c] = a[c];
                    }
                }
            };
            f32x16 tmp1[FB];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                request(1, rt, tmp1);
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) acc1[fb][rt] = tmp1[fb];
            }
            static_assert(NLAM_MAX_SRC == 3, "two addend sources");
            if constexpr (RT2 == RT) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    request(2, rt, tmp1);
#pragma unroll
                    for (int fb = 0; fb < FB; ++fb) add2[fb][rt] = tmp1[fb];
                }
#pragma unroll
                for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc1[fb][rt][r] += add2[fb][rt][r];
            } else {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    request(2, rt, tmp1);
#pragma unroll
                    for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc1[fb][rt][r] += tmp1[fb][r];
                }
            }
        }
        {
            // The gathered rows of chunk c + 2 are requested in the middle of chunk c and split / stored at the end of
            // chunk c + 1.  Loads retire in order, so a request is forced home by the first wait on anything issued after
            // it; placed behind both A fetches of chunk c, that is the second A wait of chunk c + 1: a whole chunk of
            // MFMAs later instead of half a chunk (the HBM gather latency was the largest stall of this loop).
            f32x4 sv_new[SL][2], sv_old[SL][2];
            auto next_chunk = [&](int& s_, int& c0_) {
                c0_ += 16 * KG;
                if (c0_ >= get_src(p, s_).width) {
                    ++s_;
                    c0_ = 0;
                }
            };
            int cs = 0, buf = 0, kg = 0;
            int n1s = 0, n1c = 0;
            next_chunk(n1s, n1c);
            int n2s = n1s, n2c = n1c;
            if (n1s < ngemm) next_chunk(n2s, n2c);
            stage_load(0, 0, sv_old);
            if (n1s < ngemm) stage_load(n1s, n1c, sv_new);
            stage_store(Xf, sv_old);
            __syncthreads();
            NLAM_T_MARK(1)
            auto read_b = [&](u32x4(&b)[NS][RT], const u32x4* Xb, int g) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int pa = 0; pa < NS; ++pa) b[pa][rt] = Xb[(((size_t)(rg * RT + rt) * KG + g) * NS + pa) * 64 + lane];
            };
            while (cs < ngemm) {
                const bool has1 = n1s < ngemm;
                const bool has2 = has1 && n2s < ngemm;
                const u32x4* Xb = Xf + (size_t)buf * kXfVec;
#pragma unroll
                for (int g = 0; g < KG; g += D) {
#pragma unroll
                    for (int u = 0; u < D; ++u) {
                        u32x4 bq[NS][RT];
                        read_b(bq, Xb, g + u);
                        mma_frags<NS, FB, RT>(acc1, ring[u], bq);
                        // refill the slot with the group D ahead: GEMM1's own, or the head of GEMM2 behind its last groups
                        const int nxt = kg + g + u + D;
                        const bool wrap = nxt >= TK1;
                        const u32x4* nb[FB];
#pragma unroll
                        for (int fb = 0; fb < FB; ++fb) nb[fb] = wrap ? a2b[fb] : a1b[fb];
                        load_aring<NS, FB>(ring[u], nb, wrap ? nxt - TK1 : nxt, lane);
                        if (g == 0 && u == 0) {
                            if (has1) {
#pragma unroll
                                for (int k = 0; k < SL; ++k) {
                                    sv_old[k][0] = sv_new[k][0];
                                    sv_old[k][1] = sv_new[k][1];
                                }
                            }
                            if (has2) stage_load(n2s, n2c, sv_new);
                        }
                    }
                }
                kg += KG;
                if (has1) stage_store(Xf + (size_t)(buf ^ 1) * kXfVec, sv_old);
                __syncthreads();
                buf ^= 1;
                cs = n1s;
                n1s = n2s;
                n1c = n2c;
                if (has2) next_chunk(n2s, n2c);
            }
        }
        NLAM_T_MARK(2)

        // ---- passes: hidden tile -> GEMM2 -> LayerNorm -> outputs for RTP row tiles per wave ----
        auto run_pass = [&](auto ps_c) {
            constexpr int ps = decltype(ps_c)::value;   // compile-time: acc1 is indexed with it
            // rows of this wave in the pass
            TileInfo tl[RTP];
            bool valid[RTP];
            int prow[RTP];
#pragma unroll
            for (int rp = 0; rp < RTP; ++rp) {
                tl[rp] = lds_tile(rg * RT + ps * RTP + rp);
                valid[rp] = j < tl[rp].nrows;
                prow[rp] = tl[rp].row0 + j;
            }

            // bias, save pre-activation, SiLU, split -> hidden fragments
#pragma unroll
            for (int rp = 0; rp < RTP; ++rp) {
                const size_t zrow_id = (size_t)b * p.rows + prow[rp];
                float* z1row = p.z1 != nullptr ? p.z1 + zrow_id * p.hid : nullptr;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
                    if (blk < HBT) {
                        f32x16 z16;
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) {
                            const f32x4 z = acc_chunk(acc1[fb][ps * RTP + rp], tt) + *reinterpret_cast<const f32x4*>(&pvec[8 * (blk * 4 + tt) + 4 * hi]);
#pragma unroll
                            for (int c = 0; c < 4; ++c) z16[4 * tt + c] = z[c];
                        }
                        if (p.z1 != nullptr) {
                            if constexpr (sbf) {
                                store_block_bf16(reinterpret_cast<bf16s_t*>(p.z1) + zrow_id * p.hid, 32 * blk, hi, valid[rp], z16);
                            } else {
#pragma unroll
                                for (int tt = 0; tt < 4; ++tt) store_chunk_v<V4>(z1row, p.hid, blk * 4 + tt, hi, valid[rp], acc_chunk(z16, tt));
                            }
                        }
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            float x[8];
#pragma unroll
                            for (int q = 0; q < 8; ++q) x[q] = silu_f(z16[8 * h + q]);
                            const BfFrag<NS> f = split8<NS>(x);
                            const size_t gr = (size_t)(rg * RTP + rp) * TK2 + 2 * blk + h;
#pragma unroll
                            for (int pa = 0; pa < NS; ++pa) Hf[(gr * NS + pa) * 64 + lane] = f.t[pa];
                        }
                    }
                }
            }
            __syncthreads();
            NLAM_T_MARK(3)

            // GEMM2 from the hidden fragments
            f32x16 acc2[FB][RTP];
#pragma unroll
            for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                for (int rp = 0; rp < RTP; ++rp)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc2[fb][rp][r] = 0.f;
            {
                auto read_h = [&](u32x4(&b)[NS][RTP], int g) {
#pragma unroll
                    for (int rp = 0; rp < RTP; ++rp)
#pragma unroll
                        for (int pa = 0; pa < NS; ++pa) b[pa][rp] = Hf[(((size_t)(rg * RTP + rp) * TK2 + g) * NS + pa) * 64 + lane];
                };
                // behind this pass's groups: the next pass walks W2 again; after the last pass the next super tile's GEMM1
                constexpr bool last_pass = ps + 1 == NP;
                for (int kg = 0; kg < TK2; kg += D) {
#pragma unroll
                    for (int u = 0; u < D; ++u) {
                        u32x4 hq[NS][RTP];
                        read_h(hq, kg + u);
                        mma_frags<NS, FB, RTP>(acc2, ring[u], hq);
                        const int nxt = kg + u + D;
                        const bool wrap = nxt >= TK2;
                        const u32x4* nb[FB];
#pragma unroll
                        for (int fb = 0; fb < FB; ++fb) nb[fb] = (wrap && last_pass) ? a1b[fb] : a2b[fb];
                        load_aring<NS, FB>(ring[u], nb, wrap ? nxt - TK2 : nxt, lane);
                    }
                }
            }
            NLAM_T_MARK(4)
            // bias 2 + LayerNorm over the real dout features (row statistics across the FG waves of the row group)
            float sum[RTP];
#pragma unroll
            for (int rp = 0; rp < RTP; ++rp) {
                sum[rp] = 0.f;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
                    if (blk < OBT) {
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) {
                            const int c0 = 8 * (blk * 4 + tt) + 4 * hi;
                            const f32x4 bias = *reinterpret_cast<const f32x4*>(&pvec[DP + c0]);
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                const float v = acc2[fb][rp][4 * tt + c] + bias[c];
                                acc2[fb][rp][4 * tt + c] = v;
                                sum[rp] += (c0 + c < p.dout) ? v : 0.f;
                            }
                        }
                    }
                }
            }
            if (has_ln) {
#pragma unroll
                for (int rp = 0; rp < RTP; ++rp) {
                    const float s = row_allreduce(sum[rp]);
                    if (hi == 0) red[(fg * PT + rg * RTP + rp) * 32 + j] = s;
                }
                NLAM_T_MARK(8)
                __syncthreads();   // also: every wave is done reading the hidden fragments
                NLAM_T_MARK(9)
                float rstd[RTP];
#pragma unroll
                for (int rp = 0; rp < RTP; ++rp) {
                    float tot = 0.f;
#pragma unroll
                    for (int w = 0; w < FG; ++w) tot += red[(w * PT + rg * RTP + rp) * 32 + j];
                    const float mean = tot * inv_dout;
                    float sq = 0.f;
#pragma unroll
                    for (int fb = 0; fb < FB; ++fb) {
                        const int blk = fg + fb * FG;
                        if (blk < OBT) {
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) {
                                const int c0 = 8 * (blk * 4 + tt) + 4 * hi;
#pragma unroll
                                for (int c = 0; c < 4; ++c) {
                                    const float dlt = acc2[fb][rp][4 * tt + c] - mean;
                                    acc2[fb][rp][4 * tt + c] = dlt;
                                    sq += (c0 + c < p.dout) ? dlt * dlt : 0.f;
                                }
                            }
                        }
                    }
                    sq = row_allreduce(sq);
                    if (hi == 0) red[((FG + fg) * PT + rg * RTP + rp) * 32 + j] = sq;
                }
                NLAM_T_MARK(10)
                __syncthreads();
                NLAM_T_MARK(11)
#pragma unroll
                for (int rp = 0; rp < RTP; ++rp) {
                    float tot2 = 0.f;
#pragma unroll
                    for (int w = 0; w < FG; ++w) tot2 += red[((FG + w) * PT + rg * RTP + rp) * 32 + j];
                    rstd[rp] = rsqrtf(tot2 * inv_dout + p.eps);
                    if (p.rstd != nullptr && valid[rp] && hi == 0 && fg == 0) p.rstd[(size_t)b * p.rows + prow[rp]] = rstd[rp];
                    const size_t xrow_id = (size_t)b * p.rows + prow[rp];
                    float* xrow = p.xhat != nullptr ? p.xhat + xrow_id * p.dout : nullptr;
#pragma unroll
                    for (int fb = 0; fb < FB; ++fb) {
                        const int blk = fg + fb * FG;
                        if (blk < OBT) {
                            f32x16 xh16;
#pragma unroll
                            for (int r = 0; r < 16; ++r) xh16[r] = acc2[fb][rp][r] * rstd[rp];
                            if (p.xhat != nullptr) {
                                if constexpr (sbf) {
                                    store_block_bf16(reinterpret_cast<bf16s_t*>(p.xhat) + xrow_id * p.dout, 32 * blk, hi, valid[rp], xh16);
                                } else {
#pragma unroll
                                    for (int tt = 0; tt < 4; ++tt) store_chunk_v<V4>(xrow, p.dout, blk * 4 + tt, hi, valid[rp], acc_chunk(xh16, tt));
                                }
                            }
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) {
                                const int c0 = 8 * (blk * 4 + tt) + 4 * hi;
                                const f32x4 g = *reinterpret_cast<const f32x4*>(&pvec[2 * DP + c0]);
                                const f32x4 be = *reinterpret_cast<const f32x4*>(&pvec[3 * DP + c0]);
#pragma unroll
                                for (int c = 0; c < 4; ++c) acc2[fb][rp][4 * tt + c] = xh16[4 * tt + c] * g[c] + be[c];
                            }
                        }
                    }
                }
            } else {
                __syncthreads();   // every wave is done reading the hidden fragments (the region becomes the staging blocks)
            }

            NLAM_T_MARK(5)
            // msg = mlp [+ src1]; aggregate; out = msg [+ src0] -- block by block: the residual chunks of block fb + 1 are requested
            // before the stores of block fb (a load issued behind a store waits for that store's acknowledgement, DESIGN section 3
            // finding 4), 32 registers of residual in flight instead of FB x 16
#pragma unroll
            for (int rp = 0; rp < RTP; ++rp) {
                const int kt = rg * RT + ps * RTP + rp;              // tile slot in the super tile
                const int rl = kt * 32 + j;                          // row slot in ridx
                const float* srow0 = nullptr;
                const float* srow1 = nullptr;
                if (valid[rp]) {
                    srow0 = p.src[0].ptr + (long)b * p.src[0].bstride + (long)ridx[rl] * p.src[0].width;
                    if (p.nsrc > 1) srow1 = p.src[1].ptr + (long)b * p.src[1].bstride + (long)ridx[NRT * 32 + rl] * p.src[1].width;
                }
                float* orow = nullptr;
                if (p.out != nullptr && valid[rp]) {
                    const long oidx = p.out_idx != nullptr ? p.out_idx[prow[rp]] : prow[rp];
                    orow = p.out + (long)b * p.out_bstride + oidx * (long)p.dout;
                }
                const bool add0 = (p.flags & NLAM_F_ADD_SRC0) != 0 && orow != nullptr;
                const bool add1 = (p.flags & NLAM_F_ADD_SRC1) != 0;
                int raw_ptr = 0;
                float my_scale = 1.f;
                if (p.aggr != nullptr) {
                    if (lane <= 32) raw_ptr = rps[kt * 33 + lane];
                    if (lane < 32) my_scale = scs[kt * 32 + lane];
                }
                float* out_b = p.aggr != nullptr ? p.aggr + (size_t)b * p.nseg_total * p.dout : nullptr;
                f32x4 res[2][4];
                auto request = [&](int fb, f32x4(&dst)[4]) {
                    const int blk = fg + fb * FG;
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) dst[tt] = load_chunk_v<V4>(srow0, p.dout, blk * 4 + tt, hi, add0 && valid[rp] && blk < OBT);
                };
                request(0, res[0]);
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
                    if (fb + 1 < FB) request(fb + 1, res[(fb + 1) & 1]);
                    if (blk < OBT) {
                        if (add1) {   // msg = mlp + x_j (PropagationNet)
                            f32x4 r1[4];
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) r1[tt] = load_chunk_v<V4>(srow1, p.dout, blk * 4 + tt, hi, valid[rp]);
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                                for (int c = 0; c < 4; ++c) acc2[fb][rp][4 * tt + c] += r1[tt][c];
                        }
                        if (p.aggr != nullptr) {
                            const TileInfo tk = lds_tile(kt);
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) {
                                f32x4 m = acc_chunk(acc2[fb][rp], tt);
                                if (!valid[rp]) m = f32x4{0.f, 0.f, 0.f, 0.f};
                                *reinterpret_cast<f32x4*>(&stg[j * kStgStride + 8 * tt + 4 * hi]) = m;
                            }
                            wave_lds_sync();
                            if (tk.nseg > 0)   // (also a tile of isolated receivers: their aggregate rows are written as zeros)
                                block_segment_reduce(stg, tk, raw_ptr, my_scale, out_b + 32 * blk, p.dout, min(32, p.dout - 32 * blk), lane);
                            wave_lds_sync();
                        }
                        if (orow != nullptr) {
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt)
                                store_chunk_v<V4>(orow, p.dout, blk * 4 + tt, hi, valid[rp], acc_chunk(acc2[fb][rp], tt) + res[fb & 1][tt]);
                        }
                    }
                }
            }
            __syncthreads();   // pass end: the hidden region, red and (after the last pass) Xf / ridx are reused
            NLAM_T_MARK(6)
        };
        run_pass(std::integral_constant<int, 0>{});
        if constexpr (NP > 1) run_pass(std::integral_constant<int, 1>{});
        if constexpr (NP > 2) run_pass(std::integral_constant<int, 2>{});
        if constexpr (NP > 3) run_pass(std::integral_constant<int, 3>{});
    }
    NLAM_T_DRAIN
    NLAM_T_MARK(7)
    NLAM_T_FLUSH(t_ntiles_)
}

// ---------------------------------------------------------------------------
// Round 6: the factorised edge layer's forward as a kernel of its own (mlp_fwd_edge_kernel)
// ---------------------------------------------------------------------------
// mlp_fwd_wbf_kernel is one template for every launch geometry of the family; at d = 512 it holds ~80 loop-invariant registers
// besides its accumulators (SGPR 106, 84-120 bytes of scratch per lane) and every attempt to overlap one super tile's exposed
// latencies with the previous tile's work -- 107k of 167k wave-cycles per 64 rows are descriptor / index / row gathers at the tile
// start and residual / store round trips at its end (profiles/round6/phase_cycles_d512_plans.txt) -- ended in 100-170 spilled
// registers and a SLOWER kernel (profiles/round6/ab_fwd_prefetch_rejected.log).  This kernel is that template's 8-wave / 64-row
// shape for exactly one launch -- the factorised InteractionNet edge MLP of one width D (gnn_layers.py:110-189: Linear(3D -> D)
// as W1_e e + (W1_j x)[sender] + (W1_i x)[receiver], SiLU, Linear(D -> D), LayerNorm, sum / mean aggregation, optional edge
// update), one term (autocast, d = 512) or three (fp32 class, d = 256) -- with every shape a template constant, and software-pipelined
// across super tiles:
//  * tile metadata (row ids of the three sources, CSR row pointers, descriptors) double buffered in LDS, fetched for tile t + 1
//    while tile t runs GEMM2;
//  * the first K chunk of tile t + 1's gathered edge rows requested at the top of tile t's epilogue, split and parked in an LDS
//    buffer of its own (Xp) at the epilogue's end: GEMM1 of a tile starts on data that is already there;
//  * GEMM2 for both row tiles at once (an A fragment fetched from L2 feeds two MFMAs in both GEMMs);
//  * per (row tile, 32-column block) epilogue with rolling residual requests and per-wave segment sums (as the round-6 epilogue of
//    mlp_fwd_wbf_kernel).
// Weight image: the one mlp_fwd_wbf_kernel's launch of the same problem uses (same packer, same K-group order).
template <int NS, int D_, bool SBF>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void mlp_fwd_edge_kernel(const nlam_mlp_fwd_t p) {
    static_assert(NS == 1 || (NS == 3 && !SBF), "one term (autocast) or three (fp32 class)");
    constexpr int NW = 8, NT = 512, FG = 8, RT = 2, NRT = 2;
    constexpr int HBT = D_ / 32, FB = HBT / FG, TK = D_ / 16;            // blocks of hid = dout, blocks per wave, K groups of either GEMM
    static_assert(D_ % 256 == 0 && FB >= 1 && FB <= 2, "d = 256 or 512");
    static_assert(FB * RT >= 2, "two accumulators must alternate (see mma_split_lds)");
    constexpr int SL = NS == 1 ? 4 : 2, KG = SL * NT / (NRT * 64), NCH = TK / KG;   // K groups per staged chunk (16 / 8), chunks of GEMM1
    static_assert(TK % KG == 0 && NCH >= 1, "whole chunks");
    constexpr int RD = NS == 1 ? 4 : 2;                                 // A-fragment ring depth (K groups in flight)
    (void)NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int fg = __builtin_amdgcn_readfirstlane(tid >> 6);             // wave = feature group; both row tiles
    const int j = lane & 31, hi = lane >> 5;

    // LDS map
    constexpr size_t kXfVec = (size_t)NRT * KG * NS * 64;               // u32x4 per staged chunk
    constexpr size_t kHfVec = (size_t)NRT * TK * NS * 64;               // hidden fragments of both row tiles
    constexpr size_t kR0 = kHfVec > 2 * kXfVec ? kHfVec : 2 * kXfVec;
    u32x4* Xf = reinterpret_cast<u32x4*>(smem);                         // 2 chunk buffers | later the hidden fragments | later the staging blocks
    u32x4* Hf = Xf;
    float* stg = reinterpret_cast<float*>(Hf) + (size_t)fg * 32 * kStgStride;
    u32x4* Xp = Xf + kR0;                                               // chunk 0 of the NEXT super tile
    float* red = reinterpret_cast<float*>(Xp + kXfVec);                 // 2 x FG x NRT*32
    float* pvec = red + 2 * FG * NRT * 32;                              // b1 | b2 | gamma | beta
    constexpr int kRidx = NLAM_MAX_SRC * NRT * 32;
    int* ridx0 = reinterpret_cast<int*>(pvec + 4 * D_);                 // 2 x kRidx
    int* rps0 = ridx0 + 2 * kRidx;                                      // 2 x NRT x 33
    float* scs0 = reinterpret_cast<float*>(rps0 + 2 * NRT * 33);        // 2 x NRT x 32
    int* tds0 = reinterpret_cast<int*>(scs0 + 2 * NRT * 32);            // 2 x NRT x 4
#pragma unroll 1
    for (int c = tid; c < D_; c += NT) {
        pvec[c] = p.b1[c];
        pvec[D_ + c] = p.b2[c];
        pvec[2 * D_ + c] = p.ln_w[c];
        pvec[3 * D_ + c] = p.ln_b[c];
    }
    const float inv_d = 1.f / (float)D_;
    const int spb = (p.ntiles + NRT - 1) / NRT;
    const long nsuper = (long)spb * p.batch;
    const u32x4* A1 = reinterpret_cast<const u32x4*>(p.wpack);
    const u32x4* A2 = A1 + (size_t)HBT * TK * NS * 64;
    const u32x4* a1b[FB];
    const u32x4* a2b[FB];
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
        a1b[fb] = A1 + (size_t)(fg + fb * FG) * TK * NS * 64;
        a2b[fb] = A2 + (size_t)(fg + fb * FG) * TK * NS * 64;
    }

    auto gather_ids = [&](long st_, int cbw) {
        int* ridx_w = ridx0 + cbw * kRidx;
        int* rps_w = rps0 + cbw * (NRT * 33);
        float* scs_w = scs0 + cbw * (NRT * 32);
        int* tds_w = tds0 + cbw * (NRT * 4);
        const int t0 = (int)(st_ % spb) * NRT;
        if (tid < kRidx) {
            const int s = tid / (NRT * 32), r = tid - s * (NRT * 32);
            const int ti = t0 + (r >> 5);
            int v = -1;
            if (ti < p.ntiles) {
                const TileInfo tk = get_tile(p.tiles, ti, p.rows);
                if (s == 0 && (r & 31) == 0) {
                    tds_w[4 * (r >> 5) + 0] = tk.row0;
                    tds_w[4 * (r >> 5) + 1] = tk.nrows;
                    tds_w[4 * (r >> 5) + 2] = tk.seg0;
                    tds_w[4 * (r >> 5) + 3] = tk.nseg | (tk.split ? NLAM_TILE_SPLIT : 0);
                }
                if ((r & 31) < tk.nrows) {
                    const int row = tk.row0 + (r & 31);
                    const int32_t* ix = p.src[s].idx;
                    v = ix != nullptr ? ix[row] : row;
                }
            } else if (s == 0 && (r & 31) == 0) {
                tds_w[4 * (r >> 5) + 0] = 0;
                tds_w[4 * (r >> 5) + 1] = 0;
                tds_w[4 * (r >> 5) + 2] = 0;
                tds_w[4 * (r >> 5) + 3] = 0;
            }
            ridx_w[tid] = v;
        }
        if (tid < NRT * 33) {
            const int k = tid / 33, l = tid - k * 33;
            const int ti = t0 + k;
            int rpv = 0;
            float sc = 1.f;
            if (ti < p.ntiles) {
                const TileInfo tk = get_tile(p.tiles, ti, p.rows);
                if (!tk.split && l <= tk.nseg) rpv = p.rowptr[tk.seg0 + l];
                if (l < tk.nseg && (p.flags & NLAM_F_MEAN)) sc = p.inv_deg[tk.seg0 + l];
            }
            rps_w[tid] = rpv;
            if (l < 32) scs_w[k * 32 + l] = sc;
        }
    };
    // staging: slot -> (row tile, K group, fragment lane); the gathered edge rows, 8 floats per slot
    auto stage_load = [&](int c0, f32x4(&v)[SL][2], const int* rx, int bb) {
        const float* base = p.src[0].ptr + (long)bb * p.src[0].bstride;
#pragma unroll
        for (int k = 0; k < SL; ++k) {
            const int slot = tid + k * NT;
            const int ln = slot & 63, g = (slot >> 6) % KG, rt = slot / (64 * KG);
            const int rid = rx[rt * 32 + (ln & 31)];
            const float* row = rid >= 0 ? base + (long)rid * D_ + (c0 + 16 * g + 8 * (ln >> 5)) : g_zero16;
            v[k][0] = *reinterpret_cast<const f32x4*>(row);
            v[k][1] = *reinterpret_cast<const f32x4*>(rid >= 0 ? row + 4 : g_zero16);
        }
    };
    auto stage_store = [&](u32x4* Xb, const f32x4(&v)[SL][2]) {
#pragma unroll
        for (int k = 0; k < SL; ++k) {
            const int slot = tid + k * NT;
            float x[8];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                x[c] = v[k][0][c];
                x[4 + c] = v[k][1][c];
            }
            const BfFrag<NS> f = split8<NS>(x);
            const int ln = slot & 63, gr = slot >> 6;   // gr = rt * KG + g
#pragma unroll
            for (int pa = 0; pa < NS; ++pa) Xb[((size_t)gr * NS + pa) * 64 + ln] = f.t[pa];
        }
    };
    auto lds_tile = [&](const int* tds_c, int k) {
        TileInfo t;
        t.row0 = tds_c[4 * k + 0];
        t.nrows = tds_c[4 * k + 1];
        t.seg0 = tds_c[4 * k + 2];
        t.split = (tds_c[4 * k + 3] & NLAM_TILE_SPLIT) != 0;
        t.nseg = tds_c[4 * k + 3] & ~NLAM_TILE_SPLIT;
        return t;
    };

    AFrag<NS, FB> ring[RD];
#pragma unroll
    for (int u = 0; u < RD; ++u) load_aring<NS, FB>(ring[u], a1b, u, lane);

    const long st_first = xcd_slot((int)blockIdx.x, (int)gridDim.x);
    int cb = 0;
    if (st_first < nsuper) gather_ids(st_first, 0);
    __syncthreads();
    {
        f32x4 sv0[SL][2];
        if (st_first < nsuper) {
            stage_load(0, sv0, ridx0, (int)(st_first / spb));
            stage_store(Xp, sv0);
        }
    }
    __syncthreads();

#pragma unroll 1
    for (long st = st_first; st < nsuper; st += gridDim.x) {
        const int b = (int)(st / spb);
        const long st_next = st + gridDim.x < nsuper ? st + gridDim.x : st;   // (a workgroup's last tile asks for itself again)
        const int b_next = (int)(st_next / spb);
        const int* ridx = ridx0 + cb * kRidx;
        const int* rps = rps0 + cb * (NRT * 33);
        const float* scs = scs0 + cb * (NRT * 32);
        const int* tds = tds0 + cb * (NRT * 4);
        const int* ridx_n = ridx0 + (cb ^ 1) * kRidx;

        // ---- GEMM1: the addend rows are the initial accumulators ----
        f32x16 acc1[FB][RT];
        {
            f32x16 add2[FB][RT];
#pragma unroll
            for (int k = 1; k <= 2; ++k) {
                const float* base = p.src[k].ptr + (long)b * p.src[k].bstride;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int rid = ridx[k * (NRT * 32) + rt * 32 + j];
                    const float* row = rid >= 0 ? base + (long)rid * D_ : nullptr;
#pragma unroll
                    for (int fb = 0; fb < FB; ++fb) {
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) {
                            const f32x4 a = load_chunk_v<true>(row, D_, (fg + fb * FG) * 4 + tt, hi, rid >= 0);
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                if (k == 1) acc1[fb][rt][4 * tt + c] = a[c];
                                else add2[fb][rt][4 * tt + c] = a[c];
                            }
                        }
                    }
                }
            }
            f32x4 sv[SL][2];
            if constexpr (NCH > 1) stage_load(16 * KG, sv, ridx, b);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc1[fb][rt][r] += add2[fb][rt][r];
            int kg = 0;
#pragma unroll 1
            for (int ch = 0; ch < NCH; ++ch) {
                const u32x4* Xb = ch == 0 ? Xp : Xf + (size_t)((ch - 1) & 1) * kXfVec;
#pragma unroll 1
                for (int g = 0; g < KG; g += RD) {
#pragma unroll
                    for (int u = 0; u < RD; ++u) {
                        u32x4 bq[NS][RT];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                            for (int pa = 0; pa < NS; ++pa) bq[pa][rt] = Xb[(((size_t)rt * KG + g + u) * NS + pa) * 64 + lane];
                        mma_frags<NS, FB, RT>(acc1, ring[u], bq);
                        const int nxt = kg + g + u + RD;
                        const bool wrap = nxt >= TK;
                        const u32x4* nb[FB];
#pragma unroll
                        for (int fb = 0; fb < FB; ++fb) nb[fb] = wrap ? a2b[fb] : a1b[fb];
                        load_aring<NS, FB>(ring[u], nb, wrap ? nxt - TK : nxt, lane);
                    }
                }
                kg += KG;
                if (ch + 1 < NCH) {
                    stage_store(Xf + (size_t)(ch & 1) * kXfVec, sv);
                    if (ch + 2 < NCH) stage_load(16 * KG * (ch + 2), sv, ridx, b);
                }
                __syncthreads();   // the next chunk is published; after the last one: every wave is done with the staged input
            }
        }

        // ---- publish: bias, save the pre-activation, SiLU, hidden fragments of both row tiles ----
        TileInfo tl[RT];
        bool valid[RT];
        int prow[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            tl[rt] = lds_tile(tds, rt);
            valid[rt] = j < tl[rt].nrows;
            prow[rt] = tl[rt].row0 + j;
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const size_t zrow_id = (size_t)b * p.rows + prow[rt];
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
                f32x16 z16;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const f32x4 z = acc_chunk(acc1[fb][rt], tt) + *reinterpret_cast<const f32x4*>(&pvec[8 * (blk * 4 + tt) + 4 * hi]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) z16[4 * tt + c] = z[c];
                }
                if (p.z1 != nullptr) {
                    if constexpr (SBF) {
                        store_block_bf16(reinterpret_cast<bf16s_t*>(p.z1) + zrow_id * D_, 32 * blk, hi, valid[rt], z16);
                    } else {
                        float* z1row = p.z1 + zrow_id * D_;
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) store_chunk_v<true>(z1row, D_, blk * 4 + tt, hi, valid[rt], acc_chunk(z16, tt));
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float x[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) x[q] = silu_f(z16[8 * h + q]);
                    const BfFrag<NS> f = split8<NS>(x);
#pragma unroll
                    for (int pa = 0; pa < NS; ++pa) Hf[(((size_t)rt * TK + 2 * blk + h) * NS + pa) * 64 + lane] = f.t[pa];
                }
            }
        }
        __syncthreads();
        // the next super tile's row ids / row pointers / descriptors (visible behind the LayerNorm barriers); their dependent loads
        // run under GEMM2
        gather_ids(st_next, cb ^ 1);

        // ---- GEMM2, both row tiles ----
        f32x16 acc2[FB][RT];
#pragma unroll
        for (int fb = 0; fb < FB; ++fb)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc2[fb][rt][r] = 0.f;
#pragma unroll 1
        for (int kg = 0; kg < TK; kg += RD) {
#pragma unroll
            for (int u = 0; u < RD; ++u) {
                u32x4 hq[NS][RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int pa = 0; pa < NS; ++pa) hq[pa][rt] = Hf[(((size_t)rt * TK + kg + u) * NS + pa) * 64 + lane];
                mma_frags<NS, FB, RT>(acc2, ring[u], hq);
                const int nxt = kg + u + RD;
                const bool wrap = nxt >= TK;
                const u32x4* nb[FB];
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) nb[fb] = wrap ? a1b[fb] : a2b[fb];
                load_aring<NS, FB>(ring[u], nb, wrap ? nxt - TK : nxt, lane);
            }
        }

        // ---- bias 2 + LayerNorm (row statistics across the 8 waves) ----
        float sum[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            sum[rt] = 0.f;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const f32x4 bias = *reinterpret_cast<const f32x4*>(&pvec[D_ + 8 * (blk * 4 + tt) + 4 * hi]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float v = acc2[fb][rt][4 * tt + c] + bias[c];
                        acc2[fb][rt][4 * tt + c] = v;
                        sum[rt] += v;
                    }
                }
            }
            const float s = row_allreduce(sum[rt]);
            if (hi == 0) red[(fg * NRT + rt) * 32 + j] = s;
        }
        __syncthreads();   // also: every wave is done reading the hidden fragments (the region becomes the staging blocks)
        float rstd[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < FG; ++w) tot += red[(w * NRT + rt) * 32 + j];
            const float mean = tot * inv_d;
            float sq = 0.f;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float dlt = acc2[fb][rt][r] - mean;
                    acc2[fb][rt][r] = dlt;
                    sq += dlt * dlt;
                }
            sq = row_allreduce(sq);
            if (hi == 0) red[((FG + fg) * NRT + rt) * 32 + j] = sq;
        }
        __syncthreads();
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float tot2 = 0.f;
#pragma unroll
            for (int w = 0; w < FG; ++w) tot2 += red[((FG + w) * NRT + rt) * 32 + j];
            rstd[rt] = rsqrtf(tot2 * inv_d + p.eps);
            if (p.rstd != nullptr && valid[rt] && hi == 0 && fg == 0) p.rstd[(size_t)b * p.rows + prow[rt]] = rstd[rt];
        }

        // ---- the next super tile's first chunk: requested here, flies under the epilogue ----
        f32x4 svn[SL][2];
        stage_load(0, svn, ridx_n, b_next);
        __builtin_amdgcn_sched_barrier(0);

        // ---- epilogue, per row tile and 32-column block: xhat, affine, aggregate, edge update ----
        float* out_b = p.aggr + (size_t)b * p.nseg_total * D_;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const size_t xrow_id = (size_t)b * p.rows + prow[rt];
            const float* srow0 = nullptr;
            float* orow = nullptr;
            if (p.out != nullptr && valid[rt]) {
                srow0 = p.src[0].ptr + (long)b * p.src[0].bstride + (long)ridx[rt * 32 + j] * D_;
                const long oidx = p.out_idx != nullptr ? p.out_idx[prow[rt]] : prow[rt];
                orow = p.out + (long)b * p.out_bstride + oidx * (long)D_;
            }
            const bool add0 = (p.flags & NLAM_F_ADD_SRC0) != 0 && orow != nullptr;
            int raw_ptr = 0;
            float my_scale = 1.f;
            if (lane <= 32) raw_ptr = rps[rt * 33 + lane];
            if (lane < 32) my_scale = scs[rt * 32 + lane];
            f32x4 res[2][4];
            auto request = [&](int fb, f32x4(&dst)[4]) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) dst[tt] = load_chunk_v<true>(srow0, D_, (fg + fb * FG) * 4 + tt, hi, add0);
            };
            request(0, res[0]);
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
                if (fb + 1 < FB) request(fb + 1, res[(fb + 1) & 1]);
                f32x16 xh16;
#pragma unroll
                for (int r = 0; r < 16; ++r) xh16[r] = acc2[fb][rt][r] * rstd[rt];
                if (p.xhat != nullptr) {
                    if constexpr (SBF) {
                        store_block_bf16(reinterpret_cast<bf16s_t*>(p.xhat) + xrow_id * D_, 32 * blk, hi, valid[rt], xh16);
                    } else {
                        float* xrow = p.xhat + xrow_id * D_;
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) store_chunk_v<true>(xrow, D_, blk * 4 + tt, hi, valid[rt], acc_chunk(xh16, tt));
                    }
                }
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int c0 = 8 * (blk * 4 + tt) + 4 * hi;
                    const f32x4 g = *reinterpret_cast<const f32x4*>(&pvec[2 * D_ + c0]);
                    const f32x4 be = *reinterpret_cast<const f32x4*>(&pvec[3 * D_ + c0]);
                    f32x4 m;
#pragma unroll
                    for (int c = 0; c < 4; ++c) m[c] = xh16[4 * tt + c] * g[c] + be[c];
                    *reinterpret_cast<f32x4*>(&stg[j * kStgStride + 8 * tt + 4 * hi]) = valid[rt] ? m : f32x4{0.f, 0.f, 0.f, 0.f};
                    if (orow != nullptr) store_chunk_v<true>(orow, D_, blk * 4 + tt, hi, valid[rt], m + res[fb & 1][tt]);
                }
                wave_lds_sync();
                if (tl[rt].nseg > 0) block_segment_reduce(stg, tl[rt], raw_ptr, my_scale, out_b + 32 * blk, D_, 32, lane);
                wave_lds_sync();
            }
        }
        stage_store(Xp, svn);   // (the only reader of Xp, GEMM1's first chunk, is long done)
        __syncthreads();        // tile end: Xp, the staging region and red are reused
        cb ^= 1;
    }
}

// LDS bytes of mlp_fwd_edge_kernel<NS, D_, .>
template <int NS, int D_>
constexpr size_t fwd_edge_lds() {
    constexpr size_t TK = D_ / 16, KG = NS == 1 ? 16 : 8, NRT = 2;
    constexpr size_t xf = NRT * KG * NS * 64 * 16, hf = NRT * TK * NS * 64 * 16;
    constexpr size_t r0 = hf > 2 * xf ? hf : 2 * xf;
    return r0 + xf + (size_t)2 * 8 * NRT * 32 * 4 + (size_t)4 * D_ * 4 + (size_t)2 * (NLAM_MAX_SRC * NRT * 32 + NRT * 69) * 4;
}

struct WbfPlan {
    int cfg;       // 0 = not covered; 1: <8,4,1,4,2> (d <= 128)  2: <8,8,1,4,2> (d <= 256)  3: <8,8,2,2,1> (d <= 512)
                   // 4: <8,8,1,2,2> (d <= 256, 64-row super tiles for mid-size launches)
    int nw, fg, nrt, kg, pt;
};
constexpr long kWbfSmallMinSupertiles = 24;   // of 64 rows: below that the fp32 one-tile kernels win

WbfPlan wbf_plan(int maxw, int ns = 3) {
    const int sl = ns == 1 ? 2 : 1;   // staging slots per thread relative to the three-term kernels (WbfShape::SL)
    if (maxw <= 128) return {1, 8, 4, 8, 2 * sl, 4};
    if (maxw <= 256) return {2, 8, 8, 4, 4 * sl, 2};
    if (maxw <= kMaxWide) return {3, 8, 8, 2, 8 * sl, 1};
    return {0, 0, 0, 0, 0, 0};
}

// Half-size plans (NLAM_TUNE_WBF_HALF): 4-wave workgroups on half the rows, two co-resident per CU.  The 8-wave kernels are
// bulk-synchronous -- every CU gathers, then every CU multiplies, then every CU stores (64 % of the wave-cycles of the d = 512
// one-term kernels were waits) -- and their waves hold the whole register file, so nothing else can run beside them.  Two
// independent workgroups per CU drift out of phase: one's HBM-bound gather / store phases run under the other's GEMMs.
//   5: <NS,4,4,2,2,1> (128 < d <= 256, 64 rows)   6: <1,4,4,4,1,1> (d <= 512, one term, 32 rows)
// Measured (round 4, profiles/round4/ab_half_workgroups.log): the gain is what de-synchronising the phases is worth, not more --
// two workgroups of 4 waves are still two waves per SIMD.  One term: forward d = 256 131 -> 118 us (m2m), d = 512 980 -> 859 us
// (m2g), cfg5 177.8 -> 171.1 ms; three terms: no change (167 vs 166 us); backward: no change at either; d = 128 (cfg4) slower
// (11.56 -> 11.99 ms: no instantiation).  Default: forward on (bit 0), backward off.
WbfPlan wbf_half_plan(int maxw, int ns) {
    if (maxw <= 128) return {0, 0, 0, 0, 0, 0};
    if (maxw <= 256) return {5, 4, 4, 2, 4, 1};
    // 7 (NLAM_TUNE_WBF_HALF bit 2, round 6): <1,4,4,4,2,2>, 64 rows, one pass -- an A fragment fetched from L2 feeds two MFMAs instead of one.
    // At one term the GEMM phases of plan 6 are bound by the weight stream: 1 KiB of L2 traffic per MFMA, 1.9 GB per m2m launch,
    // GEMM1 + GEMM2 = 66k of 167k wave-cycles per 32-row super tile against an MFMA floor of 8k (profiles/round6/phase_cycles_wide.txt)
    if (maxw <= kMaxWide && ns == 1) return (::nlam_detail::wbf_half & 4) ? WbfPlan{7, 4, 4, 2, 4, 2} : WbfPlan{6, 4, 4, 1, 8, 1};
    return {0, 0, 0, 0, 0, 0};
}

// launch shape of the split-bf16 forward for this problem (cfg 0 = run the fp32 kernels of nlam_wide.inc)
WbfPlan fwd_wbf_choose(const nlam_mlp_fwd_t* p, int ns) {
    const int maxw = p->hid > p->dout ? p->hid : p->dout;
    const WbfPlan pl = wbf_plan(maxw, ns);
    if (pl.cfg == 0) return pl;
    // 128-row super tiles need enough tiles to occupy the chip: the mesh-level launches of the MEPS graphs (6 561
    // rows = 206 tiles) are faster on the one-tile-per-workgroup fp32 kernels (55 vs 89 us at d = 256)
    // d > 256: the fp32 <8,2> instantiation spills and streams 4 MB of weights per tile (6 561 rows at d = 512:
    // 433 us against 78 us here), so the super-tile kernels take every launch of at least 8 super tiles
    const long tiles = (long)p->ntiles * p->batch;
    long min_st = ::nlam_detail::wbf_min_supertiles;
    if (pl.cfg == 3 && min_st > 8) min_st = 8;
    if (tiles >= min_st * pl.nrt) {
        if (::nlam_detail::wbf_half & 1) {
            const WbfPlan hp = wbf_half_plan(maxw, ns);
            if (hp.cfg != 0) return hp;
        }
        return pl;
    }
    if (pl.cfg == 2 && tiles >= kWbfSmallMinSupertiles * 2) {   // mid-size launches at 128 < d <= 256: 64-row super tiles
        const int sl = ns == 1 ? 2 : 1;
        return {4, 8, 8, 2, 8 * sl, 2};
    }
    return {0, 0, 0, 0, 0, 0};
}

// split terms the wide forward may use for this launch (0 = fp32 kernels of nlam_wide.inc)
int fwd_wbf_ns(const nlam_mlp_fwd_t* p) {
    int ns = (int)((p->flags & NLAM_F_MM_MASK) >> NLAM_F_MM_SHIFT);
    if (ns == 0) return 0;
    if (fwd_wbf_choose(p, 3).cfg == 0) return 0;
    for (int s = 0; s < p->nsrc; ++s)
        if (p->src[s].width % 4 != 0) return 0;
    if (p->hid % 4 != 0) return 0;
    // the aggregation of these kernels (block_segment_reduce) writes whole float4s of a receiver's row: with an output width that
    // is no multiple of 4 its last dout % 4 columns would never be written -- the fp32 kernels reduce element by element
    if (p->aggr != nullptr && p->dout % 4 != 0) return 0;
    if (p->flags & NLAM_F_PRE_ADD)   // addends of width hid, whole 32-feature blocks, no PropagationNet sender term
        for (int s = 1; s < p->nsrc; ++s)
            if (p->src[s].width != p->hid || p->hid % 32 != 0 || (p->flags & NLAM_F_ADD_SRC1)) return 0;
    if (ns == 1 && (((p->hid + 31) / 32) & 1)) return 3;   // the one-term A ring holds 4 K groups: GEMM2 has 2 per hidden block
    return ns == 2 ? 3 : ns;   // two terms are not instantiated for the wide shapes: use the fp32-class path
}

// NLAM_F_STORE_BF16 for this launch: the one-term super-tile forward with a bf16-storage instantiation (plans 2, 3, 5, 6), whole
// 32-column blocks of hid and dout, and shapes whose backward and weight gradients take the one-term split-bf16 kernels too --
// the same tiles / batch put the backward above its own (lower) super-tile threshold, widths above 64 and multiples of 4 make
// both weight gradients wide, and a source of <= kSmallN columns (the streaming weight-gradient kernel) is excluded.
template <typename P>
bool mlp_is_wide(const P* p);   // nlam_hip.hip

bool store_bf16_ok(const nlam_mlp_fwd_t* p) {
    if (p->ncat != 0 || !mlp_is_wide(p) || fwd_wbf_ns(p) != 1) return false;
    if (p->hid % 32 != 0 || p->dout % 32 != 0 || p->hid <= 64 || p->dout <= 64) return false;
    if (((p->dout + 31) / 32) & 1) return false;   // the backward's W2^T phase is padded for odd counts, but keep to tested shapes
    if (p->flags & NLAM_F_NO_ACT) return false;
    for (int s = 0; s < p->nsrc; ++s)
        if (p->src[s].width % 4 != 0 || p->src[s].width <= 8) return false;
    const WbfPlan pl = fwd_wbf_choose(p, 1);
    return pl.cfg == 2 || pl.cfg == 3 || pl.cfg == 5 || pl.cfg == 6 || pl.cfg == 7;
}

int fwd_wbf_tk1(const nlam_mlp_fwd_t* p, int kg) {
    int t = 0;
    const int ngemm = (p->flags & NLAM_F_PRE_ADD) ? 1 : p->nsrc;
    for (int s = 0; s < ngemm; ++s) t += ((p->src[s].width + 16 * kg - 1) / (16 * kg)) * kg;
    return t;
}

int64_t fwd_wbf_wpack_floats(const nlam_mlp_fwd_t* p, int ns) {
    const WbfPlan pl = fwd_wbf_choose(p, ns);
    if (pl.cfg == 0) return 0;
    const int64_t HBT = (p->hid + 31) / 32, OBT = (p->dout + 31) / 32;
    return (HBT * fwd_wbf_tk1(p, pl.kg) + OBT * 2 * HBT) * ns * 256;
}

size_t fwd_wbf_lds(const nlam_mlp_fwd_t* p, int ns, const WbfPlan& pl) {
    const size_t HBT = (p->hid + 31) / 32, OBT = (p->dout + 31) / 32;
    const size_t xf = (size_t)2 * pl.nrt * pl.kg * ns * 1024;
    const size_t hf = (size_t)pl.pt * 2 * HBT * ns * 1024;
    size_t r0 = xf;
    if (hf > r0) r0 = hf;
    const size_t dp = (HBT > OBT ? HBT : OBT) * 32;
    const size_t stg = (size_t)pl.nw * 32 * kStgStride * 4;   // per-wave staging blocks, inside the hidden-fragment region
    if (stg > r0) r0 = stg;
    return r0 + (size_t)2 * pl.fg * pl.pt * 32 * 4 + (size_t)NLAM_MAX_SRC * pl.nrt * 32 * 4 + 4 * dp * 4 + (size_t)pl.nrt * 69 * 4;
}

// ---------------------------------------------------------------------------
// weight gradients  dW[m][n] = sum_rows A[row][m] * S[idx(row)][n]  on the split-bf16 cores
// ---------------------------------------------------------------------------
// The reduction dimension of this product is the row index, so both MFMA operands need
// 8 consecutive ROWS of one column per lane: a transposed read of the row-major tensors.
// Thread t of the 256 owns one column of the 128 x 128 output window's operands (waves
// 0,1: the 128 columns of A, waves 2,3: the 128 gathered columns of S) and reads its
// column of a 16-row step with 16 dword loads, each a coalesced 256-byte row segment per
// wave; it splits the two 8-row halves once and writes them as finished A / B fragments
// (fragment order, conflict-free b128) for the four MFMA waves (2 x 2 grid of 64 x 64
// sub-windows, 24 MFMAs per step at NS = 3).  One split per element, no LDS transpose.
// The next step's rows are in flight in registers while the current one is multiplied;
// fragments are double buffered (2 x 8 NS KiB), so three workgroups share a CU.
constexpr int kWbStep = 16;   // rows per MFMA K step

// KS = K steps (16 rows each) staged per barrier.  KS = 1 ships: with one term a step is only 4 MFMAs per wave, but
// KS = 4 measured 8 % slower there (dW1 at d = 256: 439 vs 408 us) -- that launch already moves 3.1 GB (every
// 128 x 128 window re-reads its rows) in 408 us = the HBM roof; wider windows are the lever, not longer stages.
// Window = (WM x 2 blocks) x (WN x NBW blocks) of 32: <2,2,2> = 128 x 128 with 4 waves (three workgroups per CU),
// <4,2,4> = 256 x 256 with 8 waves: every row is then read once per 256 output columns instead of once per 128 x 128
// window -- the 128 x 128 launch at d = 256 moves 3.1 GB for 1.04 GB of distinct rows and sits at the HBM roof.
// ABF / SBFS: the A operand (dz1 / dz2) / the single un-gathered S operand (z1) are rows of bf16 (NLAM_F_A_BF16 / NLAM_F_S_BF16,
// one-term kernels).  A wave stages either A columns or S columns for the whole launch, so the element type of its loads is
// chosen ONCE, outside the stage loop (both sides pass the same barriers).
// (the body takes its workgroup coordinates as arguments: bx / gx = row slice and slice count of ITS problem, by = output window;
// wgrad_wbf_group_kernel binds every workgroup of one grid to one of several problems of the same shape)
template <int NS, bool SILU, int KS, int WM, int WN, int NBW, bool ABF, bool SBFS>
__device__ __forceinline__ void wgrad_wbf_body(const nlam_wgrad_t& p, const unsigned bx, const unsigned gx, const unsigned by) {
    static_assert(!(ABF || SBFS) || NS == 1, "bf16 operands belong to the one-term (autocast) kernels");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int WINM = WM * 64, WINN = WN * NBW * 32;   // window size in columns of A / of S
    constexpr int MBW = WINM / 32, NBT = WINN / 32;       // fragment blocks of A / of S per step
    static_assert(WINM + WINN == WM * WN * 64, "one operand column per thread");
    u32x4* F = reinterpret_cast<u32x4*>(smem);            // 2 x [KS][MBW blocks of A, NBT blocks of S][NS][64]
    constexpr int kStepVec = (MBW + NBT) * NS * 64;
    constexpr int kBufVec = KS * kStepVec;
    constexpr int kRows = KS * kWbStep;                   // rows per stage
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, hi = lane >> 5;

    // decode the output window (same enumeration as wgrad_wide_kernel)
    const int mwins = (p.m + WINM - 1) / WINM;
    const int mw = by % mwins;
    int nwi = by / mwins;
    int s_sel = 0, off = 0;
    for (int s = 0; s < p.nsrc; ++s) {
        const int w = get_src(p, s).width;
        const int nws = (w + WINN - 1) / WINN;
        if (nwi < nws) {
            s_sel = s;
            break;
        }
        nwi -= nws;
        off += w;
    }
    const nlam_src_t S = get_src(p, s_sel);
    const int m0 = mw * WINM, mcols = min(WINM, p.m - m0);
    const int n0 = nwi * WINN, ncols = min(WINN, S.width - n0);
    const int gcol0 = off + n0;

    // staging role of this thread: waves [0, WINM/64) hold the columns of A, the rest those of S
    const bool is_b = wave >= WINM / 64;
    const int col = is_b ? tid - WINM : tid;                // column inside the window's A or S operand
    const bool col_ok = col < (is_b ? ncols : mcols);
    const int fblk = (is_b ? MBW : 0) + (col >> 5);         // fragment block it writes
    const int flane = col & 31;

    const int stages_per_batch = (p.rows + kRows - 1) / kRows;
    const long total_stages = (long)stages_per_batch * p.batch;

    // lane q < kRows: gathered row id of row q of the stage (-1 = past the end)
    auto load_idxv = [&](long st) -> int {
        const int r = (int)(st % stages_per_batch) * kRows + lane;
        int v = -1;
        if (lane < kRows && r < p.rows) v = (is_b && S.idx != nullptr) ? S.idx[r] : r;
        return v;
    };
    // A bf16 operand is staged with another thread -> data mapping: thread = (pair of adjacent columns, 8-row half of the stage),
    // 8 dword loads of two bf16 each (a wave covers 256-byte row segments, as the fp32 mapping does; 2-byte loads ran 3.3x
    // slower) instead of (one column, 16 rows); it writes two fragment entries of one 8-row half.  The half is uniform per wave.
    static_assert(!(ABF || SBFS) || KS == 1, "bf16 operand staging is written for one K step per stage");
    const int wop = is_b ? WINN : WINM;                    // columns of this thread's operand in the window
    const int ct = is_b ? tid - WINM : tid;
    const int cpair = ct % (wop / 2), rhalf = __builtin_amdgcn_readfirstlane(ct / (wop / 2));
    auto load_rows = [&](auto half_c, long st, int idxv, float(&v)[kRows]) {
        constexpr bool half = decltype(half_c)::value;   // this wave's operand is stored as bf16
        const int b = (int)(st / stages_per_batch);
        const long ld = is_b ? S.width : p.m;
        if constexpr (half) {
            const long boff = is_b ? (long)b * S.bstride + n0 + 2 * cpair : (long)((size_t)b * p.rows * p.m) + m0 + 2 * cpair;
            const unsigned* base32 = reinterpret_cast<const unsigned*>(reinterpret_cast<const bf16s_t*>(is_b ? S.ptr : p.A) + boff);
            const bool ok = 2 * cpair < (is_b ? ncols : mcols);   // widths are multiples of 4: a pair is inside or outside as a whole
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int rid = __builtin_amdgcn_readlane(idxv, 8 * rhalf + q);
                const unsigned w = (rid >= 0 && ok) ? base32[((long)rid * ld) >> 1] : 0u;
                v[q] = __builtin_bit_cast(float, w << 16);
                v[8 + q] = __builtin_bit_cast(float, w & 0xffff0000u);
            }
        } else {
            const long boff = is_b ? (long)b * S.bstride + n0 + col : (long)((size_t)b * p.rows * p.m) + m0 + col;
            const float* base = (is_b ? S.ptr : p.A) + boff;
#pragma unroll
            for (int q = 0; q < kRows; ++q) {
                const int rid = __builtin_amdgcn_readlane(idxv, q);
                v[q] = (rid >= 0 && col_ok) ? base[(long)rid * ld] : 0.f;
            }
        }
    };
    auto store_frags = [&](auto half_c, u32x4* Fb, const float(&v)[kRows]) {
        constexpr bool half = decltype(half_c)::value;
#pragma unroll
        for (int h = 0; h < 2 * KS; ++h) {
            float x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                x[q] = v[8 * h + q];
                if constexpr (SILU) {
                    if (is_b) x[q] = silu_f(x[q]);
                }
            }
            const BfFrag<NS> f = split8<NS>(x);
            if constexpr (half) {   // h = column of the pair; the 8 rows are half `rhalf` of the stage
                const int c2 = 2 * cpair + h;
                Fb[((size_t)((is_b ? MBW : 0) + (c2 >> 5)) * NS) * 64 + (c2 & 31) + 32 * rhalf] = f.t[0];
            } else {
#pragma unroll
                for (int pa = 0; pa < NS; ++pa) Fb[(size_t)(h >> 1) * kStepVec + ((size_t)fblk * NS + pa) * 64 + flane + 32 * (h & 1)] = f.t[pa];
            }
        }
    };

    const int wm = wave / WN, wn = wave % WN;
    f32x16 acc[2][NBW];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < NBW; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

    auto run = [&](auto half_c) {
        long st = bx;
        int buf = 0;
        float v[kRows];
        int idxv = -1;
        if (st < total_stages) {
            idxv = load_idxv(st);
            load_rows(half_c, st, idxv, v);
            store_frags(half_c, F, v);
            if (st + gx < total_stages) {
                idxv = load_idxv(st + gx);
                load_rows(half_c, st + gx, idxv, v);
            }
            if (st + 2 * (long)gx < total_stages) idxv = load_idxv(st + 2 * (long)gx);
        }
        __syncthreads();
        for (; st < total_stages; st += gx) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const u32x4* Fb = F + (size_t)buf * kBufVec + (size_t)ks * kStepVec;
                u32x4 a[NS][2], bq[NS][NBW];
#pragma unroll
                for (int pa = 0; pa < NS; ++pa) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) a[pa][u] = Fb[((size_t)(2 * wm + u) * NS + pa) * 64 + lane];
#pragma unroll
                    for (int u = 0; u < NBW; ++u) bq[pa][u] = Fb[((size_t)(MBW + NBW * wn + u) * NS + pa) * 64 + lane];
                }
#pragma unroll
                for (int ord = NS - 1; ord >= 0; --ord)
#pragma unroll
                    for (int pa = 0; pa <= ord; ++pa)
#pragma unroll
                        for (int u = 0; u < 2; ++u)
#pragma unroll
                            for (int w2 = 0; w2 < NBW; ++w2) acc[u][w2] = MFMA_BF16(a[pa][u], bq[ord - pa][w2], acc[u][w2]);
            }
            const bool has1 = st + gx < total_stages;
            const bool has2 = st + 2 * (long)gx < total_stages;
            if (has1) store_frags(half_c, F + (size_t)(buf ^ 1) * kBufVec, v);
            if (has2) {
                load_rows(half_c, st + 2 * (long)gx, idxv, v);
                if (st + 3 * (long)gx < total_stages) idxv = load_idxv(st + 3 * (long)gx);
            }
            __syncthreads();
            buf ^= 1;
        }
    };
    // fp32 operands, one K step per stage: BALANCED staging -- every thread stages one (column, 8-row half) unit of A and one of
    // S (same column index, rows 8 rhalf2 .. + 7: uniform per wave), 8 + 8 dword loads.  With the role split above the S waves
    // alone applied SiLU to their 16 values per stage (dW2 = dz2^T silu(z1)) while the A waves waited at the barrier: dW2 ran 2x
    // as long as dW1 on the same shapes (77.6 vs 39.1 us at 57 616 x 256 x 256, profiles/round4/pmc_wide_d256_x3.md).
    constexpr int W2 = WINM;                               // == WINN == half the workgroup
    static_assert(WINM == WINN, "balanced staging: as many A as S columns per window");
    const int col2 = tid % W2, rhalf2 = __builtin_amdgcn_readfirstlane(tid / W2);
    auto run_balanced = [&]() {
        struct Idx2 { int a, s; };
        auto load_idx2 = [&](long st) -> Idx2 {
            const int r = (int)(st % stages_per_batch) * kRows + lane;
            Idx2 v = {-1, -1};
            if (lane < kRows && r < p.rows) {
                v.a = r;
                v.s = S.idx != nullptr ? S.idx[r] : r;
            }
            return v;
        };
        auto load2 = [&](long st, Idx2 ix, float(&v)[kRows]) {
            const int b = (int)(st / stages_per_batch);
            const float* ba = p.A + (size_t)b * p.rows * p.m + m0 + col2;
            const float* bs = S.ptr + (long)b * S.bstride + n0 + col2;
            const bool oka = col2 < mcols, oks = col2 < ncols;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int ra = __builtin_amdgcn_readlane(ix.a, 8 * rhalf2 + q), rs = __builtin_amdgcn_readlane(ix.s, 8 * rhalf2 + q);
                v[q] = (ra >= 0 && oka) ? ba[(long)ra * p.m] : 0.f;
                v[8 + q] = (rs >= 0 && oks) ? bs[(long)rs * S.width] : 0.f;
            }
        };
        auto store2 = [&](u32x4* Fb, const float(&v)[kRows]) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {   // 0: the A unit, 1: the S unit
                float x[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    x[q] = v[8 * h + q];
                    if constexpr (SILU) {
                        if (h == 1) x[q] = silu_f(x[q]);
                    }
                }
                const BfFrag<NS> f = split8<NS>(x);
#pragma unroll
                for (int pa = 0; pa < NS; ++pa) Fb[((size_t)((h == 1 ? MBW : 0) + (col2 >> 5)) * NS + pa) * 64 + (col2 & 31) + 32 * rhalf2] = f.t[pa];
            }
        };
        long st = bx;
        int buf = 0;
        float v[kRows];
        Idx2 ix = {-1, -1};
        if (st < total_stages) {
            ix = load_idx2(st);
            load2(st, ix, v);
            store2(F, v);
            if (st + gx < total_stages) {
                ix = load_idx2(st + gx);
                load2(st + gx, ix, v);
            }
            if (st + 2 * (long)gx < total_stages) ix = load_idx2(st + 2 * (long)gx);
        }
        __syncthreads();
        for (; st < total_stages; st += gx) {
            const u32x4* Fb = F + (size_t)buf * kBufVec;
            u32x4 a[NS][2], bq[NS][NBW];
#pragma unroll
            for (int pa = 0; pa < NS; ++pa) {
#pragma unroll
                for (int u = 0; u < 2; ++u) a[pa][u] = Fb[((size_t)(2 * wm + u) * NS + pa) * 64 + lane];
#pragma unroll
                for (int u = 0; u < NBW; ++u) bq[pa][u] = Fb[((size_t)(MBW + NBW * wn + u) * NS + pa) * 64 + lane];
            }
#pragma unroll
            for (int ord = NS - 1; ord >= 0; --ord)
#pragma unroll
                for (int pa = 0; pa <= ord; ++pa)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int w2 = 0; w2 < NBW; ++w2) acc[u][w2] = MFMA_BF16(a[pa][u], bq[ord - pa][w2], acc[u][w2]);
            const bool has1 = st + gx < total_stages;
            const bool has2 = st + 2 * (long)gx < total_stages;
            if (has1) store2(F + (size_t)(buf ^ 1) * kBufVec, v);
            if (has2) {
                load2(st + 2 * (long)gx, ix, v);
                if (st + 3 * (long)gx < total_stages) ix = load_idx2(st + 3 * (long)gx);
            }
            __syncthreads();
            buf ^= 1;
        }
    };
    if constexpr (!(ABF || SBFS) && KS == 1) {
        run_balanced();
    } else if constexpr (ABF != SBFS) {   // the two wave roles read different element types
        if (is_b) run(std::integral_constant<bool, SBFS>{});
        else run(std::integral_constant<bool, ABF>{});
    } else {
        run(std::integral_constant<bool, ABF>{});
    }

    float* P = p.partials + (size_t)bx * p.m * p.n;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w2 = 0; w2 < NBW; ++w2) {
            const int nl = (NBW * wn + w2) * 32 + i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = (2 * wm + u) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (ml < mcols && nl < ncols) P[(size_t)(m0 + ml) * p.n + gcol0 + nl] = acc[u][w2][r];
            }
        }
}

template <int NS, bool SILU, int KS, int WM, int WN, int NBW, bool ABF = false, bool SBFS = false>
__global__ __launch_bounds__(WM * WN * 64) void wgrad_wbf_kernel(const nlam_wgrad_t p) {
    wgrad_wbf_body<NS, SILU, KS, WM, WN, NBW, ABF, SBFS>(p, blockIdx.x, gridDim.x, blockIdx.y);
}

// Grouped launch (nlam_wgrad_group): the weight gradients of the chunks of a SplitMLPs layer (hi_lam_parallel.py:127-143) are
// 3 .. 200 row slices each; a launch apiece was 21 launches of 8-50 us per edge stage on the side queues -- more than the
// chain they were moved off could hide (the chain's next kernel waits behind them whenever it lands on their queue).
struct wgrad_group_t {
    nlam_wgrad_t g[NLAM_MAX_GROUP];
    int n;
    int first[NLAM_MAX_GROUP + 1];   // first row slice (blockIdx.x) of each member; first[n] = gridDim.x
};
template <int NS, bool SILU, int WM, int WN, int NBW>
__global__ __launch_bounds__(WM * WN * 64) void wgrad_wbf_group_kernel(const wgrad_group_t G) {
    int gi = 0;
#pragma unroll
    for (int k = 1; k < NLAM_MAX_GROUP; ++k)
        if (k < G.n && (int)blockIdx.x >= G.first[k]) gi = k;
    wgrad_wbf_body<NS, SILU, 1, WM, WN, NBW, false, false>(G.g[gi], blockIdx.x - G.first[gi], G.first[gi + 1] - G.first[gi], blockIdx.y);
}

// ---------------------------------------------------------------------------
// Round 6: one-term weight gradients with both operands streamed by LDS-DMA (wgrad_ldma_kernel)
// ---------------------------------------------------------------------------
// wgrad_wbf_body gives every thread one operand COLUMN and reads it with one dword load per row: per MFMA 23 vector + 21 scalar
// instructions (readlane of the row id, 64-bit address arithmetic, widening, the bf16 split) -- issue-bound at 0.11 of the matrix
// peak and 0.25 of HBM (profiles/round4/pmc_wide_d512_bf16.md: dW = 512 x 512 over 57 616 rows in 108-119 us).  Here no thread
// touches a row on its way in:
//  * a stage = R rows of the window's 256 A columns and 256 S columns, fetched by global_load_lds_dwordx4 (16 bytes per lane,
//    1 KiB per wave instruction, whole 128-byte lines, per-lane gathered source address) into a ring of NBUF = 3 stages; the
//    wave waits with a COUNTED vmcnt (the next stage stays in flight across the barrier: raw s_barrier, no __syncthreads --
//    cdna_hip_programming.md section 5, "pipelining across barriers");
//  * bf16 operands (dz1 / dz2 / z1 of a layer running with NLAM_F_STORE_BF16) land as [8 rows][64 columns] pieces whose 16-byte
//    slots are permuted on the SOURCE side (slot ^ 4 for rows 2, 3, 6, 7 of a piece: the LDS image of an LDS-DMA is lane-linear)
//    so that ds_read_b64_tr_b16 -- the LDS transpose read: a 16-lane group reads a [4 rows][16 columns] block and lane i
//    receives column i's four rows (tools/probes/tr16_probe.hip, profiles/round6/tr16_probe.log) -- delivers an MFMA fragment
//    (8 consecutive ROWS of one column per lane, rows = K) in two conflict-free instructions;
//  * fp32 operands (the layer's input rows) land row-major and are read as 8 conflict-free dwords per fragment + 4 conversions;
//  * dW2's SiLU is applied once per element, in place in LDS, between two barriers (not once per consuming wave).
// Window, row slices, partial-sum layout and the order of the 16-row K steps inside a workgroup are those of wgrad_wbf_body's
// 256 x 256 instantiation; a workgroup takes R-row stages bx, bx + gx, ..
template <bool ABF, bool SBF, bool SILU, int R_, int NBUF_>
struct WgLdma {
    static constexpr int R = R_;                                  // rows per stage (16 or 32)
    static constexpr int A_ROWB = ABF ? 512 : 1024;               // bytes of a tile row (256 columns)
    static constexpr int S_ROWB = SBF ? 512 : 1024;
    static constexpr int A_TILE = R * A_ROWB, S_TILE = R * S_ROWB;
    static constexpr int STAGE = A_TILE + S_TILE;
    // ring depth: two stages in flight behind the one being multiplied; with SiLU one more, so that the in-place SiLU pass of
    // stage k + 1 runs in the SAME barrier interval as the products of stage k (no second barrier, VALU beside MFMA)
    static constexpr int NBUF = NBUF_;
    static_assert(NBUF_ >= (SILU ? 4 : 3), "ring depth");
    static_assert(R_ == 16 || R_ == 32, "one or two K steps per stage");
    static constexpr int A_IPW = A_TILE / 8192, S_IPW = S_TILE / 8192;   // LDS-DMA instructions per wave and stage (8 waves, 1 KiB each)
    static constexpr int IPS = A_IPW + S_IPW;
    static constexpr size_t LDS = (size_t)NBUF * STAGE;
};

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

// The transpose reads of one 16-row K step, with their wait, as ONE asm statement (early-clobber outputs): hipcc treats the
// ds_read_tr16 builtin as a read of anything an LDS-DMA in flight may write and puts s_waitcnt vmcnt(0) in front of it, which
// drains the stage that was requested a moment ago (seen in the ISA; plain ds_read instructions are not affected).
// (A: two fragments at aA0 / aA1; S: four fragments, block pairs at +0 / +1024 of aS0 / aS1; the second half of a fragment = rows + 4 = +512)
#define NLAM_TR_STEP_AS(K0, K1, K2, K3)                                                                                   \
    asm volatile("ds_read_b64_tr_b16 %0, %12 offset:" #K0 "\n\tds_read_b64_tr_b16 %1, %12 offset:" #K1 "\n\t"             \
                 "ds_read_b64_tr_b16 %2, %13 offset:" #K0 "\n\tds_read_b64_tr_b16 %3, %13 offset:" #K1 "\n\t"             \
                 "ds_read_b64_tr_b16 %4, %14 offset:" #K0 "\n\tds_read_b64_tr_b16 %5, %14 offset:" #K1 "\n\t"             \
                 "ds_read_b64_tr_b16 %6, %15 offset:" #K0 "\n\tds_read_b64_tr_b16 %7, %15 offset:" #K1 "\n\t"             \
                 "ds_read_b64_tr_b16 %8, %14 offset:" #K2 "\n\tds_read_b64_tr_b16 %9, %14 offset:" #K3 "\n\t"             \
                 "ds_read_b64_tr_b16 %10, %15 offset:" #K2 "\n\tds_read_b64_tr_b16 %11, %15 offset:" #K3 "\n\t"           \
                 "s_waitcnt lgkmcnt(0)\n\ts_nop 1"                                                                        \
                 : "=&v"(al[0]), "=&v"(au[0]), "=&v"(al[1]), "=&v"(au[1]), "=&v"(sl[0]), "=&v"(su[0]), "=&v"(sl[1]), "=&v"(su[1]),   \
                   "=&v"(sl[2]), "=&v"(su[2]), "=&v"(sl[3]), "=&v"(su[3])                                                 \
                 : "v"(aA0), "v"(aA1), "v"(aS0), "v"(aS1)                                                                 \
                 : "memory")
#define NLAM_TR_STEP_A(K0, K1)                                                                                            \
    asm volatile("ds_read_b64_tr_b16 %0, %4 offset:" #K0 "\n\tds_read_b64_tr_b16 %1, %4 offset:" #K1 "\n\t"               \
                 "ds_read_b64_tr_b16 %2, %5 offset:" #K0 "\n\tds_read_b64_tr_b16 %3, %5 offset:" #K1 "\n\t"               \
                 "s_waitcnt lgkmcnt(0)\n\ts_nop 1"                                                                        \
                 : "=&v"(al[0]), "=&v"(au[0]), "=&v"(al[1]), "=&v"(au[1])                                                 \
                 : "v"(aA0), "v"(aA1)                                                                                     \
                 : "memory")

template <int NS, bool ABF, bool SBF, bool SILU, int R_, int NBUF_>
__global__ __launch_bounds__(512) void wgrad_ldma_kernel(const nlam_wgrad_t p) {
    using CF = WgLdma<ABF, SBF, SILU, R_, NBUF_>;
    constexpr int R = CF::R, NBUF = CF::NBUF;
    static_assert(!SBF || ABF, "a bf16 S operand comes with a bf16 A operand (dW2 of a layer with bf16 storage)");
    // NS = 3 (fp32-class): fp32 operands, every fragment split into three bf16 terms by the wave that reads it (6 MFMAs per block
    // pair, the term order of mma_frags: bit-identical to wgrad_wbf_body, whose 16-row K steps and row slices these are)
    static_assert(NS == 1 || (NS == 3 && !ABF && !SBF && R_ == 16), "three terms: fp32 operands, one K step per stage");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* lds = reinterpret_cast<char*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned bx = blockIdx.x, gx = gridDim.x, by = blockIdx.y;

    // output window (the enumeration of wgrad_wbf_body / wgrad_wide_kernel)
    constexpr int WIN = 256;
    const int mwins = (p.m + WIN - 1) / WIN;
    const int mw = by % mwins;
    int nwi = by / mwins;
    int s_sel = 0, off = 0;
    for (int s = 0; s < p.nsrc; ++s) {
        const int w = get_src(p, s).width;
        const int nws = (w + WIN - 1) / WIN;
        if (nwi < nws) {
            s_sel = s;
            break;
        }
        nwi -= nws;
        off += w;
    }
    const nlam_src_t S = get_src(p, s_sel);
    const int m0 = mw * WIN, mcols = min(WIN, p.m - m0);
    const int n0 = nwi * WIN, ncols = min(WIN, S.width - n0);
    const int gcol0 = off + n0;

    const int spb = (p.rows + R - 1) / R;                  // stages per batch item
    const int nst = spb * p.batch;                         // (a launch has far fewer than 2^31 stages)
    // this workgroup's stages are bx, bx + gx, ..: a cursor (batch item, stage inside it) advanced by gx -- the 64-bit division
    // `stage / spb` was ~300 scalar instructions per request
    struct StageCur {
        int b, s;
    };
    auto advance = [&](StageCur& c) {
        c.s += (int)gx;
        while (c.s >= spb) {
            c.s -= spb;
            ++c.b;
        }
    };

    // ---- LDS-DMA: lane -> (row of the piece, first column); everything that does not depend on the stage is computed once ----
    // bf16 tile: piece = [8 rows][64 columns]: lane -> row l / 8, LDS slot l % 8, which holds source slot (l % 8) ^ 4 for rows 2, 3, 6, 7
    // fp32 tile: piece = one row of 256 columns: lane -> columns 4 l ..
    const int br = lane >> 3;
    const int bslot = (lane & 7) ^ (((br >> 1) & 1) << 2);
    int a_row[CF::A_IPW], a_col[CF::A_IPW], s_row[CF::S_IPW], s_col[CF::S_IPW];   // row inside the stage, column inside the window (-1: past its end)
#pragma unroll
    for (int q = 0; q < CF::A_IPW; ++q) {
        const int pi = wave * CF::A_IPW + q;
        a_row[q] = ABF ? 8 * (pi >> 2) + br : pi;
        const int c = ABF ? 64 * (pi & 3) + 8 * bslot : 4 * lane;
        a_col[q] = c < mcols ? c : -1;
    }
#pragma unroll
    for (int q = 0; q < CF::S_IPW; ++q) {
        const int pi = wave * CF::S_IPW + q;
        s_row[q] = SBF ? 8 * (pi >> 2) + br : pi;
        const int c = SBF ? 64 * (pi & 3) + 8 * bslot : 4 * lane;
        s_col[q] = c < ncols ? c : -1;
    }
    // gather indices of an fp32 S tile: one row per instruction, so the index is wave-uniform (a scalar load), fetched one stage
    // ahead of the request that uses it
    long rid[CF::S_IPW];
    auto load_rid = [&](const StageCur& c) {
        if constexpr (!SBF) {
            const bool live = c.b < p.batch;
            const int r0 = live ? c.s * R : 0;
#pragma unroll
            for (int q = 0; q < CF::S_IPW; ++q) {
                const int row = r0 + (wave * CF::S_IPW + q);                       // uniform
                rid[q] = row;
                if (live && row < p.rows && S.idx != nullptr) rid[q] = S.idx[row];   // uniform branch, scalar load
            }
        }
    };
    auto issue = [&](const StageCur& c, int buf) {
        const bool live = c.b < p.batch;
        const int b = live ? c.b : 0;
        const int r0 = live ? c.s * R : 0;
        char* base = lds + (size_t)buf * CF::STAGE;
#pragma unroll
        for (int q = 0; q < CF::A_IPW; ++q) {
            const int row = r0 + a_row[q];
            const bool ok = live && row < p.rows && a_col[q] >= 0;
            const size_t e = ((size_t)b * p.rows + row) * p.m + m0 + a_col[q];
            const void* src = ABF ? static_cast<const void*>(reinterpret_cast<const bf16s_t*>(p.A) + e) : static_cast<const void*>(p.A + e);
            src = ok ? src : static_cast<const void*>(g_zero16);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(base + (size_t)(wave * CF::A_IPW + q) * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < CF::S_IPW; ++q) {
            const int row = r0 + s_row[q];
            const bool ok = live && row < p.rows && s_col[q] >= 0;
            const void* src;
            if constexpr (SBF) {   // never gathered (the launcher checks): z1 of this very launch's rows
                src = reinterpret_cast<const bf16s_t*>(S.ptr) + ((long)b * S.bstride + (long)row * S.width + n0 + s_col[q]);
            } else {
                src = S.ptr + ((long)b * S.bstride + rid[q] * S.width + n0 + s_col[q]);
            }
            src = ok ? src : static_cast<const void*>(g_zero16);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(base + CF::A_TILE + (size_t)(wave * CF::S_IPW + q) * 1024), 16, 0, 0);
        }
    };

    // ---- fragment reads ----
    // bf16 tile, transpose read: lane (g = l / 16, i = l % 16) supplies the address of row i / 4 (of the 4 rows 8 kg .. + 3, kg = g / 2),
    // columns 16 (g % 2) + 4 (i % 4) .. + 3 of the block, and receives column 16 (g % 2) + i = l % 32 of those four rows
    const int tg = lane >> 4, ti = lane & 15;
    const int tr_r = ti >> 2;
    const int tr_lo = 2 * (tg & 1) + ((ti & 3) >> 1);                       // slot inside the block's 64-byte half
    const int tr_base = (tg >> 1) * 4096 + tr_r * 128 + (ti & 1) * 8;       // row group kg, row, 8-byte half of the slot
    const int tr_off0 = tr_base + ((tr_lo | ((0 ^ ((tr_r >> 1) & 1)) << 2)) << 4);   // even block of a 64-column piece
    const int tr_off1 = tr_base + ((tr_lo | ((1 ^ ((tr_r >> 1) & 1)) << 2)) << 4);   // odd block
    const int wm = wave >> 1, wn = wave & 1;
    // LDS byte addresses for the asm reads (the dynamic segment's own address: 0 in a kernel without static __shared__)
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)lds;
    const unsigned ldsA0 = lds0 + (unsigned)(wm * 1024 + tr_off0), ldsA1 = lds0 + (unsigned)(wm * 1024 + tr_off1);   // blocks 2 wm, 2 wm + 1
    const unsigned ldsS0 = lds0 + (unsigned)(CF::A_TILE + wn * 2048 + tr_off0), ldsS1 = lds0 + (unsigned)(CF::A_TILE + wn * 2048 + tr_off1);
    const int fc = lane & 31, fkg = lane >> 5;
    auto frag_f32n = [&](const char* tile, int ks, int blk) -> BfFrag<NS> {
        const float* q = reinterpret_cast<const float*>(tile) + (size_t)(16 * ks + 8 * fkg) * 256 + 32 * blk + fc;
        float x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = q[k * 256];
        return split8<NS>(x);
    };
    auto frag_f32 = [&](const char* tile, int ks, int blk) -> u32x4 { return frag_f32n(tile, ks, blk).t[0]; };
    auto join = [](u32x2_t lo, u32x2_t up) -> u32x4 { return u32x4{lo[0], lo[1], up[0], up[1]}; };

    f32x16 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
    auto mma = [&](const u32x4 (&a)[2], const u32x4 (&bq)[4]) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int w2 = 0; w2 < 4; ++w2) acc[u][w2] = MFMA_BF16(a[u], bq[w2], acc[u][w2]);
    };

    StageCur cur = {0, (int)bx};        // the stage the next request is for (its gather indices: one stage further)
    while (cur.s >= spb) {
        cur.s -= spb;
        ++cur.b;
    }
    // dW2 = dz2^T silu(z1): SiLU once per element, in place in the S tile of a landed stage (layout-agnostic)
    auto silu_pass = [&](int b_) {
        char* Sq = lds + (size_t)b_ * CF::STAGE + CF::A_TILE;
#pragma unroll
        for (int k = 0; k < CF::S_TILE / (16 * 512); ++k) {
            u32x4* q = reinterpret_cast<u32x4*>(Sq) + tid + 512 * k;
            const u32x4 v = *q;
            u32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned vc = v[c];   // (element copy first: __builtin_bit_cast on a vector-element lvalue reads element 0 with this clang)
                if constexpr (SBF) {
                    unsigned w[1];
                    split_pair<1>(silu_f(__builtin_bit_cast(float, vc << 16)), silu_f(__builtin_bit_cast(float, vc & 0xffff0000u)), w);
                    o[c] = w[0];
                } else {
                    o[c] = __builtin_bit_cast(unsigned, silu_f(__builtin_bit_cast(float, vc)));
                }
            }
            *q = o;
        }
    };
    // prologue: NBUF - 1 stages requested; with SiLU the first one is also transformed before the loop
#pragma unroll
    for (int k = 0; k < NBUF - 1; ++k) {
        load_rid(cur);
        issue(cur, k);
        advance(cur);
    }
    load_rid(cur);
    if constexpr (SILU) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * CF::IPS) : "memory");
        asm volatile("s_barrier" ::: "memory");
        silu_pass(0);
    }
    const int nmine = (int)bx < nst ? (nst - (int)bx + (int)gx - 1) / (int)gx : 0;
    int buf = 0;
    for (int it = 0; it < nmine; ++it) {
        // without SiLU: this wave's pieces of stage `it` have landed (one more stage stays in flight); with SiLU: those of stage
        // it + 1 (stage `it` landed an iteration ago and was transformed then) ...
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CF::IPS) : "memory");
        // ... and so have everybody's; every wave is done with the buffer the next request goes to (and, with SiLU, with its
        // share of the transformation of stage `it`: the LDS stores are waited for in front of the barrier)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        issue(cur, buf == 0 ? NBUF - 1 : buf - 1);
        advance(cur);
        load_rid(cur);
        char* At = lds + (size_t)buf * CF::STAGE;
        char* St = At + CF::A_TILE;
        if constexpr (SILU) silu_pass(buf == NBUF - 1 ? 0 : buf + 1);   // the NEXT stage, beside this stage's products
        if constexpr (ABF) {
            const unsigned bo = (unsigned)buf * CF::STAGE;
            const unsigned aA0 = ldsA0 + bo, aA1 = ldsA1 + bo;
            u32x2_t al[2], au[2];
            if constexpr (SBF) {
                const unsigned aS0 = ldsS0 + bo, aS1 = ldsS1 + bo;
                u32x2_t sl[4], su[4];
                {
                    NLAM_TR_STEP_AS(0, 512, 1024, 1536);
                    const u32x4 a[2] = {join(al[0], au[0]), join(al[1], au[1])};
                    const u32x4 bq[4] = {join(sl[0], su[0]), join(sl[1], su[1]), join(sl[2], su[2]), join(sl[3], su[3])};
                    mma(a, bq);
                }
                if constexpr (R == 32) {
                    NLAM_TR_STEP_AS(8192, 8704, 9216, 9728);
                    const u32x4 a[2] = {join(al[0], au[0]), join(al[1], au[1])};
                    const u32x4 bq[4] = {join(sl[0], su[0]), join(sl[1], su[1]), join(sl[2], su[2]), join(sl[3], su[3])};
                    mma(a, bq);
                }
            } else {
                {
                    u32x4 bq[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) bq[u] = frag_f32(St, 0, 4 * wn + u);
                    NLAM_TR_STEP_A(0, 512);
                    const u32x4 a[2] = {join(al[0], au[0]), join(al[1], au[1])};
                    mma(a, bq);
                }
                if constexpr (R == 32) {
                    u32x4 bq[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) bq[u] = frag_f32(St, 1, 4 * wn + u);
                    NLAM_TR_STEP_A(8192, 8704);
                    const u32x4 a[2] = {join(al[0], au[0]), join(al[1], au[1])};
                    mma(a, bq);
                }
            }
        } else if constexpr (NS == 1) {
#pragma unroll
            for (int ks = 0; ks < R / 16; ++ks) {
                u32x4 a[2], bq[4];
#pragma unroll
                for (int u = 0; u < 2; ++u) a[u] = frag_f32(At, ks, 2 * wm + u);
#pragma unroll
                for (int u = 0; u < 4; ++u) bq[u] = frag_f32(St, ks, 4 * wn + u);
                mma(a, bq);
            }
        } else {
            BfFrag<NS> a[2], bq[4];
#pragma unroll
            for (int u = 0; u < 2; ++u) a[u] = frag_f32n(At, 0, 2 * wm + u);
#pragma unroll
            for (int u = 0; u < 4; ++u) bq[u] = frag_f32n(St, 0, 4 * wn + u);
#pragma unroll
            for (int ord = NS - 1; ord >= 0; --ord)
#pragma unroll
                for (int pa = 0; pa <= ord; ++pa)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int w2 = 0; w2 < 4; ++w2) acc[u][w2] = MFMA_BF16(a[u].t[pa], bq[w2].t[ord - pa], acc[u][w2]);
        }
        buf = buf == NBUF - 1 ? 0 : buf + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the run-ahead stages (zero sources past the end) before the wave leaves

    float* P = p.partials + (size_t)bx * p.m * p.n;
    const int i = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w2 = 0; w2 < 4; ++w2) {
            const int nl = (4 * wn + w2) * 32 + i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = (2 * wm + u) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (ml < mcols && nl < ncols) P[(size_t)(m0 + ml) * p.n + gcol0 + nl] = acc[u][w2][r];
            }
        }
}

int wgrad_wbf_ns(const nlam_wgrad_t* p) {
    int ns = (int)((p->flags & NLAM_F_MM_MASK) >> NLAM_F_MM_SHIFT);
    if (ns == 0) return 0;
    return ns == 2 ? 3 : ns;
}

// ---------------------------------------------------------------------------
// backward of the fused MLP on the split-bf16 cores (data gradients; saved-tensor and
// output conventions of mlp_bwd_wide_kernel)
// ---------------------------------------------------------------------------
// A workgroup owns NRT = RG * RT row tiles at a time; wave (rg, fg) owns feature blocks
// fg, fg + FG, .. of row tiles rg*RT .. rg*RT + RT - 1 in every stage:
//   A  dmsg -> LayerNorm backward (row statistics across the FG waves) -> dz2: stored for
//      the weight gradient, split and published as B fragments (accumulator layout =
//      slot-permuted K order, as in the forward);
//   B  dh = W2^T dz2, dz1 = dh * silu'(z1): stored, split, published over the dz2 fragments;
//   C  dx_s = W1_s^T dz1 for every source with a data gradient, then the residual terms and
//      the three output modes.
// Column sums (db1, db2, dgamma, dbeta) stay inside the owning wave: a [32][36] staging
// block per wave turns its 32 x 32 register block into per-column sums (lane = column).
// The transposed weights stream from L2 pre-split (pack_bf_kernel), one K group ahead.
// K groups of a backward GEMM over `blocks` 32-feature blocks, padded to a multiple of the A-ring depth of the term count
__host__ __device__ inline int wbf_bwd_tk(int blocks, int ns) {
    const int d = ns == 1 ? 4 : 2;
    return (2 * blocks + d - 1) / d * d;
}

template <int NS, int NW, int FG, int FB, int RT, bool SBF = false, bool V4 = false>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void mlp_bwd_wbf_kernel(const nlam_mlp_bwd_t p) {
    static_assert(!SBF || NS == 1, "bf16 storage belongs to the one-term (autocast) kernels");
    constexpr bool sbf = SBF;   // NLAM_F_STORE_BF16: z1 / xhat are read and dz1 / dz2 written as bf16 rows
    constexpr int RG = NW / FG, NRT = RG * RT;
    static_assert(FB * RT >= 2, "two accumulators must alternate (see mma_split_lds)");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rg = wave / FG, fg = wave % FG;
    const int j = lane & 31, hi = lane >> 5;

    const int HBT = (p.hid + 31) >> 5, OBT = (p.dout + 31) >> 5;
    // K groups of W2^T / W1_s^T, padded to whole ring revolutions (the packed matrices hold zero groups there, the B fragments
    // whatever finite dz2 / dz1 fragments the region held before: the fragment region is zeroed once, below)
    const int TKA = wbf_bwd_tk(OBT, NS), TKB = wbf_bwd_tk(HBT, NS);
    const int TKM = TKA > TKB ? TKA : TKB;

    // A stream: phase 0 = W2^T (HBT blocks x TKA groups), then one phase (TKB groups) per source with a data gradient.
    // Scalars, not arrays: a run-time index into a register array would send it to scratch.
    const u32x4* A0 = reinterpret_cast<const u32x4*>(p.wpack);
    const u32x4 *A1 = A0, *A2 = A0, *A3 = A0;
    int nb1 = 1, nb2 = 1, nb3 = 1, nact = 0;
    bool act[NLAM_MAX_SRC];
    {
        size_t off = (size_t)HBT * TKA * NS * 64;
#pragma unroll
        for (int s = 0; s < NLAM_MAX_SRC; ++s) {
            // NLAM_F_PRE_ADD: only source 0 has columns in W1; the gradient of an addend source is dz1 itself (stage B)
            act[s] = s < p.nsrc && p.dmode[s] != 0 && (s == 0 || (p.flags & NLAM_F_PRE_ADD) == 0);
            if (act[s]) {
                const int SB = (p.src[s].width + 31) >> 5;
                if (nact == 0) {
                    A1 = A0 + off;
                    nb1 = SB;
                } else if (nact == 1) {
                    A2 = A0 + off;
                    nb2 = SB;
                } else {
                    A3 = A0 + off;
                    nb3 = SB;
                }
                off += (size_t)SB * TKB * NS * 64;
                ++nact;
            }
        }
    }
    // Per phase, the wave's FB block bases (uniform pointers; see the forward kernel): phase 0 = W2^T, then one phase per source
    // with a data gradient, in source order.  nxt*[..] = the phase that follows (the next active source, or W2^T of the next
    // super tile), so that the last D groups of a phase prefetch the head of the next one.
    constexpr int D = WbfRing<NS, FB>::D;
    const u32x4* pb0[FB];
    const u32x4 *pbs0[FB], *pbs1[FB], *pbs2[FB];       // by SOURCE index (valid where act[s])
    const u32x4 *nx0[FB], *nxs0[FB], *nxs1[FB], *nxs2[FB];
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
        const int blk = fg + fb * FG;
        pb0[fb] = A0 + (size_t)min(blk, HBT - 1) * TKA * NS * 64;
        const u32x4* ph1 = A1 + (size_t)min(blk, nb1 - 1) * TKB * NS * 64;   // phases by ORDER (1st, 2nd, 3rd active source)
        const u32x4* ph2 = A2 + (size_t)min(blk, nb2 - 1) * TKB * NS * 64;
        const u32x4* ph3 = A3 + (size_t)min(blk, nb3 - 1) * TKB * NS * 64;
        // order of source s among the active ones
        const int o0 = 0, o1 = act[0] ? 1 : 0, o2 = o1 + (act[1] ? 1 : 0);
        auto by_order = [&](int o) { return o == 0 ? ph1 : (o == 1 ? ph2 : ph3); };
        pbs0[fb] = by_order(o0);
        pbs1[fb] = by_order(o1);
        pbs2[fb] = by_order(o2);
        auto after = [&](int o) { return o + 1 < nact ? by_order(o + 1) : pb0[fb]; };   // phase behind the o-th active source
        nx0[fb] = nact > 0 ? ph1 : pb0[fb];
        nxs0[fb] = after(o0);
        nxs1[fb] = after(o1);
        nxs2[fb] = after(o2);
    }
    // LDS map
    u32x4* Zf = reinterpret_cast<u32x4*>(smem);                               // [NRT][TKM][NS][64]: dz2, later dz1 fragments
    float* stg_all = reinterpret_cast<float*>(Zf + (size_t)NRT * TKM * NS * 64);   // NW x [32][36]
    float* stg = stg_all + wave * (32 * kStgStride);
    float* red = stg_all + NW * (32 * kStgStride);                            // 2 x FG x NRT*32
    float* gvec = red + 2 * FG * NRT * 32;                                    // gamma, zero padded to whole blocks
    for (int c = tid; c < OBT * 32; c += NW * 64) gvec[c] = (p.ln_w != nullptr && c < p.dout) ? p.ln_w[c] : 0.f;
    for (int c = tid; c < NRT * TKM * NS * 64; c += NW * 64) Zf[c] = u32x4{0u, 0u, 0u, 0u};   // padded K groups: finite from the start
    __syncthreads();

    const bool has_ln = p.ln_w != nullptr;
    const float inv_dout = 1.f / (float)p.dout;

    // column sums of the wave's block(s): lane & 31 = column
    float acc_db1[FB], acc_db2[FB], acc_dg[FB], acc_dbt[FB];
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) acc_db1[fb] = acc_db2[fb] = acc_dg[fb] = acc_dbt[fb] = 0.f;
    // v = this lane's 16 values (chunk layout) of a 32 x 32 block, row = j: add the block's column sums to acc
    auto colsum_add = [&](const f32x16& v, float& acc) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) *reinterpret_cast<f32x4*>(&stg[j * kStgStride + 8 * tt + 4 * hi]) = acc_chunk(v, tt);
        wave_lds_sync();
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += stg[(16 * hi + q) * kStgStride + j];
        wave_lds_sync();
        acc += s + __shfl_xor(s, 32, 64);
    };
    // publish a block's values as the B fragments of K groups 2*blk, 2*blk + 1 of row tile rtl
    auto publish = [&](const f32x16& v, int rtl, int TK, int blk) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = v[8 * h + q];
            const BfFrag<NS> f = split8<NS>(x);
#pragma unroll
            for (int pa = 0; pa < NS; ++pa) Zf[(((size_t)rtl * TK + 2 * blk + h) * NS + pa) * 64 + lane] = f.t[pa];
        }
    };
    AFrag<NS, FB> ring[D];
    // one GEMM phase: TK groups of the matrix at cur[], the ring refilled D groups ahead -- behind the phase's last groups with
    // the head of the matrix at nxt[] (TK of every phase is a multiple of D)
    auto gemm = [&](f32x16(&acc)[FB][RT], const u32x4* const (&cur)[FB], const u32x4* const (&nxt)[FB], int TK) {
#pragma unroll
        for (int fb = 0; fb < FB; ++fb)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[fb][rt][r] = 0.f;
        for (int kg = 0; kg < TK; kg += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                u32x4 bq[NS][RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int pa = 0; pa < NS; ++pa) bq[pa][rt] = Zf[(((size_t)(rg * RT + rt) * TK + kg + u) * NS + pa) * 64 + lane];
                mma_frags<NS, FB, RT>(acc, ring[u], bq);
                const int g = kg + u + D;
                const bool wrap = g >= TK;
                const u32x4* nb[FB];
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) nb[fb] = wrap ? nxt[fb] : cur[fb];
                load_aring<NS, FB>(ring[u], nb, wrap ? g - TK : g, lane);
            }
        }
    };

#pragma unroll
    for (int u = 0; u < D; ++u) load_aring<NS, FB>(ring[u], pb0, u, lane);
    NLAM_T_DECL
    int t_ntiles_ = 0;

    const int spb = (p.ntiles + NRT - 1) / NRT;
    const long nsuper = (long)spb * p.batch;
    for (long st = xcd_slot((int)blockIdx.x, (int)gridDim.x); st < nsuper; st += gridDim.x) {
        const int b = (int)(st / spb);
        const int t0 = (int)(st % spb) * NRT;

        TileInfo tl[RT];
        bool valid[RT];
        int prow[RT];
        size_t srow_id[RT];
        const float* grow[RT];
        const float* garow[RT];
        float gscale[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int ti = t0 + rg * RT + rt;
            if (ti < p.ntiles) {
                tl[rt] = get_tile(p.tiles, ti, p.rows);
            } else {
                tl[rt].row0 = 0;
                tl[rt].nrows = 0;
                tl[rt].seg0 = 0;
                tl[rt].nseg = 0;
                tl[rt].split = false;
            }
            valid[rt] = j < tl[rt].nrows;
            prow[rt] = tl[rt].row0 + j;
            srow_id[rt] = (size_t)b * p.rows + prow[rt];
            grow[rt] = nullptr;
            garow[rt] = nullptr;
            gscale[rt] = 1.f;
            if (p.g_out != nullptr && valid[rt]) {
                const long oidx = p.out_idx != nullptr ? p.out_idx[prow[rt]] : prow[rt];
                grow[rt] = p.g_out + (long)b * p.out_bstride + oidx * (long)p.dout;
            }
            if (p.g_aggr != nullptr && valid[rt]) {
                const int sg = p.seg_of_row[prow[rt]];
                garow[rt] = p.g_aggr + ((size_t)b * p.nseg_total + sg) * p.dout;
                if (p.flags & NLAM_F_MEAN) gscale[rt] = p.inv_deg[sg];
            }
        }
        auto dmsg_chunk = [&](int rt, int t) {
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (grow[rt] != nullptr) g += load_chunk_v<V4>(grow[rt], p.dout, t, hi, true);
            if (garow[rt] != nullptr) g += load_chunk_v<V4>(garow[rt], p.dout, t, hi, true) * gscale[rt];
            return g;
        };

        ++t_ntiles_;
        NLAM_T_MARK(0)
        // ---- stage A: dmsg, LayerNorm backward, dz2 ----
        f32x16 dz[FB][RT];
        // every row this stage and the next need is requested before the first use: dmsg, xhat, rstd and (for stage
        // B, behind GEMM dh) the saved pre-activations z1
        f32x16 zv[FB][RT];
        u32x4 zraw[FB][RT][2];   // bf16 storage: the raw halves of the z1 rows, widened behind GEMM dh (8 registers instead of 16 across it)
        float rstd_r[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) rstd_r[rt] = (has_ln && valid[rt]) ? p.rstd[srow_id[rt]] : 0.f;
        if (has_ln) {
            f32x16 xh[FB][RT], g16[FB][RT];
            float m1[RT], m2[RT];
            // Requests first, arithmetic afterwards: every load_chunk is a (lane-predicated) branch, and the scheduler does not
            // move code across branches -- `g = load(g_out) + load(g_aggr) * scale` per chunk therefore waited for each chunk before
            // the next one was even requested: 32 serial round trips per super tile, 40 % of this kernel at one bf16 term.
            f32x16 ga16[FB][RT];
            u32x4 xraw[FB][RT][2];   // bf16 storage: the raw halves; widened behind the requests
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float* xrow = valid[rt] ? p.xhat + srow_id[rt] * p.dout : nullptr;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
                    if constexpr (sbf)
                        load_block_bf16_raw(reinterpret_cast<const bf16s_t*>(p.xhat) + srow_id[rt] * p.dout, 32 * blk, hi, valid[rt] && blk < OBT,
                                            xraw[fb][rt]);
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        const bool inb = blk < OBT;
                        const f32x4 g = load_chunk_v<V4>(grow[rt], p.dout, t, hi, inb && grow[rt] != nullptr);
                        const f32x4 a = load_chunk_v<V4>(garow[rt], p.dout, t, hi, inb && garow[rt] != nullptr);
                        f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
                        if constexpr (!sbf) x4 = load_chunk_v<V4>(xrow, p.dout, t, hi, inb && valid[rt]);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            g16[fb][rt][4 * tt + c] = g[c];
                            ga16[fb][rt][4 * tt + c] = a[c];
                            xh[fb][rt][4 * tt + c] = x4[c];
                        }
                    }
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float* zrow = valid[rt] ? p.z1 + srow_id[rt] * p.hid : nullptr;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    if constexpr (sbf) {
                        load_block_bf16_raw(reinterpret_cast<const bf16s_t*>(p.z1) + srow_id[rt] * p.hid, 32 * (fg + fb * FG), hi,
                                            valid[rt] && fg + fb * FG < HBT, zraw[fb][rt]);
                    } else {
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) {
                            const f32x4 z = load_chunk_v<V4>(zrow, p.hid, (fg + fb * FG) * 4 + tt, hi, valid[rt] && fg + fb * FG < HBT);
#pragma unroll
                            for (int c = 0; c < 4; ++c) zv[fb][rt][4 * tt + c] = z[c];
                        }
                    }
                }
            }
            if constexpr (sbf) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int fb = 0; fb < FB; ++fb) xh[fb][rt] = block_from_bf16_raw(xraw[fb][rt]);
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)   // dmsg = g_out + g_aggr * scale, in that order (as dmsg_chunk)
#pragma unroll
                for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) g16[fb][rt][r] = g16[fb][rt][r] + ga16[fb][rt][r] * gscale[rt];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                m1[rt] = m2[rt] = 0.f;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const f32x4 gm = *reinterpret_cast<const f32x4*>(&gvec[(blk < OBT ? 8 * (blk * 4 + tt) : 0) + 4 * hi]);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float gy = g16[fb][rt][4 * tt + c] * gm[c];
                            dz[fb][rt][4 * tt + c] = gy;
                            m1[rt] += gy;
                            m2[rt] += gy * xh[fb][rt][4 * tt + c];
                        }
                    }
                }
                m1[rt] = row_allreduce(m1[rt]);
                m2[rt] = row_allreduce(m2[rt]);
                if (hi == 0) {
                    red[(fg * NRT + rg * RT + rt) * 32 + j] = m1[rt];
                    red[((FG + fg) * NRT + rg * RT + rt) * 32 + j] = m2[rt];
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    f32x16 gx16;
#pragma unroll
                    for (int r = 0; r < 16; ++r) gx16[r] = g16[fb][rt][r] * xh[fb][rt][r];
                    colsum_add(g16[fb][rt], acc_dbt[fb]);
                    colsum_add(gx16, acc_dg[fb]);
                }
            NLAM_T_MARK(1)
            __syncthreads();
            NLAM_T_MARK(8)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float rstd = rstd_r[rt];
                float t1 = 0.f, t2 = 0.f;
#pragma unroll
                for (int w = 0; w < FG; ++w) {
                    t1 += red[(w * NRT + rg * RT + rt) * 32 + j];
                    t2 += red[((FG + w) * NRT + rg * RT + rt) * 32 + j];
                }
                t1 *= inv_dout;
                t2 *= inv_dout;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int col = 32 * blk + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        const float v = rstd * (dz[fb][rt][r] - t1 - xh[fb][rt][r] * t2);
                        dz[fb][rt][r] = (valid[rt] && col < p.dout) ? v : 0.f;
                    }
                }
            }
        } else {
            f32x16 ga16[FB][RT];   // requests first, see above
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float* zrow = valid[rt] ? p.z1 + srow_id[rt] * p.hid : nullptr;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
                    if constexpr (sbf)
                        load_block_bf16_raw(reinterpret_cast<const bf16s_t*>(p.z1) + srow_id[rt] * p.hid, 32 * blk, hi, valid[rt] && blk < HBT,
                                            zraw[fb][rt]);
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const f32x4 g = load_chunk_v<V4>(grow[rt], p.dout, blk * 4 + tt, hi, blk < OBT && grow[rt] != nullptr);
                        const f32x4 a = load_chunk_v<V4>(garow[rt], p.dout, blk * 4 + tt, hi, blk < OBT && garow[rt] != nullptr);
                        f32x4 z = {0.f, 0.f, 0.f, 0.f};
                        if constexpr (!sbf) z = load_chunk_v<V4>(zrow, p.hid, blk * 4 + tt, hi, valid[rt] && blk < HBT);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            dz[fb][rt][4 * tt + c] = g[c];
                            ga16[fb][rt][4 * tt + c] = a[c];
                            zv[fb][rt][4 * tt + c] = z[c];
                        }
                    }
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) dz[fb][rt][r] = dz[fb][rt][r] + ga16[fb][rt][r] * gscale[rt];
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float* drow = p.dz2 != nullptr ? p.dz2 + srow_id[rt] * (size_t)(p.dz2_ld > 0 ? p.dz2_ld : p.dout) : nullptr;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
                if (blk < OBT) {
                    if (drow != nullptr) {
                        if constexpr (sbf) {
                            store_block_bf16(reinterpret_cast<bf16s_t*>(p.dz2) + srow_id[rt] * p.dout, 32 * blk, hi, valid[rt], dz[fb][rt]);
                        } else {
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) store_chunk_v<V4>(drow, p.dout, blk * 4 + tt, hi, valid[rt], acc_chunk(dz[fb][rt], tt));
                        }
                    }
                    colsum_add(dz[fb][rt], acc_db2[fb]);
                    publish(dz[fb][rt], rg * RT + rt, TKA, blk);
                }
            }
        }
        __syncthreads();
        NLAM_T_MARK(2)

        // ---- stage B: dh = W2^T dz2 ; dz1 = dh * silu'(z1) ----
        gemm(dz, pb0, nx0, TKA);
        NLAM_T_MARK(3)
        __syncthreads();   // every wave is done with the dz2 fragments
        if constexpr (sbf) {   // the bf16 z1 rows requested in stage A, widened here
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) zv[fb][rt] = block_from_bf16_raw(zraw[fb][rt]);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float* drow = p.dz1 != nullptr ? p.dz1 + srow_id[rt] * p.hid : nullptr;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
                if (blk < HBT) {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const int t = blk * 4 + tt;
                        f32x4 v;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            v[c] = valid[rt] ? dz[fb][rt][4 * tt + c] * silu_grad_f(zv[fb][rt][4 * tt + c]) : 0.f;
                            dz[fb][rt][4 * tt + c] = v[c];
                        }
                        if constexpr (!sbf) {
                            if (drow != nullptr) store_chunk_v<V4>(drow, p.hid, t, hi, valid[rt], v);
                        }
                    }
                    if constexpr (sbf) {
                        if (drow != nullptr) store_block_bf16(reinterpret_cast<bf16s_t*>(p.dz1) + srow_id[rt] * p.hid, 32 * blk, hi, valid[rt], dz[fb][rt]);
                    }
                    colsum_add(dz[fb][rt], acc_db1[fb]);
                    if (p.flags & NLAM_F_PRE_ADD) {
                        // gradient of a receiver-gathered addend: dz1 summed over each receiver's rows (whole receivers per tile)
#pragma unroll
                        for (int s = 1; s < NLAM_MAX_SRC; ++s) {
                            if (s < p.nsrc && p.dmode[s] == 3 && tl[rt].nseg > 0) {   // a tile of isolated receivers (no rows) still owns their zeros
                                int raw_ptr = 0;
                                if (!tl[rt].split && lane <= tl[rt].nseg) raw_ptr = p.rowptr[tl[rt].seg0 + lane];
#pragma unroll
                                for (int tt = 0; tt < 4; ++tt)
                                    *reinterpret_cast<f32x4*>(&stg[j * kStgStride + 8 * tt + 4 * hi]) = acc_chunk(dz[fb][rt], tt);
                                wave_lds_sync();
                                block_segment_reduce(stg, tl[rt], raw_ptr, 1.f, p.dsrc[s] + (long)b * p.dsrc_bstride[s] + 32 * blk, p.hid,
                                                     min(32, p.hid - 32 * blk), lane);
                                wave_lds_sync();
                            }
                        }
                    }
                    publish(dz[fb][rt], rg * RT + rt, TKB, blk);
                }
            }
        }
        __syncthreads();
        NLAM_T_MARK(4)

        // ---- stage C: dx_s = W1_s^T dz1 per source ----
#pragma unroll
        for (int s = 0; s < NLAM_MAX_SRC; ++s) {
            if (!act[s]) continue;
            const nlam_src_t S = p.src[s];
            const int mode = p.dmode[s];
            float* dbase = p.dsrc[s];
            const long dbstride = p.dsrc_bstride[s];
            const int w = S.width;
            const int SB = (w + 31) >> 5;
            if (s == 0) gemm(dz, pbs0, nxs0, TKB);
            else if (s == 1) gemm(dz, pbs1, nxs1, TKB);
            else gemm(dz, pbs2, nxs2, TKB);
            NLAM_T_MARK(5)
            const bool add_gout = (s == 0) && (p.flags & NLAM_F_ADD_SRC0) && p.g_out != nullptr;
            const bool add_gmsg = (s == 1) && (p.flags & NLAM_F_ADD_SRC1);
            // NLAM_F_ACC_DSRC0: d src0 += (an earlier autoregressive step's gradient of the same tensor is already there); its rows
            // ride in the request slots of the aggregated-gradient residual, which source 0 never uses
            const bool acc0 = (s == 0) && mode == 1 && (p.flags & NLAM_F_ACC_DSRC0);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                float* drow = nullptr;
                if (valid[rt]) {
                    if (mode == 1) {
                        const long ridx = S.idx != nullptr ? S.idx[prow[rt]] : prow[rt];
                        drow = dbase + (long)b * dbstride + ridx * (long)w;
                    } else if (mode == 2) {
                        drow = dbase + srow_id[rt] * w;
                    }
                }
                int raw_ptr = 0;
                if (mode == 3 && !tl[rt].split && lane <= tl[rt].nseg) raw_ptr = p.rowptr[tl[rt].seg0 + lane];
                // the residual terms of the whole row are requested before its first store (a load behind a store
                // waits for the store's acknowledgement)
                f32x4 rs[FB][4], rs2[FB][4];   // g_out rows (either residual), aggregated-gradient rows (d src1 += dmsg): no arithmetic
                                               // between the requests
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        rs[fb][tt] = load_chunk_v<V4>(grow[rt], p.dout, blk * 4 + tt, hi, blk < SB && (add_gout || add_gmsg) && grow[rt] != nullptr);
                        rs2[fb][tt] = load_chunk_v<V4>(acc0 ? drow : garow[rt], acc0 ? w : p.dout, blk * 4 + tt, hi,
                                                       blk < SB && ((add_gmsg && garow[rt] != nullptr) || (acc0 && drow != nullptr)));
                    }
                }
#pragma unroll
                for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) rs[fb][tt] += rs2[fb][tt] * (acc0 ? 1.f : gscale[rt]);
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) {
                    const int blk = fg + fb * FG;
                    if (blk < SB) {
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) {
                            const int t = blk * 4 + tt;
                            f32x4 v = acc_chunk(dz[fb][rt], tt) + rs[fb][tt];
                            if (mode == 3) {
                                if (!valid[rt]) v = f32x4{0.f, 0.f, 0.f, 0.f};
                                *reinterpret_cast<f32x4*>(&stg[j * kStgStride + 8 * tt + 4 * hi]) = v;
                            } else {
                                store_chunk_v<V4>(drow, w, t, hi, valid[rt], v);
                            }
                        }
                        if (mode == 3) {
                            wave_lds_sync();
                            if (tl[rt].nseg > 0)   // also for a tile of isolated receivers (nrows == 0): their gradient rows are written as zeros
                                block_segment_reduce(stg, tl[rt], raw_ptr, 1.f, dbase + (long)b * dbstride + 32 * blk, w, min(32, w - 32 * blk), lane);
                            wave_lds_sync();
                        }
                    }
                }
            }
            NLAM_T_MARK(6)
        }
        __syncthreads();   // super tile end: the fragments and red are rewritten by the next one
        NLAM_T_MARK(9)
    }
    NLAM_T_DRAIN
    NLAM_T_MARK(7)
    NLAM_T_FLUSH(t_ntiles_)

    if (p.vec_partials != nullptr) {
        float* vp = p.vec_partials + ((size_t)blockIdx.x * RG + rg) * 4 * p.vec_stride;
#pragma unroll
        for (int fb = 0; fb < FB; ++fb) {
            const int c = 32 * (fg + fb * FG) + j;
            if (hi == 0 && c < p.vec_stride) {
                vp[0 * p.vec_stride + c] = acc_db1[fb];
                vp[1 * p.vec_stride + c] = acc_db2[fb];
                vp[2 * p.vec_stride + c] = acc_dg[fb];
                vp[3 * p.vec_stride + c] = acc_dbt[fb];
            }
        }
        for (int c = 32 * FG * FB + fg * 64 + lane; c < p.vec_stride; c += FG * 64) {
#pragma unroll
            for (int k = 0; k < 4; ++k) vp[k * p.vec_stride + c] = 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
// Round 6: the factorised edge layer's backward as a kernel of its own (mlp_bwd_edge_kernel)
// ---------------------------------------------------------------------------
// The counterpart of mlp_fwd_edge_kernel for the data-gradient launch of the same layer (gnn_layers.py:110-189 back-propagated):
// d = 512, one term (and d = 256, three terms: the fp32-class configuration).  mlp_bwd_wbf_kernel's shape for d = 512 is 8 waves x 2 feature blocks on ONE 32-row tile: every A
// fragment fetched from L2 feeds one MFMA (the vector memory path delivers 64 bytes per clock and CU: 16 clocks per 1-KiB
// fragment against 8 clocks of matrix pipe per MFMA and CU), and six workgroup barriers are paid per 32 rows (101k wave-cycles
// per 32 rows, GEMMs 23k of them: profiles/round6/phase_cycles_wide.txt).  Here a workgroup owns TWO row tiles:
//  * stage A runs row tile by row tile (the requests of a tile's g_out / aggregated-gradient / xhat rows need 80 registers), the
//    LayerNorm statistics of both tiles cross the waves behind one barrier;
//  * both GEMMs feed two MFMAs per A fragment; z1 and the residual rows are requested ahead of the GEMM in front of their use;
//  * row metadata (scatter / gather indices, mean scales, row pointers, descriptors) double buffered in LDS, fetched a tile ahead;
//  * shapes are template constants.
// Launch conditions: see bwd_edge_ok().  Outputs and saved-tensor conventions are those of mlp_bwd_wbf_kernel.
template <int NS_, int D_, bool SBF>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void mlp_bwd_edge_kernel(const nlam_mlp_bwd_t p) {
    constexpr int NS = NS_, NT = 512, FG = 8, RT = 2, NRT = 2;
    constexpr int HBT = D_ / 32, FB = HBT / FG, TK = D_ / 16;
    static_assert((D_ == 512 && NS == 1 && FB == 2) || (D_ == 256 && NS == 3 && FB == 1 && !SBF), "d = 512 one term, d = 256 three terms");
    constexpr int RD = 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int fg = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hi = lane >> 5;

    // LDS map
    u32x4* Zf = reinterpret_cast<u32x4*>(smem);                               // [NRT][TK][NS][64]: dz2, later dz1 fragments
    float* stg = reinterpret_cast<float*>(Zf + (size_t)NRT * TK * NS * 64) + (size_t)fg * 32 * kStgStride;   // 8 x [32][36]
    float* red = reinterpret_cast<float*>(Zf + (size_t)NRT * TK * NS * 64) + (size_t)FG * 32 * kStgStride;   // 2 x FG x NRT*32
    float* gvec = red + 2 * FG * NRT * 32;                                    // gamma
    int* meta0 = reinterpret_cast<int*>(gvec + D_);                           // 2 x { oidx[64] | seg[64] | sidx[64] | scale[64] | rps[2*33] | tds[2*4] }
    constexpr int kMeta = 4 * NRT * 32 + NRT * 33 + NRT * 4;
#pragma unroll 1
    for (int c = tid; c < D_; c += NT) gvec[c] = p.ln_w[c];
    const float inv_d = 1.f / (float)D_;

    const u32x4* A0 = reinterpret_cast<const u32x4*>(p.wpack);               // W2^T: HBT blocks x TK groups
    const u32x4* A1 = A0 + (size_t)HBT * TK * NS * 64;                       // W1_e^T: HBT blocks x TK groups
    const u32x4 *pb0[FB], *pb1[FB];
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) {
        pb0[fb] = A0 + (size_t)(fg + fb * FG) * TK * NS * 64;
        pb1[fb] = A1 + (size_t)(fg + fb * FG) * TK * NS * 64;
    }
    const bool want0 = p.dmode[0] == 1;                                      // gradient of the edge rows wanted
    const bool want2 = p.nsrc > 2 && p.dmode[2] == 3;                        // gradient of the receiver-gathered addend wanted
    const u32x4* pn0[FB];                                                     // what follows W2^T in the weight stream (W1_e^T exists in the image
#pragma unroll                                                                //  only when the edge gradient is wanted)
    for (int fb = 0; fb < FB; ++fb) pn0[fb] = want0 ? pb1[fb] : pb0[fb];

    float acc_db1[FB], acc_db2[FB], acc_dg[FB], acc_dbt[FB];
#pragma unroll
    for (int fb = 0; fb < FB; ++fb) acc_db1[fb] = acc_db2[fb] = acc_dg[fb] = acc_dbt[fb] = 0.f;
    auto colsum_add = [&](const f32x16& v, float& acc) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) *reinterpret_cast<f32x4*>(&stg[j * kStgStride + 8 * tt + 4 * hi]) = acc_chunk(v, tt);
        wave_lds_sync();
        float s_ = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s_ += stg[(16 * hi + q) * kStgStride + j];
        wave_lds_sync();
        acc += s_ + __shfl_xor(s_, 32, 64);
    };
    auto publish = [&](const f32x16& v, int rt, int blk) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = v[8 * h + q];
            const BfFrag<NS> f = split8<NS>(x);
#pragma unroll
            for (int pa = 0; pa < NS; ++pa) Zf[(((size_t)rt * TK + 2 * blk + h) * NS + pa) * 64 + lane] = f.t[pa];
        }
    };
    AFrag<NS, FB> ring[RD];
    auto gemm = [&](f32x16(&acc)[FB][RT], const u32x4* const (&cur)[FB], const u32x4* const (&nxt)[FB]) {
#pragma unroll
        for (int fb = 0; fb < FB; ++fb)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[fb][rt][r] = 0.f;
#pragma unroll 1
        for (int kg = 0; kg < TK; kg += RD) {
#pragma unroll
            for (int u = 0; u < RD; ++u) {
                u32x4 bq[NS][RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int pa = 0; pa < NS; ++pa) bq[pa][rt] = Zf[(((size_t)rt * TK + kg + u) * NS + pa) * 64 + lane];
                mma_frags<NS, FB, RT>(acc, ring[u], bq);
                const int g = kg + u + RD;
                const bool wrap = g >= TK;
                const u32x4* nb[FB];
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) nb[fb] = wrap ? nxt[fb] : cur[fb];
                load_aring<NS, FB>(ring[u], nb, wrap ? g - TK : g, lane);
            }
        }
    };
    const int spb = (p.ntiles + NRT - 1) / NRT;
    const long nsuper = (long)spb * p.batch;
    // row metadata of super tile st_ into buffer cbw: thread r < 64 = row j of row tile r / 32
    auto gather_meta = [&](long st_, int cbw) {
        int* m = meta0 + cbw * kMeta;
        const int t0 = (int)(st_ % spb) * NRT;
        if (tid < NRT * 32) {
            const int rt = tid >> 5, jj = tid & 31;
            int oidx = -1, seg = 0, sidx = 0;
            float sc = 1.f;
            if (t0 + rt < p.ntiles) {
                const TileInfo tk = get_tile(p.tiles, t0 + rt, p.rows);
                if (jj == 0) {
                    int* td = m + 4 * NRT * 32 + NRT * 33 + 4 * rt;
                    td[0] = tk.row0;
                    td[1] = tk.nrows;
                    td[2] = tk.seg0;
                    td[3] = tk.nseg | (tk.split ? NLAM_TILE_SPLIT : 0);
                }
                if (jj < tk.nrows) {
                    const int prow = tk.row0 + jj;
                    oidx = p.out_idx != nullptr ? p.out_idx[prow] : prow;
                    seg = p.seg_of_row[prow];
                    sidx = p.src[0].idx != nullptr ? p.src[0].idx[prow] : prow;
                    if (p.flags & NLAM_F_MEAN) sc = p.inv_deg[seg];
                }
            } else if (jj == 0) {
                int* td = m + 4 * NRT * 32 + NRT * 33 + 4 * rt;
                td[0] = td[1] = td[2] = td[3] = 0;
            }
            m[tid] = oidx;
            m[NRT * 32 + tid] = seg;
            m[2 * NRT * 32 + tid] = sidx;
            reinterpret_cast<float*>(m)[3 * NRT * 32 + tid] = sc;
        } else if (tid < NRT * 32 + NRT * 33) {
            const int q = tid - NRT * 32, k = q / 33, l = q - k * 33;
            int rpv = 0;
            if (t0 + k < p.ntiles) {
                const TileInfo tk = get_tile(p.tiles, t0 + k, p.rows);
                if (!tk.split && l <= tk.nseg) rpv = p.rowptr[tk.seg0 + l];
            }
            m[4 * NRT * 32 + q] = rpv;
        }
    };

    const long st_first = xcd_slot((int)blockIdx.x, (int)gridDim.x);
#pragma unroll
    for (int u = 0; u < RD; ++u) load_aring<NS, FB>(ring[u], pb0, u, lane);
    int cb = 0;
    if (st_first < nsuper) gather_meta(st_first, 0);
    __syncthreads();

#pragma unroll 1
    for (long st = st_first; st < nsuper; st += gridDim.x) {
        const int b = (int)(st / spb);
        const long st_next = st + gridDim.x < nsuper ? st + gridDim.x : st;
        const int* m = meta0 + cb * kMeta;
        TileInfo tl[RT];
        bool valid[RT];
        int prow[RT];
        size_t srow_id[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int* td = m + 4 * NRT * 32 + NRT * 33 + 4 * rt;
            tl[rt].row0 = td[0];
            tl[rt].nrows = td[1];
            tl[rt].seg0 = td[2];
            tl[rt].split = (td[3] & NLAM_TILE_SPLIT) != 0;
            tl[rt].nseg = td[3] & ~NLAM_TILE_SPLIT;
            valid[rt] = j < tl[rt].nrows;
            prow[rt] = tl[rt].row0 + j;
            srow_id[rt] = (size_t)b * p.rows + prow[rt];
        }

        // ---- stage A, row tile by row tile: dmsg, LayerNorm sums, column sums ----
        f32x16 dz[FB][RT];
        // xhat of both row tiles is needed again behind the statistics barrier: kept as the raw bf16 halves (8 registers per block
        // instead of 16) where the layer stores bf16, widened at each use
        f32x16 xh[SBF ? 1 : FB][SBF ? 1 : RT];
        u32x4 xkeep[SBF ? FB : 1][SBF ? RT : 1][2];
        float rstd_r[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const float* grow = nullptr;
            const float* garow = nullptr;
            float gscale = 1.f;
            rstd_r[rt] = valid[rt] ? p.rstd[srow_id[rt]] : 0.f;
            if (valid[rt]) {
                if (p.g_out != nullptr) grow = p.g_out + (long)b * p.out_bstride + (long)m[rt * 32 + j] * D_;
                garow = p.g_aggr + ((size_t)b * p.nseg_total + m[NRT * 32 + rt * 32 + j]) * D_;
                gscale = reinterpret_cast<const float*>(m)[3 * NRT * 32 + rt * 32 + j];
            }
            f32x16 g16[FB], ga16[FB];
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
                if constexpr (SBF) load_block_bf16_raw(reinterpret_cast<const bf16s_t*>(p.xhat) + srow_id[rt] * D_, 32 * blk, hi, valid[rt], xkeep[fb][rt]);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const f32x4 g = load_chunk_v<true>(grow, D_, blk * 4 + tt, hi, grow != nullptr);
                    const f32x4 a = load_chunk_v<true>(garow, D_, blk * 4 + tt, hi, garow != nullptr);
                    f32x4 x4 = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (!SBF) x4 = load_chunk_v<true>(valid[rt] ? p.xhat + srow_id[rt] * D_ : nullptr, D_, blk * 4 + tt, hi, valid[rt]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        g16[fb][4 * tt + c] = g[c];
                        ga16[fb][4 * tt + c] = a[c];
                        if constexpr (!SBF) xh[fb][rt][4 * tt + c] = x4[c];
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            float m1 = 0.f, m2 = 0.f;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
                f32x16 xw;
                if constexpr (SBF) xw = block_from_bf16_raw(xkeep[fb][rt]);
                else xw = xh[fb][rt];
#pragma unroll
                for (int r = 0; r < 16; ++r) g16[fb][r] = g16[fb][r] + ga16[fb][r] * gscale;   // dmsg = g_out + g_aggr * scale, in that order
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const f32x4 gm = *reinterpret_cast<const f32x4*>(&gvec[8 * (blk * 4 + tt) + 4 * hi]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float gy = g16[fb][4 * tt + c] * gm[c];
                        dz[fb][rt][4 * tt + c] = gy;
                        m1 += gy;
                        m2 += gy * xw[4 * tt + c];
                    }
                }
                f32x16 gx16;
#pragma unroll
                for (int r = 0; r < 16; ++r) gx16[r] = g16[fb][r] * xw[r];
                colsum_add(g16[fb], acc_dbt[fb]);
                colsum_add(gx16, acc_dg[fb]);
            }
            m1 = row_allreduce(m1);
            m2 = row_allreduce(m2);
            if (hi == 0) {
                red[(fg * NRT + rt) * 32 + j] = m1;
                red[((FG + fg) * NRT + rt) * 32 + j] = m2;
            }
        }
        __syncthreads();
        // ---- LayerNorm finish: dz2, stored for the weight gradient, its column sums, published as B fragments ----
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int w = 0; w < FG; ++w) {
                t1 += red[(w * NRT + rt) * 32 + j];
                t2 += red[((FG + w) * NRT + rt) * 32 + j];
            }
            t1 *= inv_d;
            t2 *= inv_d;
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
                f32x16 xw;
                if constexpr (SBF) xw = block_from_bf16_raw(xkeep[fb][rt]);
                else xw = xh[fb][rt];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = rstd_r[rt] * (dz[fb][rt][r] - t1 - xw[r] * t2);
                    dz[fb][rt][r] = valid[rt] ? v : 0.f;
                }
                if (p.dz2 != nullptr) {
                    if constexpr (SBF) {
                        store_block_bf16(reinterpret_cast<bf16s_t*>(p.dz2) + srow_id[rt] * D_, 32 * blk, hi, valid[rt], dz[fb][rt]);
                    } else {
                        float* drow = p.dz2 + srow_id[rt] * D_;
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) store_chunk_v<true>(drow, D_, blk * 4 + tt, hi, valid[rt], acc_chunk(dz[fb][rt], tt));
                    }
                }
                colsum_add(dz[fb][rt], acc_db2[fb]);
                publish(dz[fb][rt], rt, blk);
            }
        }
        __syncthreads();
        // the next super tile's row metadata (read behind this tile's last barrier); z1 of this one, requested ahead of GEMM dh
        gather_meta(st_next, cb ^ 1);
        u32x4 zraw[FB][RT][2];
        f32x16 zv[FB][RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
                if constexpr (SBF) {
                    load_block_bf16_raw(reinterpret_cast<const bf16s_t*>(p.z1) + srow_id[rt] * D_, 32 * blk, hi, valid[rt], zraw[fb][rt]);
                } else {
                    const float* zrow = valid[rt] ? p.z1 + srow_id[rt] * D_ : nullptr;
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) {
                        const f32x4 z = load_chunk_v<true>(zrow, D_, blk * 4 + tt, hi, valid[rt]);
#pragma unroll
                        for (int c = 0; c < 4; ++c) zv[fb][rt][4 * tt + c] = z[c];
                    }
                }
            }
        __builtin_amdgcn_sched_barrier(0);

        // ---- dh = W2^T dz2 ; dz1 = dh * silu'(z1) ----
        gemm(dz, pb0, pn0);
        __syncthreads();   // every wave is done with the dz2 fragments
        if constexpr (SBF) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) zv[fb][rt] = block_from_bf16_raw(zraw[fb][rt]);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            int raw_ptr = 0;
            if (want2 && lane <= 32) raw_ptr = m[4 * NRT * 32 + rt * 33 + lane];
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const int blk = fg + fb * FG;
#pragma unroll
                for (int r = 0; r < 16; ++r) dz[fb][rt][r] = valid[rt] ? dz[fb][rt][r] * silu_grad_f(zv[fb][rt][r]) : 0.f;
                if (p.dz1 != nullptr) {
                    if constexpr (SBF) {
                        store_block_bf16(reinterpret_cast<bf16s_t*>(p.dz1) + srow_id[rt] * D_, 32 * blk, hi, valid[rt], dz[fb][rt]);
                    } else {
                        float* drow = p.dz1 + srow_id[rt] * D_;
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) store_chunk_v<true>(drow, D_, blk * 4 + tt, hi, valid[rt], acc_chunk(dz[fb][rt], tt));
                    }
                }
                // column sum (db1) and, for the receiver-gathered addend, the segment sum of dz1 over each receiver's rows: one staging
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) *reinterpret_cast<f32x4*>(&stg[j * kStgStride + 8 * tt + 4 * hi]) = acc_chunk(dz[fb][rt], tt);
                wave_lds_sync();
                {
                    float s_ = 0.f;
#pragma unroll
                    for (int q = 0; q < 16; ++q) s_ += stg[(16 * hi + q) * kStgStride + j];
                    acc_db1[fb] += s_ + __shfl_xor(s_, 32, 64);
                }
                if (want2 && tl[rt].nseg > 0)
                    block_segment_reduce(stg, tl[rt], raw_ptr, 1.f, p.dsrc[2] + (long)b * p.dsrc_bstride[2] + 32 * blk, D_, 32, lane);
                wave_lds_sync();
                publish(dz[fb][rt], rt, blk);
            }
        }
        __syncthreads();
        if (want0) {
            // the residual rows (d edge_out passes through the edge update) requested ahead of GEMM dx
            const bool add_gout = (p.flags & NLAM_F_ADD_SRC0) != 0 && p.g_out != nullptr;
            const bool acc0 = (p.flags & NLAM_F_ACC_DSRC0) != 0;
            f32x4 rs[FB][RT][4];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float* grow = (valid[rt] && add_gout) ? p.g_out + (long)b * p.out_bstride + (long)m[rt * 32 + j] * D_ : nullptr;
#pragma unroll
                for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) rs[fb][rt][tt] = load_chunk_v<true>(grow, D_, (fg + fb * FG) * 4 + tt, hi, grow != nullptr);
            }
            __builtin_amdgcn_sched_barrier(0);
            // ---- dx_e = W1_e^T dz1, scattered through the edge index ----
            gemm(dz, pb1, pb0);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                float* drow = valid[rt] ? p.dsrc[0] + (long)b * p.dsrc_bstride[0] + (long)m[2 * NRT * 32 + rt * 32 + j] * D_ : nullptr;
                if (acc0) {   // an earlier autoregressive step's gradient of the same tensor is already there
                    f32x4 pv[FB][4];
#pragma unroll
                    for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) pv[fb][tt] = load_chunk_v<true>(drow, D_, (fg + fb * FG) * 4 + tt, hi, drow != nullptr);
#pragma unroll
                    for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt) rs[fb][rt][tt] += pv[fb][tt];
                }
#pragma unroll
                for (int fb = 0; fb < FB; ++fb)
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt)
                        store_chunk_v<true>(drow, D_, (fg + fb * FG) * 4 + tt, hi, valid[rt], acc_chunk(dz[fb][rt], tt) + rs[fb][rt][tt]);
            }
        }
        __syncthreads();   // super tile end: the fragments, red and the metadata buffer are rewritten
        cb ^= 1;
    }

    if (p.vec_partials != nullptr) {
        float* vp = p.vec_partials + (size_t)blockIdx.x * 4 * p.vec_stride;
#pragma unroll
        for (int fb = 0; fb < FB; ++fb) {
            const int c = 32 * (fg + fb * FG) + j;
            if (hi == 0 && c < p.vec_stride) {
                vp[0 * p.vec_stride + c] = acc_db1[fb];
                vp[1 * p.vec_stride + c] = acc_db2[fb];
                vp[2 * p.vec_stride + c] = acc_dg[fb];
                vp[3 * p.vec_stride + c] = acc_dbt[fb];
            }
        }
        for (int c = D_ + fg * 64 + lane; c < p.vec_stride; c += FG * 64) {
#pragma unroll
            for (int k = 0; k < 4; ++k) vp[k * p.vec_stride + c] = 0.f;
        }
    }
}

template <int NS_, int D_>
constexpr size_t bwd_edge_lds() {
    return (size_t)2 * (D_ / 16) * NS_ * 1024 + (size_t)8 * 32 * kStgStride * 4 + (size_t)2 * 8 * 2 * 32 * 4 + (size_t)D_ * 4 +
           (size_t)2 * (4 * 2 * 32 + 2 * 33 + 2 * 4) * 4;
}

struct WbfBwdPlan {
    int cfg;   // 0 = not covered; 8 waves: 1: <4,1,2> (<= 128)  2: <8,1,2> (<= 256)  3: <8,2,1> (<= 512)
               // 4 waves, two workgroups per CU (NLAM_TUNE_WBF_HALF bit 1): 5: <4,2,1> (128 < d <= 256)
    int fg, fb, rt, rg, nrt, nw;
};

WbfBwdPlan wbf_bwd_plan(int maxw) {
    if (maxw <= 128) return {1, 4, 1, 2, 2, 4, 8};
    if (maxw <= 256) return {2, 8, 1, 2, 1, 2, 8};
    if (maxw <= kMaxWide) return {3, 8, 2, 1, 1, 1, 8};
    return {0, 0, 0, 0, 0, 0, 0};
}

// the plan a launch runs: the 8-wave plan decides coverage (bwd_wbf_ns); with NLAM_TUNE_WBF_HALF bit 1 the widths that have a
// 4-wave instantiation take it (see wbf_half_plan)
WbfBwdPlan wbf_bwd_choose(int maxw) {
    const WbfBwdPlan pl = wbf_bwd_plan(maxw);
    if (pl.cfg == 2 && (::nlam_detail::wbf_half & 2)) return {5, 4, 2, 1, 1, 1, 4};
    return pl;
}

int bwd_wide_maxw(const nlam_mlp_bwd_t* p);   // nlam_hip.hip

int bwd_wbf_ns(const nlam_mlp_bwd_t* p) {
    int ns = (int)((p->flags & NLAM_F_MM_MASK) >> NLAM_F_MM_SHIFT);
    if (ns == 0) return 0;
    // an output width that is not a multiple of 4 (output_map: 17 state variables) is read / written element-wise (load_chunk /
    // store_chunk) and its W2^T is zero-padded by the pack kernel; dz2 then has a 32-padded row stride (nlam_mlp_bwd_dz2_ld)
    if (p->hid % 4 != 0) return 0;
    for (int s = 0; s < p->nsrc; ++s)
        if (p->dmode[s] != 0 && p->src[s].width % 4 != 0) return 0;
    if (p->flags & NLAM_F_PRE_ADD)
        for (int s = 1; s < p->nsrc; ++s)
            if (p->src[s].width != p->hid || p->hid % 32 != 0 || (p->flags & NLAM_F_ADD_SRC1) || (p->dmode[s] != 0 && p->dmode[s] != 3)) return 0;
    const WbfBwdPlan pl = wbf_bwd_plan(bwd_wide_maxw(p));
    long min_st = ::nlam_detail::wbf_min_supertiles;
    if (pl.cfg == 3 && min_st > 8) min_st = 8;   // as in the forward: the fp32 <8,2> backward spills
    if (pl.cfg == 0 || (long)p->ntiles * p->batch < min_st * pl.nrt) return 0;
    return ns == 2 ? 3 : ns;
}

int64_t bwd_wbf_wpack_floats(const nlam_mlp_bwd_t* p, int ns) {
    const int64_t HBT = (p->hid + 31) / 32, OBT = (p->dout + 31) / 32;
    const int64_t TKA = wbf_bwd_tk((int)OBT, ns), TKB = wbf_bwd_tk((int)HBT, ns);
    int64_t groups = HBT * TKA;
    for (int s = 0; s < p->nsrc; ++s)
        if (p->dmode[s] != 0 && (s == 0 || (p->flags & NLAM_F_PRE_ADD) == 0)) groups += (int64_t)((p->src[s].width + 31) / 32) * TKB;
    return groups * ns * 256;
}

size_t bwd_wbf_lds(const nlam_mlp_bwd_t* p, int ns, const WbfBwdPlan& pl) {
    const size_t HBT = (p->hid + 31) / 32, OBT = (p->dout + 31) / 32;
    const size_t TKM = (size_t)wbf_bwd_tk((int)(HBT > OBT ? HBT : OBT), ns);
    return (size_t)pl.nrt * TKM * ns * 1024 + (size_t)pl.nw * 32 * kStgStride * 4 + (size_t)2 * pl.fg * pl.nrt * 32 * 4 + OBT * 32 * 4;
}
