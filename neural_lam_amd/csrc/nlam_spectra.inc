// nlam_dct_spectra: binned variance spectra of lattice fields from a 2-D orthonormal DCT (Denis, Cote and Laprise 2002), inside the
// recorded forecast step (before nlam_forecast_finish).  The grid is a lattice: node n = i * ny + j; the window is cx x cy.
//
// At the sizes of a limited-area grid (268 x 238 = 4 * 67 x 2 * 7 * 17) a matrix DCT on the matrix cores is the algorithm, not an
// FFT: G = Cx g Cy^T as two fp32 GEMMs on v_mfma_f32_16x16x4_f32, whose result is bit for bit the fp32 fmaf chain in ascending k
// that the tests' error budget assumes.  Three launches for every size; an item is one (source, batch item):
//   pass 1  along j.  T[i][n'][v] = sum_j Cy[n'][j] x[i][j][var[v]]: M = K = cy, and the N dimension is (i, v) -- with V <= 64
//           a tile holds 64 / V whole rows i.  The B operand is the contiguous (cy, F) slab of row i: a K tile of it is read with
//           16-byte loads where the address allows and the V selected variables are picked as it is written to LDS (an inverse
//           table f -> v, chained so that a variable listed twice works), so every cache line of x is used whole.  The M tiles of
//           one column block are neighbours in launch order and share the slab through the L2.
//   pass 2  along i.  G[m][(n', v)] = sum_i Cx[m][i] T[i][(n', v)]: a plain GEMM, M = K = cx, N = cy * V, B row-major contiguous.
//   bins    one workgroup per (item, bin): thread (e, v) adds G^2 of the bin's entries e, e + EP, ... (EP = 256 / V) in list
//           order, the EP partial sums of a variable are added in order by one thread, times scale_v / (cx cy) in float64,
//           rounded once.  An empty bin writes 0.
// Both GEMMs are one kernel template: a workgroup of four waves owns a 64 x 64 tile of the output, a wave 32 x 32 of it as 2 x 2
// MFMA tiles (four independent accumulators cover the 40-cycle dependent latency), K in tiles of 32 through LDS.  Ragged edges
// are zero fill: every word of the A tile is written (0 outside M and K), the rows of the B tile past K are zeroed, and the
// columns of a B tile past N only feed output columns that are never stored.  Nothing outside the window is read.
// No floating-point atomics: two runs give the same bits.  All kernels only read *lead and do nothing once *lead >= max_lead.
// Table values are clamped as they are read: the window's origin into [0, nx - cx] x [0, ny - cy], var into [0, d_state),
// bin_ptr into [0, bin_entries], bin_idx into [0, cx cy).
// Included from nlam_hip.hip inside NLAM_IN_TU(1).

namespace {

constexpr int kSpecTile = 64;   // rows and columns of a workgroup's output tile
constexpr int kSpecKT = 32;     // K per LDS tile
constexpr int kSpecLDA = 81;    // words between two k rows of the A tile: odd, the transposing scalar writes spread over the banks
constexpr int kSpecLDB = 80;    // and of the B tile: a multiple of 4 (16-byte writes), 16 mod 64 (the four k rows of an operand read)

struct SpecSrc {
    const float* x;
    float* spec;
    long batch_stride, lead_stride;
    int batch, physical, first;   // first: items of the sources before this one
};

// source s of the call by three uniform branches, never by an index: the argument struct stays where the kernel arguments are
__device__ __forceinline__ SpecSrc spec_src(const nlam_dct_spectra_t& p, int s) {
    const auto pick = [](const nlam_dct_spectra_src_t& q, int first) {
        return SpecSrc{q.x, q.spec, (long)q.batch_stride, (long)q.lead_stride, q.batch, q.physical, first};
    };
    if (s == 0) return pick(p.src[0], 0);
    if (s == 1) return pick(p.src[1], p.src[0].batch);
    return pick(p.src[2], p.src[0].batch + p.src[1].batch);
}
__device__ __forceinline__ int spec_items(const nlam_dct_spectra_t& p) {
    return p.src[0].batch + (p.sources > 1 ? p.src[1].batch : 0) + (p.sources > 2 ? p.src[2].batch : 0);
}

// columns of a pass-1 tile: whole rows i where a row's V columns fit
__host__ __device__ __forceinline__ int spec_tile_cols(int V) { return V <= kSpecTile ? (kSpecTile / V) * V : kSpecTile; }

// PASS 1: T = Cy x (along j); PASS 2: G = Cx T (along i).
// blockIdx.x = M tile + tiles_m * column tile, .y = item of the source, .z = source
template <int PASS>
__global__ __launch_bounds__(256) void spec_gemm_kernel(const nlam_dct_spectra_t p, int tiles_m) {
    __shared__ __attribute__((aligned(16))) float As[kSpecKT * kSpecLDA];
    __shared__ __attribute__((aligned(16))) float Bs[kSpecKT * kSpecLDB];
    __shared__ int vfirst[PASS == 1 ? NLAM_EVAL_MAX_VARS : 1];   // the first v with var[v] == f, or -1
    __shared__ int vnext[PASS == 1 ? NLAM_EVAL_MAX_VARS : 1];    // the next v with the same variable, or -1
    const int lead = *p.lead;
    if (lead >= p.max_lead) return;   // the same in every thread of the grid, ahead of every barrier
    const SpecSrc src = spec_src(p, blockIdx.z);
    const int b = blockIdx.y;
    if (b >= src.batch) return;       // the same in every thread of the workgroup
    const int cx = p.cx, cy = p.cy, V = p.vars, F = p.d_state;
    const int i0 = min(max(p.origin[0], 0), p.nx - cx), j0 = min(max(p.origin[1], 0), p.ny - cy);   // only pass 1 reads the grid
    const int KD = PASS == 1 ? cy : cx;                 // M and K of the product
    const int NC = (PASS == 1 ? cx : cy) * V;           // its columns
    const int TN = PASS == 1 ? spec_tile_cols(V) : kSpecTile;
    const int tm = blockIdx.x % tiles_m, tn = blockIdx.x / tiles_m;
    const int m0 = tm * kSpecTile, c0 = tn * TN, c1 = min(NC, c0 + TN);
    const float* const A = PASS == 1 ? p.basis_y : p.basis_x;
    const long per = (long)cx * cy * V;
    float* const T = p.workspace + (long)(src.first + b) * per;
    float* const G = p.workspace + ((long)spec_items(p) + src.first + b) * per;
    const float* const xb = src.x + (long)b * src.batch_stride + (long)lead * src.lead_stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;

    if (PASS == 1) {
        for (int f = tid; f < F; f += 256) vfirst[f] = -1;
        __syncthreads();
        if (tid == 0)
            for (int v = V - 1; v >= 0; --v) {   // the chains ascend in v
                const int f = min(max(p.var[v], 0), F - 1);
                vnext[v] = vfirst[f];
                vfirst[f] = v;
            }
        __syncthreads();
    }

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < KD; k0 += kSpecKT) {
        const int kt = min(kSpecKT, KD - k0);
        // A tile, transposed: As[k][m] = A[m0 + m][k0 + k], 0 outside; consecutive lanes read consecutive k
#pragma unroll
        for (int u = 0; u < kSpecTile * kSpecKT / 256; ++u) {
            const int idx = tid + 256 * u, k = idx & (kSpecKT - 1), m = idx / kSpecKT;
            As[k * kSpecLDA + m] = (m0 + m < KD && k < kt) ? A[(long)(m0 + m) * KD + k0 + k] : 0.f;
        }
        if (PASS == 1) {
            // rows r_lo .. r_hi of the window have columns in this tile; of each, the kt * F floats of j = k0 .. k0 + kt - 1
            const int r_lo = c0 / V, nrows = (c1 - 1) / V - r_lo + 1;
            const int len = kt * F, nqmax = (len + 6) / 4;
            const bool vec = (reinterpret_cast<uintptr_t>(xb) & 15) == 0;
            for (int idx = tid; idx < nrows * nqmax; idx += 256) {
                const int rr = idx / nqmax, q = idx - rr * nqmax, r = r_lo + rr;
                const long seg0 = ((long)(i0 + r) * p.ny + j0 + k0) * F, seg1 = seg0 + len;
                const long a = (vec ? seg0 & ~3L : seg0) + 4L * q;   // quads on 16-byte addresses
                if (a >= seg1) continue;
                f32x4 val = {0.f, 0.f, 0.f, 0.f};
                if (vec && a >= seg0 && a + 3 < seg1) {
                    val = *reinterpret_cast<const f32x4*>(xb + a);
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (a + c >= seg0 && a + c < seg1) val[c] = xb[a + c];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (a + c < seg0 || a + c >= seg1) continue;
                    const int rel = (int)(a + c - seg0), j = rel / F, f = rel - j * F;
                    for (int v = vfirst[f]; v >= 0; v = vnext[v]) {
                        const int col = r * V + v - c0;
                        if (col >= 0 && col < c1 - c0) Bs[j * kSpecLDB + col] = val[c];
                    }
                }
            }
            // rows of the tile past K
            for (int idx = tid; idx < (kSpecKT - kt) * kSpecTile; idx += 256)
                Bs[(kt + idx / kSpecTile) * kSpecLDB + (idx & (kSpecTile - 1))] = 0.f;
        } else {
            // Bs[k][c] = T[k0 + k][c0 + c], 0 outside
#pragma unroll
            for (int u = 0; u < kSpecKT * kSpecTile / 4 / 256; ++u) {
                const int idx = tid + 256 * u, k = idx / (kSpecTile / 4), cq = 4 * (idx & (kSpecTile / 4 - 1));
                f32x4 val = {0.f, 0.f, 0.f, 0.f};
                if (k < kt) {
                    const float* const row = T + (long)(k0 + k) * NC + c0 + cq;
                    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0 && c0 + cq + 3 < NC) {
                        val = *reinterpret_cast<const f32x4*>(row);
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (c0 + cq + c < NC) val[c] = row[c];
                    }
                }
                *reinterpret_cast<f32x4*>(&Bs[k * kSpecLDB + cq]) = val;
            }
        }
        __syncthreads();
        // lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15] of a 16 x 16 x 4 step
        const int kl = lane >> 4, cl = lane & 15;
#pragma unroll
        for (int ks = 0; ks < kSpecKT; ks += 4) {
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                av[i] = As[(ks + kl) * kSpecLDA + wm + 16 * i + cl];
                bv[i] = Bs[(ks + kl) * kSpecLDB + wn + 16 * i + cl];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();   // the next K tile overwrites both tiles
    }

    // D: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + wn + 16 * j + (lane & 15);
            if (c >= c1) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + 4 * (lane >> 4) + r;
                if (m >= KD) continue;
                if (PASS == 1) {
                    const int ii = c / V, v = c - ii * V;
                    T[((long)ii * cy + m) * V + v] = acc[i][j][r];
                } else {
                    G[(long)m * NC + c] = acc[i][j][r];
                }
            }
        }
}

// blockIdx.x = bin, .y = item of the source, .z = source
__global__ __launch_bounds__(256) void spec_bins_kernel(const nlam_dct_spectra_t p) {
    __shared__ float part[256];
    const int lead = *p.lead;
    if (lead >= p.max_lead) return;
    const SpecSrc src = spec_src(p, blockIdx.z);
    const int b = blockIdx.y, bin = blockIdx.x;
    if (b >= src.batch) return;
    const int cx = p.cx, cy = p.cy, V = p.vars, cells = cx * cy;
    const int EP = 256 / V;   // entries in flight; V <= NLAM_EVAL_MAX_VARS = 256
    const int t = threadIdx.x, e = t / V, v = t - e * V;
    const int lo = min(max(p.bin_ptr[bin], 0), p.bin_entries), hi = min(max(p.bin_ptr[bin + 1], lo), p.bin_entries);
    const float* const G = p.workspace + ((long)spec_items(p) + src.first + b) * ((long)cells * V);
    float acc = 0.f;
    if (e < EP)
        for (int q = lo + e; q < hi; q += EP) {
            const int idx = min(max(p.bin_idx[q], 0), cells - 1);
            const float g = G[(long)idx * V + v];
            acc = fmaf(g, g, acc);
        }
    part[t] = acc;
    __syncthreads();
    if (t >= V) return;
    float sum = 0.f;
    for (int i = 0; i < EP; ++i) sum += part[i * V + t];
    double scale = 1.0 / (double)cells;
    if (!src.physical) {
        const double sd = (double)p.state_std[min(max(p.var[t], 0), p.d_state - 1)];
        scale *= sd * sd;
    }
    src.spec[(((long)b * p.max_lead + lead) * V + t) * p.bins + bin] = (float)((double)sum * scale);
}

// the size checks nlam_dct_spectra and its workspace function share
int32_t spec_sizes_check(long items, long cx, long cy, long vars) {
    if (items < 1 || vars < 1 || cx < 2 || cy < 2) return NLAM_EINVAL;
    if (items > NLAM_SPEC_MAX_SOURCES * 65535L || vars > NLAM_EVAL_MAX_VARS) return NLAM_EUNSUP;
    if (cx >= (1L << 31) || cy >= (1L << 31) || cx * cy >= (1L << 31) || cx * cy * vars >= (1L << 31)) return NLAM_EUNSUP;
    return 0;
}

// every check before any launch
int32_t dct_spectra_check(const nlam_dct_spectra_t* p) {
    if (p == nullptr || p->lead == nullptr || p->max_lead < 1) return NLAM_EINVAL;
    if (p->sources < 1 || p->sources > NLAM_SPEC_MAX_SOURCES) return NLAM_EINVAL;
    if (p->nx < 1 || p->ny < 1 || p->d_state < 1 || p->vars < 1 || p->bins < 1) return NLAM_EINVAL;
    if (p->cx < 2 || p->cy < 2 || p->cx > p->nx || p->cy > p->ny) return NLAM_EINVAL;
    const long cx = p->cx, cy = p->cy;
    long items = 0;
    bool standardised = false;
    for (int s = 0; s < p->sources; ++s) {
        const nlam_dct_spectra_src_t& q = p->src[s];
        if (q.batch < 1 || q.batch_stride < 0 || q.lead_stride < 0) return NLAM_EINVAL;
        items += q.batch;
        standardised |= q.physical == 0;
    }
    if (p->d_state > NLAM_EVAL_MAX_VARS || p->vars > p->d_state) return NLAM_EUNSUP;
    for (int s = 0; s < p->sources; ++s)
        if (p->src[s].batch > 65535) return NLAM_EUNSUP;
    if ((long)p->nx * p->ny >= (1L << 31) || (long)p->nx * p->ny * p->d_state >= (1L << 31)) return NLAM_EUNSUP;
    if (const int32_t rc = spec_sizes_check(items, cx, cy, p->vars)) return rc;
    if (p->bin_entries < 0 || p->bin_entries > cx * cy) return NLAM_EINVAL;
    if (p->origin == nullptr || p->basis_x == nullptr || p->basis_y == nullptr || p->var == nullptr || p->bin_ptr == nullptr ||
        p->bin_idx == nullptr || p->workspace == nullptr || (standardised && p->state_std == nullptr))
        return NLAM_EINVAL;
    for (int s = 0; s < p->sources; ++s)
        if (p->src[s].x == nullptr || p->src[s].spec == nullptr) return NLAM_EINVAL;
    if (p->workspace_floats < 2 * items * cx * cy * p->vars) return NLAM_EINVAL;
    return 0;
}

}  // namespace

extern "C" {

int32_t nlam_dct_spectra(const nlam_dct_spectra_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_dct_spectra");
    if (const int32_t rc = dct_spectra_check(p)) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const long cx = p->cx, cy = p->cy, V = p->vars;
    int batch = 0;
    for (int s = 0; s < p->sources; ++s) batch = std::max(batch, p->src[s].batch);
    const auto tiles = [](long n, long t) { return (n + t - 1) / t; };
    const long tm1 = tiles(cy, kSpecTile), tm2 = tiles(cx, kSpecTile);
    const long g1 = tm1 * tiles(cx * V, spec_tile_cols((int)V)), g2 = tm2 * tiles(cy * V, kSpecTile);   // < 2^31: cx cy V is
    hipLaunchKernelGGL(spec_gemm_kernel<1>, dim3((unsigned)g1, batch, p->sources), dim3(256), 0, stream, *p, (int)tm1);
    if (const hipError_t e = hipGetLastError()) return (int32_t)e;   // nothing more is queued behind a launch that failed
    hipLaunchKernelGGL(spec_gemm_kernel<2>, dim3((unsigned)g2, batch, p->sources), dim3(256), 0, stream, *p, (int)tm2);
    if (const hipError_t e = hipGetLastError()) return (int32_t)e;
    hipLaunchKernelGGL(spec_bins_kernel, dim3(p->bins, batch, p->sources), dim3(256), 0, stream, *p);
    return (int32_t)hipGetLastError();
}

int64_t nlam_dct_spectra_workspace_floats(int32_t items, int32_t cx, int32_t cy, int32_t vars) {
    if (const int32_t rc = spec_sizes_check(items, cx, cy, vars)) return rc;
    return 2L * items * cx * cy * vars;
}

}  // extern "C"
