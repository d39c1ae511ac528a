// nlam_ens_neighbourhood: neighbourhood probabilities of the events of nlam_ens_products over a ladder of square windows, and the
// two sums of the fractions skill score (Roberts and Lean 2008), inside the recorded forecast step (after nlam_ens_products,
// before nlam_forecast_finish).  The grid is a lattice here: node n = i * ny + j.
//
// Every window sum is an integer, so it is exact in any order, and it comes from summed-area tables in the workspace: one int32
// table of nx * ny words for the live mask, and one each per (start, event) for C (the members of a live node in the event) and
// O (1 where the truth of a live node is in it).  Five launches, four with truth == NULL, whatever S, M, E, W and the radii:
//   count   the geometry of ens_products_kernel: a workgroup owns (start, chunk of fc_chunk_nodes whole nodes) and passes the chunk
//           through an LDS tile in pieces of whole nodes -- rows 0 .. M - 1 the members, row M the truth -- with 16-byte loads
//           where every row of the piece is aligned (DESIGN 4.17's rule); one thread per (event, node), node-minor, counts the
//           members in the event and stores C and O of the node, 0 where the node is dead: table[e][n] is contiguous in n, so
//           consecutive lanes write consecutive words.  The workgroups of start 0 store the live mask.  Every state element is
//           read here, once.
//   rows    inclusive running sums along j, in place.  All tables are one contiguous array of rows; a wave owns 64 / L rows at
//           a time, L = min(64, ny rounded up to a power of two) lanes each, scans 64 words per step with __shfl_up inside the
//           L lanes of a row and carries the last lane's sum to the next step.
//   cols    inclusive running sums along i, in place: one thread per (table, j), consecutive lanes on consecutive j, eight loads
//           in flight.
//   eval    one thread per node, blockIdx.y = event, blockIdx.z = start: per scale the window is clipped to the grid and A, SC,
//           SO are four corners of a table each -- the cost does not depend on the radius --, nprob = (float)SC / (float)(M A)
//           goes straight to global memory (contiguous in n), and with the truth the node's two terms are added over the
//           workgroup in a fixed order (shuffles inside a wave, the four waves through LDS) into the workgroup's own words.
//   finish  one wave per (start, event, scale, sum): the workgroups' words in a fixed order.
// No floating-point atomics: two runs give the same bits.  members * nx * ny <= 2^24 is required, so every table entry and M A
// are integers a float holds exactly and nprob is one correctly rounded division.  All kernels only read *lead and do nothing
// once *lead >= max_lead.  The tables' values are clamped as they are staged: a variable index into [0, d_state), a radius into
// [0, max(nx, ny)] (a window that large is the whole grid, and i + r cannot overflow).
// Included from nlam_hip.hip inside NLAM_IN_TU(1), behind nlam_ens_products.inc (kEnsTileFloats; fc_chunk_nodes, launch<>).

namespace {

constexpr int kNbrTabWords = 3 * NLAM_ENS_MAX_EVENTS;
constexpr int kNbrThreads = 256;        // nodes per workgroup of the evaluation pass
constexpr int kNbrMaxBlocks = 1 << 16;  // workgroups of the two scans: they stride over their rows / columns

// whole nodes per piece of the counting pass: what kEnsTileFloats words hold of M + 1 tile rows and the tables; a multiple of 4
// where there are that many, never more than the chunk
__host__ __device__ __forceinline__ int nbr_tile_nodes(int nvars, int members) {
    int n = (kEnsTileFloats - kNbrTabWords) / ((members + 1) * nvars);
    if (n >= 4) n &= ~3;
    const int cn = fc_chunk_nodes(nvars);
    return n < 1 ? 1 : (n > cn ? cn : n);
}
__host__ __device__ __forceinline__ int nbr_stride(int tile_nodes, int nvars) { return (tile_nodes * nvars + 3) & ~3; }
__host__ __device__ __forceinline__ long nbr_blocks(long nodes) { return (nodes + kNbrThreads - 1) / kNbrThreads; }
// words of the tables: the live mask, then C and O of every (start, event)
__host__ __device__ __forceinline__ long nbr_table_words(long starts, long events, long nodes) { return nodes * (1 + 2 * starts * events); }
__host__ __device__ __forceinline__ long nbr_ws_words(long starts, long events, long scales, long nodes) {
    return nbr_table_words(starts, events, nodes) + 2 * starts * events * scales * nbr_blocks(nodes);
}

__global__ __launch_bounds__(256) void nbr_count_kernel(const nlam_ens_neighbourhood_t p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (*p.lead >= p.max_lead) return;   // the same in every thread of the grid, ahead of every barrier
    const int M = p.members, F = p.d_state, E = p.events;
    const int N = p.nx * p.ny;
    const int s = blockIdx.y, chunk = blockIdx.x;
    const int cn = fc_chunk_nodes(F), tn = nbr_tile_nodes(F, M), stride = nbr_stride(tn, F);
    const int n0 = chunk * cn, n1 = min(N, n0 + cn);
    const long per = (long)N * F;
    const bool score = p.truth != nullptr;
    float* const tile = smem;
    int* const evar = reinterpret_cast<int*>(tile + (M + 1) * stride);
    int* const esense = evar + NLAM_ENS_MAX_EVENTS;
    float* const ethr = reinterpret_cast<float*>(esense + NLAM_ENS_MAX_EVENTS);
    for (int i = threadIdx.x; i < E; i += blockDim.x) {
        evar[i] = min(max(p.event_var[i], 0), F - 1);
        esense[i] = p.event_sense[i];
        ethr[i] = p.event_thr[i];
    }
    int* const live = reinterpret_cast<int*>(p.workspace);
    int* const tc = live + N + (long)s * E * N;
    int* const to = tc + (long)p.starts * E * N;
    if (s == 0)
        for (int n = n0 + threadIdx.x; n < n1; n += blockDim.x) live[n] = p.row_weight[n] != 0.f ? 1 : 0;
    for (int t0 = n0; t0 < n1; t0 += tn) {
        const int t1 = min(n1, t0 + tn), tnodes = t1 - t0;
        const int cnt_e = tnodes * F, nq = (cnt_e + 3) / 4;
        const long base = (long)t0 * F;
        const float* const x0 = p.prev + (long)s * M * per + base;
        const float* const y0 = score ? p.truth + (long)s * M * per + base : x0;
        const bool vec_in = ((reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(y0)) & 15) == 0 && (M == 1 || (per & 3) == 0);
        for (int i = threadIdx.x; i < (M + (score ? 1 : 0)) * nq; i += blockDim.x) {   // rows 0 .. M - 1: the members, row M: the truth
            const int m = i / nq, e = 4 * (i - m * nq);
            const float* const src = m < M ? x0 + (long)m * per : y0;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (vec_in && e + 3 < cnt_e) {
                v = *reinterpret_cast<const f32x4*>(src + e);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (e + c < cnt_e) v[c] = src[e + c];
            }
            *reinterpret_cast<f32x4*>(tile + m * stride + e) = v;   // e + 3 < stride: tn * F rounded up to a quad
        }
        __syncthreads();   // the tile and, the first time, the tables
        for (int i = threadIdx.x; i < E * tnodes; i += blockDim.x) {   // (event, node), node-minor
            const int ev = i / tnodes, r = i - ev * tnodes;
            const float* const col = tile + r * F + evar[ev];
            const float thr = ethr[ev];
            const bool less = esense[ev] != 0;
            const bool alive = p.row_weight[t0 + r] != 0.f;
            int c = 0;
            for (int m = 0; m < M; ++m) {
                const float v = col[m * stride];
                c += (less ? v < thr : v > thr) ? 1 : 0;
            }
            tc[(long)ev * N + t0 + r] = alive ? c : 0;
            if (score) {
                const float y = col[M * stride];
                to[(long)ev * N + t0 + r] = alive && (less ? y < thr : y > thr) ? 1 : 0;
            }
        }
        __syncthreads();   // the next piece overwrites the tile
    }
}

// lanes of a wave per row of the scan: ny rounded up to a power of two, 64 at the most
__host__ __device__ __forceinline__ int nbr_row_lanes(int ny) {
    int l = 1;
    while (l < 64 && l < ny) l <<= 1;
    return l;
}

// `rows` rows of ny words, contiguous: every table's rows, one after the other
__global__ __launch_bounds__(256) void nbr_rows_kernel(const nlam_ens_neighbourhood_t p, long rows) {
    if (*p.lead >= p.max_lead) return;
    const int ny = p.ny, L = nbr_row_lanes(ny), per_wave = 64 / L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / L, sl = lane - sub * L;
    int* const tab = reinterpret_cast<int*>(p.workspace);
    const long step = (long)gridDim.x * 4 * per_wave;
    for (long first = ((long)blockIdx.x * 4 + wave) * per_wave; first < rows; first += step) {   // the same in every lane of the wave
        const long row = first + sub;
        int* const r = tab + row * ny;
        int carry = 0;
        for (int j0 = 0; j0 < ny; j0 += L) {
            const int j = j0 + sl;
            const bool in = row < rows && j < ny;
            int v = in ? r[j] : 0;
            for (int d = 1; d < L; d <<= 1) {
                const int t = __shfl_up(v, d, L);   // the row's own L lanes: the lanes below d get their own value back
                if (sl >= d) v += t;
            }
            v += carry;
            if (in) r[j] = v;
            carry = __shfl(v, L - 1, L);
        }
    }
}

// `cols` = tables * ny columns of nx words, ny apart
__global__ __launch_bounds__(256) void nbr_cols_kernel(const nlam_ens_neighbourhood_t p, long cols) {
    if (*p.lead >= p.max_lead) return;
    const int nx = p.nx, ny = p.ny;
    const long N = (long)nx * ny;
    int* const tab = reinterpret_cast<int*>(p.workspace);
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += (long)gridDim.x * blockDim.x) {
        const long t = c / ny;
        int* const col = tab + t * N + (c - t * ny);
        int acc = 0, i = 0;
        for (; i + 8 <= nx; i += 8) {
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = col[(long)(i + u) * ny];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc += v[u];
                col[(long)(i + u) * ny] = acc;
            }
        }
        for (; i < nx; ++i) {
            acc += col[(long)i * ny];
            col[(long)i * ny] = acc;
        }
    }
}

// the sum of the table over rows i0 .. i1, columns j0 .. j1 (inside the grid)
__device__ __forceinline__ int nbr_box(const int* t, int ny, int i0, int i1, int j0, int j1) {
    const int a = t[i1 * ny + j1];
    const int b = i0 > 0 ? t[(i0 - 1) * ny + j1] : 0;
    const int c = j0 > 0 ? t[i1 * ny + j0 - 1] : 0;
    const int d = i0 > 0 && j0 > 0 ? t[(i0 - 1) * ny + j0 - 1] : 0;
    return (a - b) - (c - d);
}

// blockIdx.x = 256 nodes, blockIdx.y = event, blockIdx.z = start
__global__ __launch_bounds__(kNbrThreads) void nbr_eval_kernel(const nlam_ens_neighbourhood_t p) {
    __shared__ int rad[NLAM_NBR_MAX_SCALES];
    __shared__ float red[4][2 * NLAM_NBR_MAX_SCALES];
    const int k = *p.lead;
    if (k >= p.max_lead) return;
    const int nx = p.nx, ny = p.ny, N = nx * ny, E = p.events, W = p.scales;
    const int e = blockIdx.y, s = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool score = p.truth != nullptr;
    if (threadIdx.x < W) rad[threadIdx.x] = min(max(p.radius[threadIdx.x], 0), max(nx, ny));
    __syncthreads();
    const int* const live = reinterpret_cast<const int*>(p.workspace);
    const int* const tc = live + N + ((long)s * E + e) * N;
    const int* const to = tc + (long)p.starts * E * N;
    const int n = blockIdx.x * kNbrThreads + threadIdx.x;
    const bool in = n < N;
    const int i = in ? n / ny : 0, j = in ? n - i * ny : 0;
    const float wn = in ? p.row_weight[n] : 0.f;
    float* const out = p.nprob + (((long)s * p.max_lead + k) * E + e) * W * N + n;
    for (int w = 0; w < W; ++w) {
        const int r = rad[w];
        const int i0 = max(i - r, 0), i1 = min(i + r, nx - 1), j0 = max(j - r, 0), j1 = min(j + r, ny - 1);
        float tf = 0.f, tr = 0.f;
        if (in) {
            const int A = nbr_box(live, ny, i0, i1, j0, j1);
            const int SC = nbr_box(tc, ny, i0, i1, j0, j1);
            const float fa = (float)A;
            const float pr = A == 0 ? __int_as_float(0x7fc00000) : (float)SC / (float)(p.members * A);
            out[(long)w * N] = pr;
            if (score && wn != 0.f) {   // a live node is in its own window: A >= 1
                const float of = (float)nbr_box(to, ny, i0, i1, j0, j1) / fa;
                const float d = pr - of;
                tf = wn * (d * d);
                tr = wn * (pr * pr + of * of);
            }
        }
        if (score) {   // the same in every thread
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                tf += __shfl_down(tf, d, 64);
                tr += __shfl_down(tr, d, 64);
            }
            if (lane == 0) {
                red[wave][2 * w] = tf;
                red[wave][2 * w + 1] = tr;
            }
        }
    }
    if (!score) return;
    __syncthreads();
    if (threadIdx.x < 2 * W) {   // word (scale, sum) of this workgroup: part[s][e][w][sum][workgroup]
        const int q = threadIdx.x;
        float* const part = p.workspace + nbr_table_words(p.starts, E, N);
        part[(((long)s * E + e) * 2 * W + q) * gridDim.x + blockIdx.x] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

// one wave per (start, event, scale, sum): blockIdx.x = ((s * E + e) * W + w) * 2 + sum
__global__ __launch_bounds__(64) void nbr_finish_kernel(const nlam_ens_neighbourhood_t p, int nblocks) {
    const int k = *p.lead;
    if (k >= p.max_lead) return;
    const int E = p.events, W = p.scales;
    const long o = blockIdx.x;
    const float* const src = p.workspace + nbr_table_words(p.starts, E, (long)p.nx * p.ny) + o * nblocks;
    float v = 0.f;
    for (int b = threadIdx.x; b < nblocks; b += 64) v += src[b];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if (threadIdx.x != 0) return;
    const long sew = o >> 1, se = sew / W, w = sew - se * W, s = se / E, e = se - s * E;
    float* const dst = (o & 1) ? p.fbs_ref : p.fbs;
    dst[((s * p.max_lead + k) * E + e) * W + w] = v;
}

// the size checks nlam_ens_neighbourhood and its workspace function share
int32_t nbr_sizes_check(long starts, long members, long nx, long ny, long nvars, long events, long scales) {
    if (starts < 1 || members < 1 || nx < 1 || ny < 1 || nvars < 1 || events < 1 || scales < 1) return NLAM_EINVAL;
    if (members > NLAM_ENS_MAX_MEMBERS || nvars > NLAM_EVAL_MAX_VARS || events > NLAM_ENS_MAX_EVENTS || scales > NLAM_NBR_MAX_SCALES ||
        starts > 65535)
        return NLAM_EUNSUP;
    if (nx > (1L << 24) || ny > (1L << 24) || members * nx * ny > (1L << 24)) return NLAM_EUNSUP;
    return 0;
}

// every check before any launch
int32_t ens_neighbourhood_check(const nlam_ens_neighbourhood_t* p) {
    if (p == nullptr || p->lead == nullptr || p->max_lead < 1) return NLAM_EINVAL;
    if (const int32_t rc = nbr_sizes_check(p->starts, p->members, p->nx, p->ny, p->d_state, p->events, p->scales)) return rc;
    if (p->prev == nullptr || p->row_weight == nullptr || p->event_var == nullptr || p->event_sense == nullptr || p->event_thr == nullptr ||
        p->radius == nullptr || p->nprob == nullptr || p->workspace == nullptr)
        return NLAM_EINVAL;
    if ((p->truth == nullptr) != (p->fbs == nullptr) || (p->truth == nullptr) != (p->fbs_ref == nullptr)) return NLAM_EINVAL;
    if (p->workspace_floats < nbr_ws_words(p->starts, p->events, p->scales, (long)p->nx * p->ny)) return NLAM_EINVAL;
    return 0;
}

}  // namespace

extern "C" {

int32_t nlam_ens_neighbourhood(const nlam_ens_neighbourhood_t* p, void* hip_stream) {
    NLAM_RANGE("nlam_ens_neighbourhood");
    if (const int32_t rc = ens_neighbourhood_check(p)) return rc;
    const int M = p->members, F = p->d_state, S = p->starts, E = p->events, W = p->scales, ny = p->ny;
    const long N = (long)p->nx * ny;
    const bool score = p->truth != nullptr;
    const hipStream_t stream = (hipStream_t)hip_stream;
    const int tn = nbr_tile_nodes(F, M);
    const size_t lds = ((size_t)(M + 1) * nbr_stride(tn, F) + kNbrTabWords) * sizeof(float);
    if (const int32_t rc = launch<nbr_count_kernel>(dim3(fc_nchunks((int)N, F), S), dim3(256), lds, stream, *p)) return rc;
    const long tables = 1 + (score ? 2L : 1L) * S * E;   // without the truth the O tables are neither written nor read
    const long rows = tables * p->nx, cols = tables * ny;
    const long row_blocks = (rows + 4 * (64 / nbr_row_lanes(ny)) - 1) / (4 * (64 / nbr_row_lanes(ny)));
    hipLaunchKernelGGL(nbr_rows_kernel, dim3((unsigned)std::min<long>(row_blocks, kNbrMaxBlocks)), dim3(256), 0, stream, *p, rows);
    if (const hipError_t e = hipGetLastError()) return (int32_t)e;   // nothing more is queued behind a launch that failed
    hipLaunchKernelGGL(nbr_cols_kernel, dim3((unsigned)std::min<long>((cols + 255) / 256, kNbrMaxBlocks)), dim3(256), 0, stream, *p, cols);
    if (const hipError_t e = hipGetLastError()) return (int32_t)e;
    const int nblocks = (int)nbr_blocks(N);
    hipLaunchKernelGGL(nbr_eval_kernel, dim3(nblocks, E, S), dim3(kNbrThreads), 0, stream, *p);
    if (const hipError_t e = hipGetLastError()) return (int32_t)e;
    if (score) hipLaunchKernelGGL(nbr_finish_kernel, dim3((unsigned)(2L * S * E * W)), dim3(64), 0, stream, *p, nblocks);
    return (int32_t)hipGetLastError();
}

int64_t nlam_ens_neighbourhood_workspace_floats(int32_t starts, int32_t members, int32_t nx, int32_t ny, int32_t nvars, int32_t events,
                                                int32_t scales) {
    if (const int32_t rc = nbr_sizes_check(starts, members, nx, ny, nvars, events, scales)) return rc;
    return nbr_ws_words(starts, events, scales, (long)nx * ny);
}

}  // extern "C"
