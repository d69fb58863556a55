// grid.hip -- the build of the uniform-grid search structure (grid.h) for gfx950: its kernels and the host launchers through
// which every user goes -- the ball query, the moment kernel and the a1-a5 pair chain, the kNN entries (corr_knn.hip), f1
// (corr.hip), the ICP (icp.hip) and the matcher's reset (match.hip).
//
// pytorch3d's kernel tests every point against every query (one thread per query, linear scan).
// Measured here, that scan was 263 of 346 us per KITTI-sized cloud, so the search is restructured
// around a uniform grid while keeping the result BIT-IDENTICAL to the linear scan:
//
//   prep    (5 tiny launches per cloud, all deterministic)
//           pack [N,3] -> {x,y,z,-} + bounding box (ordered-uint atomicMax) ;
//           cell id per point, per-workgroup LDS histograms ; exclusive scan over (cell, workgroup) ;
//           STABLE scatter into cell-sorted order {x,y,z,original index}.
//           Cell edge >= 1.0001 r, so a ball touches at most 3x3x3 cells, and because cells are
//           linearised x-fastest the three x-neighbours are ONE contiguous run: 9 runs per query.
// The search over the structure is ball_search.h; its two kernels are ball_query.hip (a1) and ume_moments.hip (a1+a2).
#include "grid.h"

namespace umereg {

// ---- K0: pack [N,3] -> [Npad] float4, and the bounding box -------------------------------------
// Few fat workgroups (grid-stride) so the bounding box costs ~6 atomics per workgroup: thousands of
// same-address atomics serialise at ~12 ns each and made this kernel 56 us in its first version.
constexpr int kPackWG = 1024;
constexpr int kPackMaxBlocks = 32;

__global__ __launch_bounds__(kPackWG) void pack_points_kernel(const float* __restrict__ pts, char* __restrict__ ws,
                                                              size_t ws_stride, int N, const PairDesc* __restrict__ desc)
{
    __shared__ unsigned int red[kPackWG / 64][6];
    const GridWs w = grid_ws(N);
    const int b = blockIdx.y;
    // (a ragged pair: cloud b where the caller left it, n_live <= N points of it; the table is padded to the capacity)
    const int n_live = desc ? desc->n_pts[b] : N;
    const UMEREG_GLOBAL_AS float* __restrict__ src = global_ptr(desc ? desc->pts[b] : pts + (size_t)b * N * 3);
    float4* out = reinterpret_cast<float4*>(ws + b * ws_stride + w.off_p4o);
    unsigned int* bbox = reinterpret_cast<unsigned int*>(ws + b * ws_stride + w.off_bbox);
    unsigned int e[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    for (int j = blockIdx.x * kPackWG + threadIdx.x; j < w.Npad; j += gridDim.x * kPackWG) {
        float4 v = make_float4(kFar, kFar, kFar, 0.f);
        if (j < n_live) {
            const UMEREG_GLOBAL_AS float* p = src + (size_t)j * 3;
            v = make_float4(p[0], p[1], p[2], 0.f);
            const unsigned int ex = enc_ord(v.x), ey = enc_ord(v.y), ez = enc_ord(v.z);
            e[0] = max(e[0], ~ex); e[1] = max(e[1], ~ey); e[2] = max(e[2], ~ez);
            e[3] = max(e[3], ex);  e[4] = max(e[4], ey);  e[5] = max(e[5], ez);
        }
        out[j] = v;
    }
    if (desc && desc->kp[b]) {
        // a ragged pair's keypoint indices, int64 lists wherever the caller keeps them -> int32 at a fixed place of the workspace (n_kp <=
        // Npad: the pair chain checks).  Anything outside int32 becomes -1: "outside the cloud", which the moment kernel answers with NaN.
        const UMEREG_GLOBAL_AS int64_t* __restrict__ kp = global_ptr(desc->kp[b]);
        int* __restrict__ kpi = reinterpret_cast<int*>(ws + b * ws_stride + w.off_kpi);
        const int n_kp = desc->n_kp < w.Npad ? desc->n_kp : w.Npad;
        for (int k = blockIdx.x * kPackWG + threadIdx.x; k < n_kp; k += gridDim.x * kPackWG) {
            const int64_t i = kp[k];
            kpi[k] = (i < 0 || i > 0x7fffffffLL) ? -1 : (int)i;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned int o = __shfl_xor(e[k], m, kWave);
            e[k] = o > e[k] ? o : e[k];
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[threadIdx.x >> 6][k] = e[k];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned int v = 0u;
        for (int wv = 0; wv < kPackWG / 64; ++wv) v = max(v, red[wv][threadIdx.x]);
        atomicMax(bbox + threadIdx.x, v);   // max is order-independent: deterministic
    }
}

// ---- K1: cell ids + per-workgroup histograms --------------------------------------------------
// order_only (a bit per batch element; -1 = all) set: the structure will only be used as a PROCESSING ORDER (corr.hip: the source cloud of the correlation
// scores), never searched.  Single-layer grids then sort by the cell's position along the Hilbert curve instead of the
// row-major cell id: 64 consecutive points of the sorted table form a compact blob (~8 m x 8 m on a KITTI cloud) instead of a
// strip one cell wide and ~40 m long, which is what makes "a chunk of 64 slots" a neighbourhood (per-chunk hypothesis orders,
// per-record candidate sets).  The start[] table of such a structure is indexed by curve position and of no use to a search.
__device__ __forceinline__ int hilbert64(int x, int y)
{
    // position of cell (x, y), 0 <= x, y < 64, along the Hilbert curve of the 64 x 64 grid: consecutive positions are always
    // edge-adjacent cells (a Morton code jumps across the grid at every quadrant boundary)
    int d = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int rx = (x & s) ? 1 : 0, ry = (y & s) ? 1 : 0;
        d += s * s * ((3 * rx) ^ ry);
        if (ry == 0) {
            if (rx == 1) { x = 63 - x; y = 63 - y; }
            const int t = x; x = y; y = t;
        }
    }
    return d;
}

__global__ __launch_bounds__(kSortWG) void grid_hist_kernel(char* __restrict__ ws, size_t ws_stride, int N,
                                                            float radius, int order_only, const PairDesc* __restrict__ desc)
{
    __shared__ int hist[kMaxCells];
    __shared__ Grid g_sh;
    const GridWs w = grid_ws(N);
    char* wb = ws + blockIdx.y * ws_stride;
    const float4* P4o = reinterpret_cast<const float4*>(wb + w.off_p4o);
    int* cell_of = reinterpret_cast<int*>(wb + w.off_cell);
    int* counts = reinterpret_cast<int*>(wb + w.off_counts) + (size_t)blockIdx.x * kMaxCells;
    // (the geometry -- divisions and, in kNN mode, the cell-edge search loop -- by the first wavefront only: sixteen wavefronts doing
    // it side by side share four SIMDs)
    if (threadIdx.x < 64) {
        const Grid g0 = load_grid_compute(reinterpret_cast<const unsigned int*>(wb + w.off_bbox), radius, desc ? desc->n_pts[blockIdx.y] : N);
        if (threadIdx.x == 0) g_sh = g0;
    }
    for (int c = threadIdx.x; c < kMaxCells; c += kSortWG) hist[c] = 0;
    __syncthreads();
    const Grid g = g_sh;
    const int j = blockIdx.x * kSortWG + threadIdx.x;
    if (j < (desc ? desc->n_pts[blockIdx.y] : N)) {
        const float4 p = P4o[j];
        int c = (cell_axis(p.z, g.minz, g.invz, g.nz) * g.ny + cell_axis(p.y, g.miny, g.invy, g.ny)) * g.nx +
                cell_axis(p.x, g.minx, g.invx, g.nx);
        if (((order_only >> blockIdx.y) & 1) && g.nz == 1 && g.nx <= 64 && g.ny <= 64)          // (positions < 64 * 64 = kMaxCells)
            c = hilbert64(cell_axis(p.x, g.minx, g.invx, g.nx), cell_axis(p.y, g.miny, g.invy, g.ny));
        cell_of[j] = c;
        atomicAdd(&hist[c], 1);   // integer counts: order-independent
    }
    __syncthreads();
    for (int c = threadIdx.x; c < kMaxCells; c += kSortWG) counts[c] = hist[c];
}

// ---- K2: exclusive scan over (cell, workgroup): bases[wg][c] = first slot of (wg, c) within cell c --
// kScanWGs workgroups of 256 lanes, one lane per cell: the lane walks its cell's column of the per-workgroup counts (independent
// loads, sixteen in flight) and leaves the cell's total in tot[]; the scan of the 4 096 totals is done by every workgroup of the
// scatter kernel for itself (16 KiB read, two barriers: cheaper than a launch, and than a last-workgroup-done hand-over -- an
// agent-scope fence writes the XCD's L2 back on this part).  (One workgroup did all of it in round 2: 3 MB through one CU for a
// 50 000-point cloud, 22 us.)
constexpr int kScanWGs = kMaxCells / 256;
__global__ __launch_bounds__(256) void grid_scan_kernel(char* __restrict__ ws, size_t ws_stride, int N, float radius, int order_only,
                                                        const PairDesc* __restrict__ desc)
{
    const GridWs w = grid_ws(N);
    char* wb = ws + blockIdx.y * ws_stride;
    const int* __restrict__ counts = reinterpret_cast<const int*>(wb + w.off_counts);
    int* __restrict__ bases = reinterpret_cast<int*>(wb + w.off_bases);
    int* __restrict__ tot = reinterpret_cast<int*>(wb + w.off_tot);
    unsigned int* bbox = reinterpret_cast<unsigned int*>(wb + w.off_bbox);
    const Grid gg = load_grid_compute(bbox, radius, desc ? desc->n_pts[blockIdx.y] : N);      // (the density of the LIVE points, kNN mode)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        store_grid(bbox, gg);     // for every later kernel
        if (desc) {
            // a ragged pair: what the moment kernel needs of the record -- the cloud's size and its feature table -- beside the geometry, in
            // the 64 bytes every wavefront of that kernel loads anyway (a load THROUGH the record at the head of every wavefront: +2.6 us per pair)
            const unsigned long long fp = (unsigned long long)desc->feat[blockIdx.y];
            bbox[6] = (unsigned int)fp; bbox[7] = (unsigned int)(fp >> 32);
            bbox[15] = (unsigned int)desc->n_pts[blockIdx.y];
        }
    }
    // cells beyond this are never populated (curve positions of an order-only structure: any of the 4096)
    const int n_cells = ((order_only >> blockIdx.y) & 1) ? kMaxCells : gg.nx * gg.ny * gg.nz;
    const int c = blockIdx.x * 256 + threadIdx.x;
    int run = 0;
    if (c < n_cells) {
        int g = 0;
        for (; g + 16 <= w.n_wg; g += 16) {                  // (a round trip per batch: 16 in flight, 4 batches for a 50 000-point cloud)
            int t[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) t[u] = counts[(size_t)(g + u) * kMaxCells + c];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                bases[(size_t)(g + u) * kMaxCells + c] = run;
                run += t[u];
            }
        }
        for (; g + 4 <= w.n_wg; g += 4) {
            int t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = counts[(size_t)(g + u) * kMaxCells + c];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bases[(size_t)(g + u) * kMaxCells + c] = run;
                run += t[u];
            }
        }
        for (; g < w.n_wg; ++g) {
            const int t = counts[(size_t)g * kMaxCells + c];
            bases[(size_t)g * kMaxCells + c] = run;
            run += t;
        }
    }
    tot[c] = run;
}

// ---- K3: stable scatter into cell-sorted order ------------------------------------------------
__global__ __launch_bounds__(kSortWG) void grid_scatter_kernel(char* __restrict__ ws, size_t ws_stride, int N,
                                                               const PairDesc* __restrict__ desc)
{
    __shared__ int slot[kMaxCells];
    __shared__ int part[kSortWG / 64];
    __shared__ uint4 wcnt[kMaxCells];                  // [cell][wavefront] point counts, a byte each (64 KiB)
    static_assert(kSortWG / 64 == 16, "16 wavefronts: one 16-byte row per cell");
    const GridWs w = grid_ws(N);
    char* wb = ws + blockIdx.y * ws_stride;
    const float4* P4o = reinterpret_cast<const float4*>(wb + w.off_p4o);
    float4* P4s = reinterpret_cast<float4*>(wb + w.off_p4s);
#pragma unroll
    for (int k = 0; k < kMaxCells / kSortWG; ++k) wcnt[k * kSortWG + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    const int* cell_of = reinterpret_cast<const int*>(wb + w.off_cell);
    const int* bases = reinterpret_cast<const int*>(wb + w.off_bases) + (size_t)blockIdx.x * kMaxCells;
    int* start = reinterpret_cast<int*>(wb + w.off_start);
    {
        // exclusive scan of the cells' totals (see grid_scan_kernel): kMaxCells / kSortWG = 4 consecutive cells per lane; workgroup 0
        // leaves start[] for the kernels that search the structure
        static_assert(kMaxCells == 4 * kSortWG, "4 cells per lane");
        const int4 t = reinterpret_cast<const int4*>(wb + w.off_tot)[threadIdx.x];
        const int4 bs = reinterpret_cast<const int4*>(bases)[threadIdx.x];
        const int sum = t.x + t.y + t.z + t.w;
        int incl = sum;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int o = __shfl_up(incl, m, kWave);
            if ((int)(threadIdx.x & 63) >= m) incl += o;
        }
        if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = incl;
        __syncthreads();
        int base = 0;
        for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) base += part[k];
        const int e0 = base + incl - sum, e1 = e0 + t.x, e2 = e1 + t.y, e3 = e2 + t.z;
        const int c0 = threadIdx.x * 4;
        slot[c0] = e0 + bs.x; slot[c0 + 1] = e1 + bs.y; slot[c0 + 2] = e2 + bs.z; slot[c0 + 3] = e3 + bs.w;
        if (blockIdx.x == 0) {
            reinterpret_cast<int4*>(start)[threadIdx.x] = make_int4(e0, e1, e2, e3);
            if (threadIdx.x == kSortWG - 1) start[kMaxCells] = e3 + t.w;
        }
    }
    __syncthreads();
    const int j = blockIdx.x * kSortWG + threadIdx.x;
    const int n_live = desc ? desc->n_pts[blockIdx.y] : N;
    const bool valid = j < n_live;
    const int c = valid ? cell_of[j] : -1;
    const int wave = threadIdx.x >> 6;
    // rank among the lanes of this wave with the same cell and a lower index
    int rank = 0, n_same = 0;
    {
        unsigned long long todo = __ballot(valid);
        while (todo != 0ull) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lc = __builtin_amdgcn_readlane(c, leader);            // (the leader is wave-uniform: a register read, not a trip through LDS)
            const unsigned long long same = __ballot(valid && c == lc);
            if (c == lc) { rank = mbcnt(same); n_same = __popcll(same); }
            todo &= ~same;
        }
    }
    // A point's place = the cell's first slot for this workgroup + the points of the same cell in EARLIER wavefronts + its rank in its own:
    // every wavefront publishes its per-cell counts as one byte of the cell's 16-byte row (a wavefront holds <= 64 points of a cell), one
    // barrier, and a lane adds up the bytes before its wavefront's.  (Until round 3 the sixteen wavefronts took turns on slot[], two
    // barriers a turn: 15 us for what is 7 now.)
    float4 p = P4o[valid ? j : 0];
    p.w = __int_as_float(j);
    if (valid && rank == 0) reinterpret_cast<unsigned char*>(wcnt)[c * 16 + wave] = (unsigned char)n_same;
    __syncthreads();
    if (valid) {
        const uint4 w4 = wcnt[c];
        const unsigned int words[4] = {w4.x, w4.y, w4.z, w4.w};
        unsigned int base = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int nb = min(max(wave - 4 * i, 0), 4);                       // bytes of this word that belong to earlier wavefronts
            const unsigned int mask = nb >= 4 ? 0xffffffffu : ((1u << (8 * nb)) - 1u);
            base = __builtin_amdgcn_sad_u8(words[i] & mask, 0u, base);
        }
        P4s[slot[c] + (int)base + rank] = p;
    }
    // tail padding of the sorted table (read, never accepted, by the last chunk of the last run)
    if (blockIdx.x == 0 && threadIdx.x < 64)
        P4s[n_live + threadIdx.x] = make_float4(kFar, kFar, kFar, __int_as_float(0x7fffffff));
}

// ---- keypoint processing order ---------------------------------------------------------------------
// Keypoints arrive in random order (np.random.choice), so consecutive wavefronts gather from all over
// the 6.4 MB feature table: every XCD's 4 MiB L2 sees the whole table (measured: 58 % L2 hits,
// 226 MB of fabric traffic per launch for 8 MB of unique data).  Sorting the keypoints by grid cell
// and giving each XCD one contiguous slab of that order (workgroup b runs on XCD b % 8) shrinks an
// XCD's working set to its slab plus a one-cell halo, and makes the 4 waves of a workgroup walk the
// same runs (L1 hits).  Only the ORDER in which keypoints are processed changes -- each keypoint's
// result is independent of it -- so this pass may use atomics freely.
__global__ __launch_bounds__(1024) void kp_order_kernel(char* __restrict__ ws, size_t ws_stride,
                                                         const float* __restrict__ kpts,
                                                         const int64_t* __restrict__ kp_index, int N, int n_kp,
                                                         float radius, const PairDesc* __restrict__ desc)
{
    __shared__ int cnt[kMaxCells];
    __shared__ int part[1024 / 64];
    const GridWs w = grid_ws(N);
    char* wb = ws + blockIdx.y * ws_stride;
    const int b = blockIdx.y;
    const float4* P4o = reinterpret_cast<const float4*>(wb + w.off_p4o);
    int* perm = reinterpret_cast<int*>(wb + w.off_kperm);
    const Grid g = load_grid(reinterpret_cast<const unsigned int*>(wb + w.off_bbox), radius, N);
    const int* cell_of = reinterpret_cast<const int*>(wb + w.off_cell);
    for (int c = threadIdx.x; c < kMaxCells; c += 1024) cnt[c] = 0;
    __syncthreads();
    const int n_live = desc ? desc->n_pts[b] : N;
    const int64_t* __restrict__ kpi = kp_index ? kp_index + (size_t)b * n_kp : nullptr;
    const int* __restrict__ kpi32 = reinterpret_cast<const int*>(wb + w.off_kpi);       // (a ragged pair's, written by pack_points_kernel)
    auto cell_of_kp = [&](int k) {
        if (desc || kpi) {   // the point's cell, from the hist pass (an out-of-range index only affects the ORDER here: clamped)
            const int64_t i = desc ? (int64_t)kpi32[k] : kpi[k];
            return cell_of[i < 0 ? 0 : (i >= n_live ? n_live - 1 : i)];
        }
        const float* q = kpts + ((size_t)b * n_kp + k) * 3;
        return (cell_axis(q[2], g.minz, g.invz, g.nz) * g.ny + cell_axis(q[1], g.miny, g.invy, g.ny)) * g.nx +
               cell_axis(q[0], g.minx, g.invx, g.nx);
    };
    // each thread's cells are kept in registers between the count pass and the scatter pass
    constexpr int kKeep = 16;
    int mine[kKeep];
#pragma unroll
    for (int u = 0; u < kKeep; ++u) {
        const int k = threadIdx.x + u * 1024;
        mine[u] = k < n_kp ? cell_of_kp(k) : -1;
    }
#pragma unroll
    for (int u = 0; u < kKeep; ++u)
        if (mine[u] >= 0) atomicAdd(&cnt[mine[u]], 1);
    for (int k = threadIdx.x + kKeep * 1024; k < n_kp; k += 1024) atomicAdd(&cnt[cell_of_kp(k)], 1);
    __syncthreads();
    // exclusive scan of cnt[0..4096): 4 consecutive cells per thread
    const int c0 = threadIdx.x * 4;
    const int t0 = cnt[c0], t1 = cnt[c0 + 1], t2 = cnt[c0 + 2], t3 = cnt[c0 + 3];
    const int sum = t0 + t1 + t2 + t3;
    int incl = sum;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_up(incl, m, kWave);
        if ((int)(threadIdx.x & 63) >= m) incl += o;
    }
    if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) base += part[k];
    const int excl = base + incl - sum;
    __syncthreads();
    cnt[c0] = excl; cnt[c0 + 1] = excl + t0; cnt[c0 + 2] = excl + t0 + t1; cnt[c0 + 3] = excl + t0 + t1 + t2;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kKeep; ++u)
        if (mine[u] >= 0) perm[atomicAdd(&cnt[mine[u]], 1)] = threadIdx.x + u * 1024;
    for (int k = threadIdx.x + kKeep * 1024; k < n_kp; k += 1024) perm[atomicAdd(&cnt[cell_of_kp(k)], 1)] = k;
}

// ---- zeroing, and the host launchers ---------------------------------------------------------------
__global__ __launch_bounds__(256) void zero_words_kernel(unsigned int* __restrict__ p, unsigned int words_per_row, size_t stride_words)
{
    unsigned int* row = p + blockIdx.y * stride_words;
    for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < words_per_row; i += gridDim.x * 256u) row[i] = 0u;
}

int launch_zero(void* p, size_t row_bytes, int rows, size_t stride, hipStream_t st)
{
    if (row_bytes == 0 || rows <= 0) return UMEREG_OK;
    const unsigned int words = (unsigned int)(row_bytes / 4);
    unsigned int nb = (words + 255u) / 256u;
    nb = nb > 256u ? 256u : nb;
    hipLaunchKernelGGL(zero_words_kernel, dim3(nb, rows), dim3(256), 0, st, (unsigned int*)p, words, stride / 4);
    UMEREG_CHECK_LAUNCH("zero_words_kernel");
    return UMEREG_OK;
}

int launch_prep(const float* pts, char* ws, int B, int N, float radius, hipStream_t st, int order_only, const PairDesc* desc)
{
    const GridWs w = grid_ws(N);
    // the B bounding-box records (64 B each, one per cloud's workspace slice) in one call
    if (int rc = launch_zero(ws + w.off_bbox, 64, B, w.total, st)) return rc;
    {
        int nb = (w.Npad + kPackWG - 1) / kPackWG;
        nb = nb > kPackMaxBlocks ? kPackMaxBlocks : nb;
        hipLaunchKernelGGL(pack_points_kernel, dim3(nb, B), dim3(kPackWG), 0, st, pts, ws, w.total, N, desc);
    }
    UMEREG_CHECK_LAUNCH("pack_points_kernel");
    hipLaunchKernelGGL(grid_hist_kernel, dim3(w.n_wg, B), dim3(kSortWG), 0, st, ws, w.total, N, radius, order_only, desc);
    UMEREG_CHECK_LAUNCH("grid_hist_kernel");
    hipLaunchKernelGGL(grid_scan_kernel, dim3(kScanWGs, B), dim3(256), 0, st, ws, w.total, N, radius, order_only, desc);
    UMEREG_CHECK_LAUNCH("grid_scan_kernel");
    hipLaunchKernelGGL(grid_scatter_kernel, dim3(w.n_wg, B), dim3(kSortWG), 0, st, ws, w.total, N, desc);
    UMEREG_CHECK_LAUNCH("grid_scatter_kernel");
    return UMEREG_OK;
}

int launch_query_order(char* ws, const float* kpts, const int64_t* kp_index, int B, int N, int n_q, float radius,
                       hipStream_t st, const PairDesc* desc)
{
    hipLaunchKernelGGL(kp_order_kernel, dim3(1, B), dim3(1024), 0, st, ws, grid_ws(N).total, kpts, kp_index, N, n_q, radius, desc);
    UMEREG_CHECK_LAUNCH("kp_order_kernel");
    return UMEREG_OK;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_ball_query_workspace_bytes(int B, int n2)
{
    if (B <= 0 || n2 <= 0) return 0;
    return (size_t)B * grid_ws(n2).total;
}

UMEREG_API size_t umereg_ume_moments_workspace_bytes(int B, int N)
{
    return umereg_ball_query_workspace_bytes(B, N);
}

UMEREG_API int umereg_pack_points_f32(const float* pts, int B, int N, float radius, void* packed,
                                      size_t packed_bytes, void* stream)
{
    UMEREG_REQUIRE(pts && packed, "pack_points: null pointer");
    UMEREG_REQUIRE(B > 0 && N > 0, "pack_points: B, N must be positive (got %d, %d)", B, N);
    UMEREG_REQUIRE(radius > 0.f, "pack_points: radius must be positive");
    if (int rc = check_device()) return rc;
    if (packed_bytes < umereg_ume_moments_workspace_bytes(B, N) || ((uintptr_t)packed & 15)) {
        set_error("pack_points: packed buffer too small or misaligned (%zu < %zu)", packed_bytes,
                  umereg_ume_moments_workspace_bytes(B, N));
        return UMEREG_EWORKSPACE;
    }
    return launch_prep(pts, (char*)packed, B, N, radius, (hipStream_t)stream);
}

UMEREG_API int umereg_ume_keypoint_order(void* packed, const float* kpts, const int64_t* kp_index, int B, int N,
                                         int n_kp, float radius, void* stream)
{
    UMEREG_REQUIRE(packed && (kpts || kp_index), "keypoint_order: null pointer");
    UMEREG_REQUIRE(B > 0 && N > 0 && n_kp > 0, "keypoint_order: B, N, n_kp must be positive");
    UMEREG_REQUIRE(n_kp <= grid_ws(N).Npad, "keypoint_order: n_kp (%d) exceeds the order buffer (%d)", n_kp, grid_ws(N).Npad);
    if (int rc = check_device()) return rc;
    return launch_query_order((char*)packed, kpts, kp_index, B, N, n_kp, radius, (hipStream_t)stream);
}
