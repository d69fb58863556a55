// gt_match.hip -- ground-truth correspondences of a training pair (include/umereg_gt_matches.h): the reference's
// one_side_ball_query_matches / mutual_ball_query_matches (utils/general_utils.py:38-59), whose scipy KDTree build and
// query over up to ~1e5 points runs once per item of every batch when the trainer augments (kitti_dataset.py:460-509).
//
// The exact 1-NN of corr_knn.hip is the wrong tool here: fp32 distances (the KDTree's are fp64), no radius (a query outside
// the overlap grows its box until it covers the grid), no compacted row list, no mutual check.  This unit:
//
//   clean    copy the targets, replacing a point with a NaN / infinite / > 2^20 m coordinate by the origin and raising the
//            error flag (the grid build must never see such a point: its cell arithmetic would leave the table)
//   grid     launch_prep (grid.h) over the clean targets: cell-sorted {x, y, z, original index}
//   nn       8 lanes per query: transform in fp32 (stated order, uncontracted), cell range of [q - r, q + r] per axis, the
//            x-cells of a (z, y) row are ONE contiguous run of the sorted table, read 8 points (128 B) at a time; fp64
//            distance, lower index on a tie; three xor steps reduce the 8 lanes; the winner is kept iff d2 < r * r
//   mutual   (mutual form) drop i unless the reverse search maps its j* back to i
//   compact  rows (i, j*) in ascending i (compact.h)
//
// Work per query is the points of the cells its radius reaches, wherever the query lies; a query whose range misses the grid
// reads nothing.  fp64 use is 8 VALU operations per candidate on a gather-bound loop.
#include <float.h>

#include "compact.h"
#include "grid.h"
#include "umereg_gt_matches.h"

namespace umereg {

constexpr int kGtLanes = 8;                     // lanes that share a query
constexpr int kGtBlock = 256;
constexpr int kGtQPerBlock = kGtBlock / kGtLanes;
constexpr int kGtCompactBlock = 1024;
constexpr float kGtGridRadiusMin = 1.0e-2f;     // 2 * 2^20 m / (0.5 * this) cells per axis stays below 2^31 (load_grid_compute)
constexpr float kGtGridRadiusMax = 1.0e9f;
constexpr double kGtCellSlack = 1.0e-3;         // cells: the build's fp32 cell coordinate (< 64) is off by < 1e-5 of a cell

struct GtSideWs {
    size_t off_grid, off_clean, off_nn, total;
};

__host__ __device__ inline GtSideWs gt_side_ws(int n_q, int n_t)
{
    GtSideWs w;
    size_t o = 0;
    w.off_grid = o;  o += grid_ws(n_t).total;
    w.off_clean = o; o += ((size_t)n_t * 12 + 255) / 256 * 256;
    w.off_nn = o;    o += ((size_t)n_q * 4 + 255) / 256 * 256;
    w.total = o;
    return w;
}

struct GtWs {
    size_t off_side[2], off_bcnt, total;
    int n_blocks;
};

__host__ __device__ inline GtWs gt_ws(int n_src, int n_tgt, bool mutual)
{
    GtWs w;
    size_t o = 0;
    w.off_side[0] = o; o += gt_side_ws(n_src, n_tgt).total;
    w.off_side[1] = o; o += mutual ? gt_side_ws(n_tgt, n_src).total : 0;
    w.n_blocks = (n_src + kGtCompactBlock - 1) / kGtCompactBlock;
    w.off_bcnt = o;    o += ((size_t)w.n_blocks + 1) * 4;
    w.total = (o + 255) / 256 * 256;
    return w;
}

__device__ __forceinline__ bool gt_finite(float v) { return fabsf(v) <= FLT_MAX; }      // false for NaN and +-inf

// ---- targets -> a copy the grid build can take ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gt_clean_points_kernel(const float* __restrict__ pts, int n, float* __restrict__ out,
                                                              int* __restrict__ out_count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    const float lim = UMEREG_GT_MATCHES_MAX_COORD;
    if (!(fabsf(x) <= lim && fabsf(y) <= lim && fabsf(z) <= lim)) {      // (NaN / inf / out of range)
        out_count[1] = 1;                                                 // every writer stores the same word
        x = y = z = 0.f;
    }
    out[(size_t)i * 3] = x; out[(size_t)i * 3 + 1] = y; out[(size_t)i * 3 + 2] = z;
}

// cells of axis range [lo, hi] (in cell coordinates of the grid) clipped to [0, n - 1]; false: the range misses the grid
__device__ __forceinline__ bool gt_cell_range(double q, double r, float mn, float inv, int n, int& lo, int& hi)
{
    const double a = (q - r - (double)mn) * (double)inv - kGtCellSlack, b = (q + r - (double)mn) * (double)inv + kGtCellSlack;
    // (clamped in double first: a query 1e30 m away must not overflow the conversion)
    lo = (int)floor(fmin(fmax(a, -1.0), (double)n));
    hi = (int)floor(fmin(fmax(b, -1.0), (double)n));
    lo = lo < 0 ? 0 : lo;
    hi = hi > n - 1 ? n - 1 : hi;
    return lo <= hi;
}

// ---- nearest target within the radius, per query ---------------------------------------------------------------------
__global__ __launch_bounds__(kGtBlock) void gt_nn_kernel(const float* __restrict__ q_pts, int n_q, const float* __restrict__ T,
                                                         const char* __restrict__ gws, int n_t, double radius, double r2,
                                                         int* __restrict__ nn, int* __restrict__ out_count)
{
    const GridWs w = grid_ws(n_t);
    const float4* __restrict__ P4s = reinterpret_cast<const float4*>(gws + w.off_p4s);
    const int* __restrict__ start = reinterpret_cast<const int*>(gws + w.off_start);
    const Grid g = load_grid(reinterpret_cast<const unsigned int*>(gws + w.off_bbox), 0.f, n_t);
    const int i = blockIdx.x * kGtQPerBlock + (int)(threadIdx.x / kGtLanes);
    const int sub = threadIdx.x & (kGtLanes - 1);
    double best = DBL_MAX;
    int best_j = 0x7fffffff;
    if (i < n_q) {
        float x = q_pts[(size_t)i * 3], y = q_pts[(size_t)i * 3 + 1], z = q_pts[(size_t)i * 3 + 2];
        if (T) {
            // q = ((x * R[:,0] + y * R[:,1]) + z * R[:,2]) + t, every product and sum rounded on its own (-ffp-contract=off)
            float o[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float a = x * T[4 * k], b = y * T[4 * k + 1], c = z * T[4 * k + 2];
                const float ab = a + b;
                const float abc = ab + c;
                o[k] = abc + T[4 * k + 3];
            }
            x = o[0]; y = o[1]; z = o[2];
        }
        int x0, x1, y0, y1, z0, z1;
        if (!(gt_finite(x) && gt_finite(y) && gt_finite(z))) {
            out_count[1] = 1;
        } else if (gt_cell_range((double)x, radius, g.minx, g.invx, g.nx, x0, x1) &&
                   gt_cell_range((double)y, radius, g.miny, g.invy, g.ny, y0, y1) &&
                   gt_cell_range((double)z, radius, g.minz, g.invz, g.nz, z0, z1)) {
            const double qx = (double)x, qy = (double)y, qz = (double)z;
            for (int cz = z0; cz <= z1; ++cz) {
                for (int cy = y0; cy <= y1; ++cy) {
                    const int row = (cz * g.ny + cy) * g.nx;
                    const int k1 = start[row + x1 + 1];
                    for (int k = start[row + x0] + sub; k < k1; k += kGtLanes) {
                        const float4 p = P4s[k];
                        const double dx = qx - (double)p.x, dy = qy - (double)p.y, dz = qz - (double)p.z;
                        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                        const double xy = xx + yy;
                        const double d2 = xy + zz;
                        const int j = __float_as_int(p.w);
                        if (d2 < best || (d2 == best && j < best_j)) { best = d2; best_j = j; }
                    }
                }
            }
        }
    }
    // the 8 lanes of a query (aligned inside the wavefront): minimum of (d2, index), lexicographic
#pragma unroll
    for (int m = 1; m < kGtLanes; m <<= 1) {
        const double od = shfl_xor_f64(best, m);
        const int oj = __shfl_xor(best_j, m, kWave);
        if (od < best || (od == best && oj < best_j)) { best = od; best_j = oj; }
    }
    if (sub == 0 && i < n_q) nn[i] = (best_j != 0x7fffffff && best < r2) ? best_j : -1;
}

// keep i -> j only if the reverse search gives j -> i
__global__ __launch_bounds__(256) void gt_mutual_kernel(int* __restrict__ nn_st, const int* __restrict__ nn_ts, int n_s)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_s) return;
    const int j = nn_st[i];
    if (j >= 0 && nn_ts[j] != i) nn_st[i] = -1;
}

// compact.h's count (PASS 0) and scatter (PASS 1) over the matched queries: rows (i, nn[i])
template <int PASS>
__global__ __launch_bounds__(kGtCompactBlock) void gt_compact_kernel(const int* __restrict__ nn, int n, int* __restrict__ bcnt,
                                                                     int64_t* __restrict__ out_rows)
{
    const int i = blockIdx.x * kGtCompactBlock + threadIdx.x;
    const int j = i < n ? nn[i] : -1;
    const BlockRank k = block_rank<kGtCompactBlock>(j >= 0);
    if (PASS == 0) {
        if (threadIdx.x == 0) bcnt[blockIdx.x] = k.total;
    } else if (j >= 0) {
        const size_t r = (size_t)(bcnt[blockIdx.x] + k.before);
        out_rows[2 * r] = (int64_t)i;
        out_rows[2 * r + 1] = (int64_t)j;
    }
}

// block counts -> block offsets (in place), number of rows -> out_count[0]
__global__ __launch_bounds__(1024) void gt_scan_kernel(int n_blocks, int* __restrict__ bcnt, int* __restrict__ out_count)
{
    const int total = scan_counts<1024>(bcnt, bcnt, nullptr, n_blocks);
    if (threadIdx.x == 1023) out_count[0] = total;
}

// nn[i] of n_q queries against n_t targets, into the side's slice of the workspace
static int launch_side(const float* q, int n_q, const float* tgt, int n_t, const float* T, double radius, char* side, int* out_count,
                       hipStream_t st)
{
    const GtSideWs s = gt_side_ws(n_q, n_t);
    float* clean = reinterpret_cast<float*>(side + s.off_clean);
    hipLaunchKernelGGL(gt_clean_points_kernel, dim3((n_t + 255) / 256), dim3(256), 0, st, tgt, n_t, clean, out_count);
    UMEREG_CHECK_LAUNCH("gt_clean_points_kernel");
    // (the cell edge follows the radius where the cell budget allows; any edge is correct: the search takes its cell ranges from
    // the geometry the build stored)
    const float grid_r = fminf(fmaxf((float)radius, kGtGridRadiusMin), kGtGridRadiusMax);
    if (int rc = launch_prep(clean, side + s.off_grid, 1, n_t, grid_r, st)) return rc;
    hipLaunchKernelGGL(gt_nn_kernel, dim3((n_q + kGtQPerBlock - 1) / kGtQPerBlock), dim3(kGtBlock), 0, st, q, n_q, T,
                       (const char*)(side + s.off_grid), n_t, radius, radius * radius, reinterpret_cast<int*>(side + s.off_nn), out_count);
    UMEREG_CHECK_LAUNCH("gt_nn_kernel");
    return UMEREG_OK;
}

static int launch_rows(const int* nn, int n_src, int* bcnt, int n_blocks, int64_t* out_rows, int* out_count, hipStream_t st)
{
    hipLaunchKernelGGL(gt_compact_kernel<0>, dim3(n_blocks), dim3(kGtCompactBlock), 0, st, nn, n_src, bcnt, out_rows);
    UMEREG_CHECK_LAUNCH("gt_compact_kernel");
    hipLaunchKernelGGL(gt_scan_kernel, dim3(1), dim3(1024), 0, st, n_blocks, bcnt, out_count);
    UMEREG_CHECK_LAUNCH("gt_scan_kernel");
    hipLaunchKernelGGL(gt_compact_kernel<1>, dim3(n_blocks), dim3(kGtCompactBlock), 0, st, nn, n_src, bcnt, out_rows);
    UMEREG_CHECK_LAUNCH("gt_compact_kernel");
    return UMEREG_OK;
}

static int gt_matches(const char* who, const float* src, int n_src, const float* tgt, int n_tgt, const float* T, const float* T_inv,
                      bool mutual, double radius, int64_t* out_rows, int* out_count, void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(src && tgt && out_rows && out_count, "%s: null pointer", who);
    UMEREG_REQUIRE(n_src > 0 && n_tgt > 0, "%s: n_src, n_tgt must be positive (got %d, %d)", who, n_src, n_tgt);
    UMEREG_REQUIRE(radius > 0.0 && radius <= DBL_MAX, "%s: the radius must be positive and finite", who);
    if (int rc = check_device()) return rc;
    const GtWs w = gt_ws(n_src, n_tgt, mutual);
    UMEREG_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (int rc = launch_zero(out_count, 8, 1, 8, st)) return rc;
    if (int rc = launch_side(src, n_src, tgt, n_tgt, T, radius, ws + w.off_side[0], out_count, st)) return rc;
    int* nn = reinterpret_cast<int*>(ws + w.off_side[0] + gt_side_ws(n_src, n_tgt).off_nn);
    if (mutual) {
        if (int rc = launch_side(tgt, n_tgt, src, n_src, T_inv, radius, ws + w.off_side[1], out_count, st)) return rc;
        const int* nn_ts = reinterpret_cast<const int*>(ws + w.off_side[1] + gt_side_ws(n_tgt, n_src).off_nn);
        hipLaunchKernelGGL(gt_mutual_kernel, dim3((n_src + 255) / 256), dim3(256), 0, st, nn, nn_ts, n_src);
        UMEREG_CHECK_LAUNCH("gt_mutual_kernel");
    }
    return launch_rows(nn, n_src, reinterpret_cast<int*>(ws + w.off_bcnt), w.n_blocks, out_rows, out_count, st);
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_gt_matches_workspace_bytes(int n_src, int n_tgt, int mutual)
{
    return (n_src > 0 && n_tgt > 0) ? gt_ws(n_src, n_tgt, mutual != 0).total : 0;
}

UMEREG_API int umereg_gt_matches_one_side_f32(const float* src, int n_src, const float* tgt, int n_tgt, const float* T, double radius,
                                              int64_t* out_rows, int* out_count, void* workspace, size_t workspace_bytes, void* stream)
{
    return gt_matches("gt_matches_one_side", src, n_src, tgt, n_tgt, T, nullptr, false, radius, out_rows, out_count, workspace,
                      workspace_bytes, stream);
}

UMEREG_API int umereg_gt_matches_mutual_f32(const float* src, int n_src, const float* tgt, int n_tgt, const float* T, const float* T_inv,
                                            double radius, int64_t* out_rows, int* out_count, void* workspace, size_t workspace_bytes,
                                            void* stream)
{
    return gt_matches("gt_matches_mutual", src, n_src, tgt, n_tgt, T, T_inv, true, radius, out_rows, out_count, workspace, workspace_bytes,
                      stream);
}
