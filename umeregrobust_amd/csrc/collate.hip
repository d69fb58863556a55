// collate.hip -- one batch element of the device-side collate (include/umereg_collate.h): the reference's batch_collate_fn_dset
// (datasets/kitti/kitti_dataset.py:546-616) after its two host draws -- the index gathers of both clouds straight into the element's
// slices of the batched tensors, and the correspondences that survive the dilution (the two np.intersect1d calls, :585-589).
//
//   init     position tables of both clouds = -1, the two minimum tables = INT_MAX, out_count = {0, 0}
//   gather   one thread per kept point of either cloud: position[keep[j]] = j, and the point's fields copied to row j of the outputs
//            (keep[j] is read coalesced; the 12-byte rows and 8-byte labels behind it are scattered scalar loads, the stores are
//            contiguous over the lanes); coordinates come out as {b, x, y, z}
//   first    first_row[s] = min row index over the rows of `matches` that name source s            (integer atomicMin)
//   lowest   rows that ARE their source's first row and whose source survived: first_src[t] = min s  (integer atomicMin)
//   compact  targets with a candidate that survived themselves, in ascending target index (compact.h)
//
// The two minima do not depend on the order in which the atomics land; the row order comes from the scan.  This is launch-bound,
// bandwidth-trivial work (a few hundred KB per element): seven short launches per element and no more machinery than that.
#include <limits.h>

#include "compact.h"
#include "umereg_collate.h"

namespace umereg {

constexpr int kCollateBlock = 256;
constexpr int kCollateCompactBlock = 1024;
constexpr int64_t kCollateMaxN = (int64_t)1 << 31;      // indices are int32 inside

struct CollateWs {
    size_t off_pos_src, off_pos_tgt, off_first_row, off_first_src, off_bcnt, total;
    int n_blocks;
};

__host__ __device__ inline CollateWs collate_ws(int ns, int nt)
{
    CollateWs w;
    size_t o = 0;
    w.off_pos_src = o;   o += ((size_t)ns * 4 + 255) / 256 * 256;
    w.off_pos_tgt = o;   o += ((size_t)nt * 4 + 255) / 256 * 256;
    w.off_first_row = o; o += ((size_t)ns * 4 + 255) / 256 * 256;
    w.off_first_src = o; o += ((size_t)nt * 4 + 255) / 256 * 256;
    w.n_blocks = (int)(((int64_t)nt + kCollateCompactBlock - 1) / kCollateCompactBlock);      // (int64: nt may be 2^31 - 1)
    w.off_bcnt = o;      o += ((size_t)w.n_blocks + 1) * 4;
    w.total = (o + 255) / 256 * 256;
    return w;
}

struct CollateSide {
    const float* pts;
    const int64_t* seg;
    const int32_t* coords;
    const float* moved;         // the transformed points (source only)
    const int64_t* keep;
    float* out_pts;
    int64_t* out_seg;
    int32_t* out_coords;
    float* out_moved;
    int* pos;
    int n_all, n_keep;
};

__global__ __launch_bounds__(kCollateBlock) void collate_init_kernel(int* __restrict__ pos_src, int* __restrict__ first_row, int ns,
                                                                      int* __restrict__ pos_tgt, int* __restrict__ first_src, int nt,
                                                                      int* __restrict__ out_count)
{
    const int64_t i = (int64_t)blockIdx.x * kCollateBlock + threadIdx.x;
    if (i < ns) { pos_src[i] = -1; first_row[i] = INT_MAX; }
    if (i < nt) { pos_tgt[i] = -1; first_src[i] = INT_MAX; }
    if (i < 2) out_count[i] = 0;
}

// blocks [0, src_blocks) serve the source, the others the target
__global__ __launch_bounds__(kCollateBlock) void collate_gather_kernel(CollateSide src, CollateSide tgt, int src_blocks, int b,
                                                                        int* __restrict__ out_count)
{
    const bool is_src = (int)blockIdx.x < src_blocks;
    const CollateSide s = is_src ? src : tgt;                             // (uniform over the block: scalar selects)
    const int64_t j = (int64_t)(blockIdx.x - (is_src ? 0 : src_blocks)) * kCollateBlock + threadIdx.x;
    if (j >= s.n_keep) return;
    const int64_t k = s.keep[j];
    if (k < 0 || k >= s.n_all) {
        out_count[1] = 1;                                                 // every writer stores the same word
        return;
    }
    s.pos[k] = (int)j;
    if (s.pts) {
        const float x = s.pts[3 * k], y = s.pts[3 * k + 1], z = s.pts[3 * k + 2];
        s.out_pts[3 * j] = x; s.out_pts[3 * j + 1] = y; s.out_pts[3 * j + 2] = z;
    }
    if (s.seg) s.out_seg[j] = s.seg[k];
    if (s.coords) {
        const int32_t x = s.coords[3 * k], y = s.coords[3 * k + 1], z = s.coords[3 * k + 2];
        s.out_coords[4 * j] = b; s.out_coords[4 * j + 1] = x; s.out_coords[4 * j + 2] = y; s.out_coords[4 * j + 3] = z;
    }
    if (s.moved) {
        const float x = s.moved[3 * k], y = s.moved[3 * k + 1], z = s.moved[3 * k + 2];
        s.out_moved[3 * j] = x; s.out_moved[3 * j + 1] = y; s.out_moved[3 * j + 2] = z;
    }
}

// a source point keeps the first of its rows
__global__ __launch_bounds__(kCollateBlock) void collate_first_row_kernel(const int64_t* __restrict__ matches, int m, int ns, int nt,
                                                                           int* __restrict__ first_row, int* __restrict__ out_count)
{
    const int64_t r = (int64_t)blockIdx.x * kCollateBlock + threadIdx.x;
    if (r >= m) return;
    const int64_t s = matches[2 * r], t = matches[2 * r + 1];
    if (s < 0 || s >= ns || t < 0 || t >= nt) {
        out_count[1] = 1;
        return;
    }
    atomicMin(&first_row[s], (int)r);
}

// of the first rows whose source survived, a target keeps the one with the lowest source index
__global__ __launch_bounds__(kCollateBlock) void collate_first_src_kernel(const int64_t* __restrict__ matches, int m, int ns, int nt,
                                                                           const int* __restrict__ first_row,
                                                                           const int* __restrict__ pos_src, int* __restrict__ first_src)
{
    const int64_t r = (int64_t)blockIdx.x * kCollateBlock + threadIdx.x;
    if (r >= m) return;
    const int64_t s = matches[2 * r], t = matches[2 * r + 1];
    if (s < 0 || s >= ns || t < 0 || t >= nt) return;
    if (first_row[s] == (int)r && pos_src[s] >= 0) atomicMin(&first_src[t], (int)s);
}

// compact.h's count (PASS 0) and scatter (PASS 1) over the targets that kept a candidate and survived themselves
template <int PASS>
__global__ __launch_bounds__(kCollateCompactBlock) void collate_compact_kernel(const int* __restrict__ first_src,
                                                                                const int* __restrict__ pos_src,
                                                                                const int* __restrict__ pos_tgt, int nt,
                                                                                int* __restrict__ bcnt, int64_t* __restrict__ out_rows)
{
    const int64_t t = (int64_t)blockIdx.x * kCollateCompactBlock + threadIdx.x;
    int s = INT_MAX, pt = -1;
    if (t < nt) { s = first_src[t]; pt = pos_tgt[t]; }
    const bool keep = s != INT_MAX && pt >= 0;
    const BlockRank k = block_rank<kCollateCompactBlock>(keep);
    if (PASS == 0) {
        if (threadIdx.x == 0) bcnt[blockIdx.x] = k.total;
    } else if (keep) {
        const size_t r = (size_t)(bcnt[blockIdx.x] + k.before);
        out_rows[2 * r] = (int64_t)pos_src[s];
        out_rows[2 * r + 1] = (int64_t)pt;
    }
}

// block counts -> block offsets (in place), number of rows -> out_count[0]
__global__ __launch_bounds__(1024) void collate_scan_kernel(int n_blocks, int* __restrict__ bcnt, int* __restrict__ out_count)
{
    const int total = scan_counts<1024>(bcnt, bcnt, nullptr, n_blocks);
    if (threadIdx.x == 1023) out_count[0] = total;
}

static bool collate_sizes_ok(int64_t ns, int64_t nt, int64_t m)
{
    return ns > 0 && ns < kCollateMaxN && nt > 0 && nt < kCollateMaxN && m >= 0 && m < kCollateMaxN;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_collate_workspace_bytes(int64_t ns, int64_t nt, int64_t n_matches)
{
    return collate_sizes_ok(ns, nt, n_matches) ? collate_ws((int)ns, (int)nt).total : 0;
}

UMEREG_API int umereg_collate_element(const float* src_pts, const int64_t* src_seg, const int32_t* src_coords, const float* src_pts_tform,
                                      int64_t ns, const float* tgt_pts, const int64_t* tgt_seg, const int32_t* tgt_coords, int64_t nt,
                                      const int64_t* matches, int64_t n_matches, const int64_t* keep_src, int64_t n_src,
                                      const int64_t* keep_tgt, int64_t n_tgt, int b, float* out_src_pts, int64_t* out_src_seg,
                                      int32_t* out_src_coords, float* out_src_pts_tform, float* out_tgt_pts, int64_t* out_tgt_seg,
                                      int32_t* out_tgt_coords, int64_t* out_matches, int* out_count, void* workspace,
                                      size_t workspace_bytes, void* stream)
{
    const char* who = "collate_element";
    UMEREG_REQUIRE(collate_sizes_ok(ns, nt, n_matches),
                   "%s: cloud sizes must lie in [1, 2^31) and the number of matches in [0, 2^31) (got %lld, %lld, %lld)", who,
                   (long long)ns, (long long)nt, (long long)n_matches);
    UMEREG_REQUIRE(n_src > 0 && n_src <= ns && n_tgt > 0 && n_tgt <= nt, "%s: keep sizes must lie in [1, cloud size] (got %lld of %lld, %lld of %lld)",
                   who, (long long)n_src, (long long)ns, (long long)n_tgt, (long long)nt);
    UMEREG_REQUIRE(b >= 0, "%s: the batch index must not be negative (got %d)", who, b);
    UMEREG_REQUIRE(keep_src && keep_tgt && out_count, "%s: null pointer (keep lists, out_count)", who);
    UMEREG_REQUIRE(n_matches == 0 || (matches && out_matches), "%s: null pointer (matches, out_matches)", who);
    UMEREG_REQUIRE(!src_pts == !out_src_pts && !src_seg == !out_src_seg && !src_coords == !out_src_coords &&
                       !src_pts_tform == !out_src_pts_tform && !tgt_pts == !out_tgt_pts && !tgt_seg == !out_tgt_seg &&
                       !tgt_coords == !out_tgt_coords,
                   "%s: a field needs both its input and its output pointer, or neither", who);
    if (int rc = check_device()) return rc;
    const CollateWs w = collate_ws((int)ns, (int)nt);
    UMEREG_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* pos_src = reinterpret_cast<int*>(ws + w.off_pos_src);
    int* pos_tgt = reinterpret_cast<int*>(ws + w.off_pos_tgt);
    int* first_row = reinterpret_cast<int*>(ws + w.off_first_row);
    int* first_src = reinterpret_cast<int*>(ws + w.off_first_src);
    int* bcnt = reinterpret_cast<int*>(ws + w.off_bcnt);
    const int m = (int)n_matches;
    // (block counts in int64: a size just below 2^31 plus the block size does not fit an int)
    const auto blocks = [](int64_t n) { return (unsigned)((n + kCollateBlock - 1) / kCollateBlock); };
    hipLaunchKernelGGL(collate_init_kernel, dim3(blocks(ns > nt ? ns : nt)), dim3(kCollateBlock), 0, st, pos_src, first_row,
                       (int)ns, pos_tgt, first_src, (int)nt, out_count);
    UMEREG_CHECK_LAUNCH("collate_init_kernel");
    const CollateSide src = {src_pts, src_seg, src_coords, src_pts_tform, keep_src, out_src_pts, out_src_seg, out_src_coords,
                             out_src_pts_tform, pos_src, (int)ns, (int)n_src};
    const CollateSide tgt = {tgt_pts, tgt_seg, tgt_coords, nullptr, keep_tgt, out_tgt_pts, out_tgt_seg, out_tgt_coords,
                             nullptr, pos_tgt, (int)nt, (int)n_tgt};
    const int src_blocks = (int)blocks(n_src), tgt_blocks = (int)blocks(n_tgt);
    hipLaunchKernelGGL(collate_gather_kernel, dim3(src_blocks + tgt_blocks), dim3(kCollateBlock), 0, st, src, tgt, src_blocks, b, out_count);
    UMEREG_CHECK_LAUNCH("collate_gather_kernel");
    if (m == 0) return UMEREG_OK;                                          // out_count[0] = 0 is the init kernel's
    const unsigned m_blocks = blocks(n_matches);
    hipLaunchKernelGGL(collate_first_row_kernel, dim3(m_blocks), dim3(kCollateBlock), 0, st, matches, m, (int)ns, (int)nt, first_row, out_count);
    UMEREG_CHECK_LAUNCH("collate_first_row_kernel");
    hipLaunchKernelGGL(collate_first_src_kernel, dim3(m_blocks), dim3(kCollateBlock), 0, st, matches, m, (int)ns, (int)nt,
                       (const int*)first_row, (const int*)pos_src, first_src);
    UMEREG_CHECK_LAUNCH("collate_first_src_kernel");
    hipLaunchKernelGGL(collate_compact_kernel<0>, dim3(w.n_blocks), dim3(kCollateCompactBlock), 0, st, (const int*)first_src,
                       (const int*)pos_src, (const int*)pos_tgt, (int)nt, bcnt, out_matches);
    UMEREG_CHECK_LAUNCH("collate_compact_kernel");
    hipLaunchKernelGGL(collate_scan_kernel, dim3(1), dim3(1024), 0, st, w.n_blocks, bcnt, out_count);
    UMEREG_CHECK_LAUNCH("collate_scan_kernel");
    hipLaunchKernelGGL(collate_compact_kernel<1>, dim3(w.n_blocks), dim3(kCollateCompactBlock), 0, st, (const int*)first_src,
                       (const int*)pos_src, (const int*)pos_tgt, (int)nt, bcnt, out_matches);
    UMEREG_CHECK_LAUNCH("collate_compact_kernel");
    return UMEREG_OK;
}
