// scan_prep.hip -- one raw lidar scan made ready for voxel thinning (include/umereg_scan_prep.h): the semantic half of the label
// word, the learning map, the ego box and the unlabelled mask of the reference's loaders (datasets/kitti/kitti_dataset.py:300-314,
// :407-413; datasets/nuscenes/nuscenes_dataset.py:403-421), and the compaction of what is left, in scan order.
//
//   count    one thread per scan row (an aligned 16-byte row is read as a vector, of which the compiler keeps the dwords in use: x, y
//            here, x, y, z in the scatter; a 12-byte or unaligned row is scalar loads): keep / error predicate, per-block keep count
//            and error bits -> workspace
//   scan     one block: the block counts -> block offsets, total and the OR of the error bits -> out_count
//   scatter  the same predicate again, the row written at its rank
//
// The compaction is compact.h's; every workspace word the scan reads was written by the count pass of the same call.  Launch-bound,
// bandwidth-trivial work (2 MB per KITTI scan, read twice): three short launches and no more machinery than that.
#include "compact.h"
#include "umereg_scan_prep.h"

namespace umereg {

constexpr int kScanPrepBlock = UMEREG_SCAN_PREP_BLOCK;
constexpr int kScanPrepScanBlock = 1024;                 // threads of the one block that scans the block counts
constexpr int64_t kScanPrepMaxN = (int64_t)1 << 31;      // indices are int32 inside

struct ScanPrepWs {
    size_t off_bcnt, off_berr, total;
    int n_blocks;
};

inline ScanPrepWs scan_prep_ws(int64_t n)
{
    ScanPrepWs w;
    w.n_blocks = (int)((n + kScanPrepBlock - 1) / kScanPrepBlock);
    size_t o = 0;
    w.off_bcnt = o; o += ((size_t)w.n_blocks * 4 + 255) / 256 * 256;
    w.off_berr = o; o += ((size_t)w.n_blocks * 4 + 255) / 256 * 256;
    w.total = o;
    return w;
}

struct ScanPrepArgs {
    const float* scan;
    const uint32_t* labels;
    const int32_t* lut;
    int n, stride, n_lut;
    unsigned flags;
    float ego_hx, ego_hy;      // both > 0, or both 0 (filter off)
};

// compact.h's count (PASS 0: also the block's error bits -> berr) and scatter (PASS 1) over the rows that stay.
// VEC4: rows of 4 floats at a 16-byte aligned base, read as one vector.
template <int PASS, bool VEC4>
__global__ __launch_bounds__(kScanPrepBlock) void scan_prep_kernel(ScanPrepArgs a, int* __restrict__ bcnt, int* __restrict__ berr,
                                                                    float* __restrict__ out_pts, int64_t* __restrict__ out_seg,
                                                                    int64_t* __restrict__ out_index)
{
    __shared__ int wave_err[kScanPrepBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kScanPrepBlock + threadIdx.x;
    bool keep = false;
    int err = 0;
    float x = 0.f, y = 0.f, z = 0.f;
    int64_t seg = 0;
    if (i < a.n) {
        if (VEC4) {
            const float4 r = reinterpret_cast<const float4*>(a.scan)[i];
            x = r.x; y = r.y; z = r.z;
        } else {
            const float* r = a.scan + (size_t)i * a.stride;
            x = r[0]; y = r[1]; z = r[2];
        }
        uint32_t sem = a.labels ? a.labels[i] : 1u;
        if (a.flags & UMEREG_SCAN_SEM16) sem &= 0xFFFFu;
        if (a.lut) {
            if (sem >= (uint32_t)a.n_lut) {
                err = UMEREG_SCAN_ERR_KEY_RANGE;
            } else {
                const int32_t v = a.lut[sem];
                if (v < 0) err = UMEREG_SCAN_ERR_KEY_UNMAPPED;
                else seg = v;
            }
        } else {
            seg = (int64_t)sem;
        }
        const bool ego = a.ego_hx > 0.f && fabsf(x) <= a.ego_hx && fabsf(y) <= a.ego_hy;      // (false for a NaN coordinate)
        keep = !ego && (seg != 0 || (a.flags & UMEREG_SCAN_KEEP_UNLABELED));
    }
    if (PASS == 0) {
        const unsigned long long e1 = __ballot(err & 1), e2 = __ballot(err & 2);
        if (lane_id() == 0) wave_err[threadIdx.x >> 6] = (e1 ? 1 : 0) | (e2 ? 2 : 0);      // (read behind block_rank's barrier)
    }
    const BlockRank k = block_rank<kScanPrepBlock>(keep);
    if (PASS == 0) {
        if (threadIdx.x == 0) {
            int e = 0;
            for (int v = 0; v < kScanPrepBlock / 64; ++v) e |= wave_err[v];
            bcnt[blockIdx.x] = k.total;
            berr[blockIdx.x] = e;
        }
    } else if (keep) {
        const size_t r = (size_t)(bcnt[blockIdx.x] + k.before);       // r <= i < n: inside the outputs
        out_pts[3 * r] = x; out_pts[3 * r + 1] = y; out_pts[3 * r + 2] = z;
        out_seg[r] = seg;
        if (out_index) out_index[r] = i;
    }
}

// block counts -> block offsets (in place), number of kept rows -> out_count[0], OR of the blocks' error bits -> out_count[1]
__global__ __launch_bounds__(kScanPrepScanBlock) void scan_prep_scan_kernel(int n_blocks, int* __restrict__ bcnt,
                                                                             const int* __restrict__ berr, int* __restrict__ out_count)
{
    int e = 0;
    for (int k = threadIdx.x; k < n_blocks; k += kScanPrepScanBlock) e |= berr[k];
    const int total = scan_counts<kScanPrepScanBlock>(bcnt, bcnt, nullptr, n_blocks);
    const int e1 = __syncthreads_or(e & 1), e2 = __syncthreads_or(e & 2);
    if (threadIdx.x == kScanPrepScanBlock - 1) {
        out_count[0] = total;
        out_count[1] = (e1 ? 1 : 0) | (e2 ? 2 : 0);
    }
}

static bool scan_prep_size_ok(int64_t n) { return n > 0 && n < kScanPrepMaxN; }

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_scan_prep_workspace_bytes(int64_t n) { return scan_prep_size_ok(n) ? scan_prep_ws(n).total : 0; }

UMEREG_API int umereg_scan_prep_f32(const float* scan, int64_t n, int stride, const uint32_t* labels, int flags, const int32_t* lut,
                                    int64_t n_lut, float ego_hx, float ego_hy, float* out_pts, int64_t* out_seg, int64_t* out_index,
                                    int* out_count, void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "scan_prep_f32";
    UMEREG_REQUIRE(scan_prep_size_ok(n), "%s: the number of scan rows must lie in [1, 2^31) (got %lld)", who, (long long)n);
    UMEREG_REQUIRE(stride == 3 || stride == 4, "%s: a scan row has 3 or 4 floats (got %d)", who, stride);
    UMEREG_REQUIRE((flags & ~(UMEREG_SCAN_SEM16 | UMEREG_SCAN_KEEP_UNLABELED)) == 0, "%s: unknown flag bits 0x%x", who, flags);
    UMEREG_REQUIRE(n_lut >= 0 && n_lut < kScanPrepMaxN && !lut == (n_lut == 0),
                   "%s: the label map needs a pointer and 0 < n_lut < 2^31, or neither (got n_lut %lld)", who, (long long)n_lut);
    UMEREG_REQUIRE(ego_hx == ego_hx && ego_hy == ego_hy, "%s: an extent of the ego box is NaN", who);
    UMEREG_REQUIRE(scan && out_pts && out_seg && out_count, "%s: null pointer (scan, out_pts, out_seg, out_count)", who);
    UMEREG_REQUIRE((((uintptr_t)scan | (uintptr_t)out_pts | (uintptr_t)labels | (uintptr_t)lut | (uintptr_t)out_count) & 3) == 0 &&
                       (((uintptr_t)out_seg | (uintptr_t)out_index) & 7) == 0,
                   "%s: a pointer is not aligned to its element type", who);
    if (int rc = check_device()) return rc;
    const ScanPrepWs w = scan_prep_ws(n);
    UMEREG_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    int* bcnt = reinterpret_cast<int*>((char*)workspace + w.off_bcnt);
    int* berr = reinterpret_cast<int*>((char*)workspace + w.off_berr);
    const bool filter = ego_hx > 0.f && ego_hy > 0.f;
    const ScanPrepArgs a = {scan, labels, lut, (int)n, stride, (int)n_lut, (unsigned)flags, filter ? ego_hx : 0.f, filter ? ego_hy : 0.f};
    const bool vec4 = stride == 4 && ((uintptr_t)scan & 15) == 0;
    const dim3 grid(w.n_blocks), block(kScanPrepBlock);
    if (vec4) hipLaunchKernelGGL((scan_prep_kernel<0, true>), grid, block, 0, st, a, bcnt, berr, out_pts, out_seg, out_index);
    else hipLaunchKernelGGL((scan_prep_kernel<0, false>), grid, block, 0, st, a, bcnt, berr, out_pts, out_seg, out_index);
    UMEREG_CHECK_LAUNCH("scan_prep_kernel");
    hipLaunchKernelGGL(scan_prep_scan_kernel, dim3(1), dim3(kScanPrepScanBlock), 0, st, w.n_blocks, bcnt, (const int*)berr, out_count);
    UMEREG_CHECK_LAUNCH("scan_prep_scan_kernel");
    if (vec4) hipLaunchKernelGGL((scan_prep_kernel<1, true>), grid, block, 0, st, a, bcnt, berr, out_pts, out_seg, out_index);
    else hipLaunchKernelGGL((scan_prep_kernel<1, false>), grid, block, 0, st, a, bcnt, berr, out_pts, out_seg, out_index);
    UMEREG_CHECK_LAUNCH("scan_prep_kernel");
    return UMEREG_OK;
}
