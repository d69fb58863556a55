// voxel_centroid.hip -- one centroid per occupied voxel (open3d's voxel_down_sample; contract: voxel_centroid_api.h; arithmetic:
// voxel_centroid_math.h).  Insertion and compaction are NOT restated: the entry calls umereg_voxel_first_index_f32 on the front of its
// workspace and reads what that left there through vox_ws() -- every point's table slot (slot_of) -- and the representatives it wrote
// to first_index.  What is new, behind vox_ws(n).total:
//   one 32-byte accumulator row per table slot (sum x, sum y, sum z in int64, the count), zeroed by a memset;
//   voxel_accumulate_kernel   one lane per point: three 64-bit integer atomic adds and one 32-bit into its slot's row.  Integers, so
//                             any arrival order gives the same sums (a wave-level pre-sum could be added without changing a bit);
//   voxel_finalize_kernel     one lane per rank below the device-side count: the representative's slot -> centroid and count.
// Nothing is read back.
#include "common.h"
#include "voxel_key.h"
#include "voxel_centroid_api.h"
#include "voxel_centroid_math.h"

namespace umereg {

constexpr size_t kVoxAccRow = 32;      // sum x, sum y, sum z (int64), count (int32), 4 bytes of padding

struct VoxAcc {
    long long sum[3];
    int count, pad;
};
static_assert(sizeof(VoxAcc) == kVoxAccRow, "one accumulator row is 32 bytes");

struct VoxCentroidWs {
    size_t off_acc, acc_bytes, total;
};

static VoxCentroidWs vox_centroid_ws(int n)
{
    const VoxWs v = vox_ws(n);
    VoxCentroidWs w;
    w.off_acc = v.total;                              // (a multiple of 256)
    w.acc_bytes = (size_t)v.cap * kVoxAccRow;
    w.total = w.off_acc + w.acc_bytes;
    return w;
}

__global__ __launch_bounds__(256) void voxel_accumulate_kernel(const float* __restrict__ pts, int n, float voxel,
                                                               const char* __restrict__ ws, VoxAcc* __restrict__ acc)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int* slot_of = reinterpret_cast<const unsigned int*>(ws + vox_ws(n).off_slot);
    const unsigned int s = slot_of[i];
    if (s == 0xffffffffu) return;                     // (no key: reported through count[1] by the insertion)
    VoxAcc* a = acc + s;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p = pts[(size_t)i * 3 + k];
        const long long q = voxel_quantum(p, voxel, voxel_cell(p, voxel));
        atomicAdd(reinterpret_cast<unsigned long long*>(&a->sum[k]), (unsigned long long)q);
    }
    atomicAdd(&a->count, 1);
}

__global__ __launch_bounds__(256) void voxel_finalize_kernel(const float* __restrict__ pts, int n, float voxel, const char* __restrict__ ws,
                                                             const VoxAcc* __restrict__ acc, const int64_t* __restrict__ first_index,
                                                             const int* __restrict__ count, float* __restrict__ centroids,
                                                             int32_t* __restrict__ counts)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n || r >= count[0]) return;
    const unsigned int* slot_of = reinterpret_cast<const unsigned int*>(ws + vox_ws(n).off_slot);
    const int64_t i = first_index[r];
    const VoxAcc a = acc[slot_of[i]];                 // (a representative has a slot)
#pragma unroll
    for (int k = 0; k < 3; ++k)
        centroids[(size_t)r * 3 + k] = voxel_centroid(voxel_cell(pts[(size_t)i * 3 + k], voxel), a.sum[k], a.count, voxel);
    counts[r] = a.count;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_voxel_centroid_workspace_bytes(int n)
{
    return n > 0 && n <= UMEREG_VOXEL_CENTROID_MAX_POINTS ? vox_centroid_ws(n).total : 0;
}

UMEREG_API int umereg_voxel_centroid_f32(const float* pts, int n, float voxel, float* centroids, int64_t* first_index, int32_t* counts,
                                         int* count, void* workspace, size_t workspace_bytes, void* stream)
{
    static_assert(UMEREG_VOXEL_CENTROID_MAX_POINTS == kVoxCentroidMaxPoints, "one cap");
    UMEREG_REQUIRE(pts && centroids && first_index && counts && count, "voxel_centroid: null pointer");
    UMEREG_REQUIRE(n > 0 && n <= UMEREG_VOXEL_CENTROID_MAX_POINTS, "voxel_centroid: n must be in [1, 2^20] (got %d): the 64-bit sums are exact in fp64 up to there", n);
    UMEREG_REQUIRE(voxel > 0.f, "voxel_centroid: the voxel edge must be positive");
    if (int rc = check_device()) return rc;
    const VoxCentroidWs w = vox_centroid_ws(n);
    UMEREG_REQUIRE_WORKSPACE("voxel_centroid", workspace, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (int rc = umereg_voxel_first_index_f32(pts, n, voxel, first_index, count, workspace, w.off_acc, stream)) return rc;
    VoxAcc* acc = reinterpret_cast<VoxAcc*>(ws + w.off_acc);
    if (hipMemsetAsync(acc, 0, w.acc_bytes, st) != hipSuccess) {
        set_error("voxel_centroid: hipMemsetAsync failed");
        return UMEREG_ELAUNCH;
    }
    const dim3 grid((n + 255) / 256), block(256);
    hipLaunchKernelGGL(voxel_accumulate_kernel, grid, block, 0, st, pts, n, voxel, (const char*)ws, acc);
    UMEREG_CHECK_LAUNCH("voxel_accumulate_kernel");
    hipLaunchKernelGGL(voxel_finalize_kernel, grid, block, 0, st, pts, n, voxel, (const char*)ws, (const VoxAcc*)acc,
                       (const int64_t*)first_index, (const int*)count, centroids, counts);
    UMEREG_CHECK_LAUNCH("voxel_finalize_kernel");
    return UMEREG_OK;
}
