// Voxel thinning of a raw cloud: MinkowskiEngine.utils.sparse_quantize(coordinates, return_index=True, quantization_size)
// as called at reference evaluate.py:261-264 (and datasets/kitti/kitti_dataset.py:416-419): one representative per
// occupied voxel -- here, as in this library's torch restatement, the FIRST point of every voxel (lowest index), indices
// ascending (MinkowskiEngine 0.5.4 is not installable: parity unpinned).
//
// No sort: a voxel's first point is the minimum index over its points, which an open-addressing hash table over the
// 63-bit voxel key finds with one atomicMin per point (order independent, hence deterministic); the representatives are
// the points whose own index is their voxel's minimum, compacted in index order (compact.h).
// The table plan, the key and its home slot are voxel_key.h's (host-checkable: tests/test_voxel_key_cpu.py).
// 4 small kernels + 1 memset instead of ~15 torch launches with two device sorts (evaluate.py's loop: 0.30 -> 0.03 ms).
#include "compact.h"
#include "voxel_key.h"

namespace umereg {

__global__ __launch_bounds__(256) void voxel_insert_kernel(const float* __restrict__ pts, int n, float voxel, char* __restrict__ ws,
                                                           int* __restrict__ out_count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const VoxWs w = vox_ws(n);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + w.off_keys);
    unsigned int* mins = reinterpret_cast<unsigned int*>(ws + w.off_min);
    unsigned int* slot_of = reinterpret_cast<unsigned int*>(ws + w.off_slot);
    unsigned long long key;
    if (!voxel_key(pts + (size_t)i * 3, voxel, key)) {
        out_count[1] = 1;                               // a coordinate outside the key range: reported by the host
        slot_of[i] = 0xffffffffu;
        return;
    }
    unsigned int s = voxel_home_slot(key, w.cap);
    for (;;) {
        const unsigned long long old = atomicCAS(&keys[s], kVoxEmpty, key);
        if (old == kVoxEmpty || old == key) break;
        s = (s + 1u) & (w.cap - 1u);
    }
    atomicMin(&mins[s], (unsigned int)i);
    slot_of[i] = s;
}

// compact.h's count (PASS 0) and scatter (PASS 1) over the representatives: the points that are their voxel's minimum
template <int PASS>
__global__ __launch_bounds__(kVoxBlock) void voxel_compact_kernel(int n, char* __restrict__ ws, int64_t* __restrict__ out_idx)
{
    const VoxWs w = vox_ws(n);
    const unsigned int* mins = reinterpret_cast<const unsigned int*>(ws + w.off_min);
    const unsigned int* slot_of = reinterpret_cast<const unsigned int*>(ws + w.off_slot);
    int* bcnt = reinterpret_cast<int*>(ws + w.off_bcnt);
    const int i = blockIdx.x * kVoxBlock + threadIdx.x;
    bool rep = false;
    if (i < n) {
        const unsigned int s = slot_of[i];
        rep = s != 0xffffffffu && mins[s] == (unsigned int)i;
    }
    const BlockRank r = block_rank<kVoxBlock>(rep);
    if (PASS == 0) {
        if (threadIdx.x == 0) bcnt[blockIdx.x] = r.total;
    } else if (rep) {
        out_idx[bcnt[blockIdx.x] + r.before] = (int64_t)i;
    }
}

// block counts -> block offsets (in place), number of representatives -> out_count[0]
__global__ __launch_bounds__(1024) void voxel_scan_kernel(int n, char* __restrict__ ws, int* __restrict__ out_count)
{
    const VoxWs w = vox_ws(n);
    int* bcnt = reinterpret_cast<int*>(ws + w.off_bcnt);
    const int total = scan_counts<1024>(bcnt, bcnt, nullptr, w.n_blocks);
    if (threadIdx.x == 1023) out_count[0] = total;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_voxel_first_index_workspace_bytes(int n)
{
    return n > 0 ? vox_ws(n).total : 0;
}

UMEREG_API int umereg_voxel_first_index_f32(const float* pts, int n, float voxel, int64_t* out_idx, int* out_count, void* workspace,
                                            size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(pts && out_idx && out_count, "voxel_first_index: null pointer");
    UMEREG_REQUIRE(n > 0, "voxel_first_index: n must be positive (got %d)", n);
    UMEREG_REQUIRE(voxel > 0.f, "voxel_first_index: the voxel edge must be positive");
    if (int rc = check_device()) return rc;
    const VoxWs w = vox_ws(n);
    UMEREG_REQUIRE_WORKSPACE("voxel_first_index", workspace, workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    // keys = all ones (empty), minima = all ones (> every index): one memset over both regions
    if (hipMemsetAsync(ws, 0xff, w.off_slot, st) != hipSuccess || hipMemsetAsync(out_count, 0, 2 * sizeof(int), st) != hipSuccess) {
        set_error("voxel_first_index: hipMemsetAsync failed");
        return UMEREG_ELAUNCH;
    }
    hipLaunchKernelGGL(voxel_insert_kernel, dim3((n + 255) / 256), dim3(256), 0, st, pts, n, voxel, ws, out_count);
    UMEREG_CHECK_LAUNCH("voxel_insert_kernel");
    hipLaunchKernelGGL(voxel_compact_kernel<0>, dim3(w.n_blocks), dim3(kVoxBlock), 0, st, n, ws, out_idx);
    UMEREG_CHECK_LAUNCH("voxel_compact_kernel");
    hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(1024), 0, st, n, ws, out_count);
    UMEREG_CHECK_LAUNCH("voxel_scan_kernel");
    hipLaunchKernelGGL(voxel_compact_kernel<1>, dim3(w.n_blocks), dim3(kVoxBlock), 0, st, n, ws, out_idx);
    UMEREG_CHECK_LAUNCH("voxel_compact_kernel");
    return UMEREG_OK;
}
