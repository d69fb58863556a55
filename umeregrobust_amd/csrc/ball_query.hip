// ball_query.hip -- a1 (ball query) for gfx950.  Replaces pytorch3d.ops.ball_query (reference evaluate.py:51).
//
//   a1      the ball-query entry point sorts the K kept indices (bitonic, in LDS) to emit
//           pytorch3d's ascending order, then recomputes dists / nn from them.
// The structure it searches is built by grid.hip; the search is ball_search.h.
#include "ball_search.h"

namespace umereg {

// ---- a1: ball query with idx / dists / nn outputs ---------------------------------------------
template <bool kFma>
__global__ __launch_bounds__(256) void ball_query_kernel(
    const char* __restrict__ ws, size_t ws_stride, const float* __restrict__ p1,
    const int64_t* __restrict__ lengths1, const int64_t* __restrict__ lengths2, int n1, int n2, int K, int cap,
    float radius, int64_t* __restrict__ idx, float* __restrict__ dists, float* __restrict__ nn)
{
    extern __shared__ int lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int b = blockIdx.y;
    const int i = blockIdx.x * (blockDim.x >> 6) + wave;
    if (i >= n1) return;
    int* lst = lds + wave * cap;
    const GridWs w = grid_ws(n2);
    const char* wb = ws + b * ws_stride;
    const float4* P4o = reinterpret_cast<const float4*>(wb + w.off_p4o);
    const float4* P4s = reinterpret_cast<const float4*>(wb + w.off_p4s);
    const int* start = reinterpret_cast<const int*>(wb + w.off_start);
    const Grid g = load_grid(reinterpret_cast<const unsigned int*>(wb + w.off_bbox), radius, n2);
    const int len1 = lengths1 ? (int)lengths1[b] : n1;
    int len2 = lengths2 ? (int)lengths2[b] : n2;
    len2 = len2 < n2 ? len2 : n2;
    const float* q = p1 + ((size_t)b * n1 + i) * 3;
    const float qx = q[0], qy = q[1], qz = q[2];
    const float r2 = radius * radius;
    const int nbits = 32 - __clz(n2 > 1 ? n2 - 1 : 1);
    int count = 0;
    if (i < len1 && len2 > 0) count = ball_search_grid<kFma>(P4s, start, g, qx, qy, qz, r2, K, len2, nbits, lst, cap, lane);
    sort_kept(lst, count, lane);   // pytorch3d emits the kept indices in ascending order
    const size_t row = ((size_t)b * n1 + i) * K;
    for (int e = lane; e < K; e += kWave) {
        int64_t j = -1;
        float d2 = 0.f, x = 0.f, y = 0.f, z = 0.f;
        if (e < count) {
            const int jj = lst[e];
            const float4 p = P4o[jj];
            const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
            d2 = dist2_as_the_reference<kFma>(dx, dy, dz);
            x = p.x; y = p.y; z = p.z;
            j = jj;
        }
        idx[row + e] = j;
        if (dists) dists[row + e] = d2;
        if (nn) {
            float* o = nn + (row + e) * 3;
            o[0] = x; o[1] = y; o[2] = z;
        }
    }
}

}  // namespace umereg

using namespace umereg;

UMEREG_API int umereg_ball_query_f32(const float* p1, const float* p2, const int64_t* lengths1,
                                     const int64_t* lengths2, int B, int n1, int n2, int K,
                                     float radius, int64_t* idx, float* dists, float* nn,
                                     void* workspace, size_t workspace_bytes, void* stream)
{
    return umereg_ball_query_ex_f32(p1, p2, lengths1, lengths2, B, n1, n2, K, radius, 0, idx, dists, nn, workspace, workspace_bytes, stream);
}

UMEREG_API int umereg_ball_query_ex_f32(const float* p1, const float* p2, const int64_t* lengths1,
                                        const int64_t* lengths2, int B, int n1, int n2, int K,
                                        float radius, int flags, int64_t* idx, float* dists, float* nn,
                                        void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(p1 && p2 && idx, "ball_query: null pointer (p1/p2/idx)");
    UMEREG_REQUIRE(B > 0 && n1 > 0 && n2 > 0, "ball_query: B, n1, n2 must be positive (got %d, %d, %d)", B, n1, n2);
    UMEREG_REQUIRE(K > 0 && K <= kMaxBallK, "ball_query: K must be in [1, 7680] (got %d)", K);
    UMEREG_REQUIRE(radius > 0.f, "ball_query: radius must be positive");
    UMEREG_REQUIRE((flags & ~UMEREG_BALL_FMA) == 0, "ball_query: unknown flags 0x%x", flags);
    if (int rc = check_device()) return rc;
    UMEREG_REQUIRE_WORKSPACE("ball_query", workspace, workspace_bytes, umereg_ball_query_workspace_bytes(B, n2));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_prep(p2, (char*)workspace, B, n2, radius, st)) return rc;
    int cap, waves;
    lds_plan(K, &cap, &waves);
    dim3 grid((n1 + waves - 1) / waves, B);
    if (flags & UMEREG_BALL_FMA)
        hipLaunchKernelGGL(ball_query_kernel<true>, grid, dim3(kWave * waves), (size_t)waves * cap * sizeof(int), st,
                           (const char*)workspace, grid_ws(n2).total, p1, lengths1, lengths2, n1, n2, K, cap, radius,
                           idx, dists, nn);
    else
        hipLaunchKernelGGL(ball_query_kernel<false>, grid, dim3(kWave * waves), (size_t)waves * cap * sizeof(int), st,
                           (const char*)workspace, grid_ws(n2).total, p1, lengths1, lengths2, n1, n2, K, cap, radius,
                           idx, dists, nn);
    UMEREG_CHECK_LAUNCH("ball_query_kernel");
    return UMEREG_OK;
}
