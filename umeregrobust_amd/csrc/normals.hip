// normals.hip -- target normals for the point-to-plane ICP (icp.hip): open3d's estimate_normals with a kNN or a hybrid search.
// Two steps on one stream, nothing waited for:
//   umereg_knn_points_f32   the min(knn, n) nearest points of the cloud for every point of it (exact, ties -> lower index), written
//                           into this call's workspace;
//   normals_kernel          one lane per point: the neighbours' mean, their covariance about that mean and the eigenvector of its
//                           smallest eigenvalue, all in fp64 (icp_plane_math.h).  Clouds sit up to 1e3 m from the origin: moments about
//                           the origin would cancel 1e6 against 1e-2.
// One lane per point: a point is ~30 dependent gathers of 12 bytes (latency, not bandwidth), 120 000 points are 1 900 wavefronts --
// enough to hide them; no LDS, no atomics, no cross-lane step, so the output is the same in every run.
#include "grid.h"
#include "umereg_icp_plane.h"
#include "icp_plane_math.h"

namespace umereg {

constexpr int kNormalsWG = 256;

__global__ __launch_bounds__(kNormalsWG) void normals_kernel(const float* __restrict__ pts, const int64_t* __restrict__ idx,
                                                             const float* __restrict__ dists, int n, int K, int use_radius, float r2,
                                                             float* __restrict__ out)
{
    const int i = blockIdx.x * kNormalsWG + threadIdx.x;
    if (i >= n) return;
    const int64_t* __restrict__ row = idx + (size_t)i * K;
    const float* __restrict__ drow = dists + (size_t)i * K;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0;
    for (int e = 0; e < K; ++e) {
        const int64_t j = row[e];
        if (j < 0 || j >= n || (use_radius && drow[e] > r2)) continue;
        sx += (double)pts[3 * j + 0]; sy += (double)pts[3 * j + 1]; sz += (double)pts[3 * j + 2];
        ++cnt;
    }
    double nrm[3] = {0.0, 0.0, 1.0};
    if (cnt >= 3) {
        const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
        double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int e = 0; e < K; ++e) {
            const int64_t j = row[e];
            if (j < 0 || j >= n || (use_radius && drow[e] > r2)) continue;
            const double dx = (double)pts[3 * j + 0] - mx, dy = (double)pts[3 * j + 1] - my, dz = (double)pts[3 * j + 2] - mz;
            c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz;
            c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
        }
        covariance_normal(c, nrm);
    }
    out[3 * (size_t)i + 0] = (float)nrm[0];
    out[3 * (size_t)i + 1] = (float)nrm[1];
    out[3 * (size_t)i + 2] = (float)nrm[2];
}

static inline int normals_k(int n, int knn) { return knn < n ? knn : n; }

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_normals_workspace_bytes(int n, int knn)
{
    if (n <= 0 || knn < UMEREG_NORMALS_MIN_KNN || knn > UMEREG_NORMALS_MAX_KNN) return 0;
    const size_t rows = (size_t)n * normals_k(n, knn);
    return align_up(umereg_knn_workspace_bytes(1, n), 256) + align_up(rows * sizeof(float), 256) + align_up(rows * sizeof(int64_t), 256);
}

UMEREG_API int umereg_estimate_normals_f32(const float* pts, int n, int knn, float radius, float* normals, void* workspace,
                                           size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(pts && normals, "estimate_normals: null pointer");
    UMEREG_REQUIRE(n > 0, "estimate_normals: empty cloud (n %d)", n);
    UMEREG_REQUIRE(knn >= UMEREG_NORMALS_MIN_KNN && knn <= UMEREG_NORMALS_MAX_KNN, "estimate_normals: knn must be in [%d, %d] (got %d)",
                   UMEREG_NORMALS_MIN_KNN, UMEREG_NORMALS_MAX_KNN, knn);
    UMEREG_REQUIRE(radius == radius, "estimate_normals: radius is NaN");
    if (int rc = check_device()) return rc;
    UMEREG_REQUIRE_WORKSPACE("estimate_normals", workspace, workspace_bytes, umereg_normals_workspace_bytes(n, knn));
    const int K = normals_k(n, knn);
    const size_t rows = (size_t)n * K;
    char* ws = (char*)workspace;
    const size_t knn_bytes = align_up(umereg_knn_workspace_bytes(1, n), 256);
    float* dists = (float*)(ws + knn_bytes);
    int64_t* idx = (int64_t*)(ws + knn_bytes + align_up(rows * sizeof(float), 256));
    if (int rc = umereg_knn_points_f32(pts, pts, 1, n, n, K, dists, idx, ws, knn_bytes, stream)) return rc;
    const int use_radius = radius > 0.f;
    hipLaunchKernelGGL(normals_kernel, dim3((n + kNormalsWG - 1) / kNormalsWG), dim3(kNormalsWG), 0, (hipStream_t)stream, pts, idx, dists,
                       n, K, use_radius, radius * radius, normals);
    UMEREG_CHECK_LAUNCH("normals_kernel");
    return UMEREG_OK;
}
