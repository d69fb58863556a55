// equalize.hip -- the built-in sampling equalizer: a deterministic surfel resampler with one smoothing projection (contract:
// equalize_api.h; arithmetic: equalize_math.h).  Four kernels behind umereg_knn_points_f32 and launch_prep, nothing waited for:
//   eq_surfel_kernel   one lane per point over its kNN list (the shape of normals_kernel): fp64 mean and covariance, covariance_normal,
//                      the capped support r2 and the integer area weight q;
//   eq_scan_kernel     one workgroup: the inclusive 64-bit prefix sum Q of q, 4 096 weights per round (compact.h's scan_counts is int-only;
//                      this is its 64-bit sibling, integers, so exact whatever the order) and Qt;
//   eq_sample_kernel   one lane per sample: systematic position on [0, Qt), binary search over Q (L2-resident: n * 8 bytes), placement on
//                      the source's tangent patch;
//   eq_project_kernel  the hot one: eight lanes per sample walk the x-rows of the grid cells within sqrt(rho2) * 1.001 + 1e-6 exactly as
//                      icp_eval_kernel walks them (consecutive table entries: 128-byte reads), twice -- weighted mean, then weighted
//                      covariance about it -- with fp64 partial sums per lane combined in the xor tree 4, 2, 1; the group's first lane
//                      solves for the normal and moves the sample.
// Only vector stores, no atomics, no LDS beyond the scan's sixteen wave totals.
#include "grid.h"
#include "equalize_api.h"
#include "equalize_math.h"
#include "icp_plane_math.h"

#include <math.h>

namespace umereg {

constexpr int kEqWG = 256;
constexpr int kEqScanThreads = 1024;      // eq_scan_kernel: sixteen wavefronts,
constexpr int kEqScanPer = 4;             // four consecutive weights per lane
constexpr int kEqLanes = 8;               // eq_project_kernel: lanes per sample (icp_eval_kernel's choice, for the same row walk)
constexpr int kEqPerWG = kEqWG / kEqLanes;

static inline int eq_k(int n, int knn) { return knn < n ? knn : n; }

// One carve-up for the four entries.  The stage block is first, so its offsets do not depend on num_points: it holds, one after the
// other in time, the kNN structure with the neighbour lists (surfels), Q (sample) and the grid (project).  The rest is what
// umereg_equalize_cloud_f32 keeps between its stages.
struct EqWs {
    size_t knn_bytes, off_dists, off_idx, stage, off_normals, off_r2, off_q, off_samples, off_rho2, total;
};

static EqWs eq_ws(int n, int num_points, int knn)
{
    EqWs w;
    const size_t rows = (size_t)n * eq_k(n, knn);
    w.knn_bytes = align_up(umereg_knn_workspace_bytes(1, n), 256);
    w.off_dists = w.knn_bytes;
    w.off_idx = w.off_dists + align_up(rows * sizeof(float), 256);
    w.stage = w.off_idx + align_up(rows * sizeof(int64_t), 256);      // >= n * 8 (Q) and >= grid_ws(n).total
    size_t o = w.stage;
    w.off_normals = o; o += align_up((size_t)n * 3 * sizeof(float), 256);
    w.off_r2 = o;      o += align_up((size_t)n * sizeof(float), 256);
    w.off_q = o;       o += align_up((size_t)n * sizeof(uint32_t), 256);
    w.off_samples = o; o += align_up((size_t)num_points * 3 * sizeof(float), 256);
    w.off_rho2 = o;    o += align_up((size_t)num_points * sizeof(float), 256);
    w.total = o;
    return w;
}

__global__ __launch_bounds__(kEqWG) void eq_surfel_kernel(const float* __restrict__ pts, const int64_t* __restrict__ idx,
                                                          const float* __restrict__ dists, int n, int K, float rmax2, float s,
                                                          float* __restrict__ normals, float* __restrict__ r2_out,
                                                          uint32_t* __restrict__ q_out)
{
    const int i = blockIdx.x * kEqWG + threadIdx.x;
    if (i >= n) return;
    const int64_t* __restrict__ row = idx + (size_t)i * K;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int cnt = 0;
    for (int e = 0; e < K; ++e) {
        const int64_t j = row[e];
        if (j < 0 || j >= n) continue;
        sx += (double)pts[3 * j + 0]; sy += (double)pts[3 * j + 1]; sz += (double)pts[3 * j + 2];
        ++cnt;
    }
    double nrm[3] = {0.0, 0.0, 1.0};
    if (cnt >= 3) {
        const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
        double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int e = 0; e < K; ++e) {
            const int64_t j = row[e];
            if (j < 0 || j >= n) continue;
            const double dx = (double)pts[3 * j + 0] - mx, dy = (double)pts[3 * j + 1] - my, dz = (double)pts[3 * j + 2] - mz;
            c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz;
            c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
        }
        covariance_normal(c, nrm);
    }
    const float r2 = fminf(dists[(size_t)i * K + (K - 1)], rmax2);      // the lists are ascending: the K-th neighbour is the last
    normals[3 * (size_t)i + 0] = (float)nrm[0];
    normals[3 * (size_t)i + 1] = (float)nrm[1];
    normals[3 * (size_t)i + 2] = (float)nrm[2];
    r2_out[i] = r2;
    q_out[i] = cnt >= 3 ? eq_area_weight(r2, s) : 0u;
}

// Q[i] = q[0] + .. + q[i] in 64 bits, *total = Q[n-1].  Per round a lane sums its four weights, the wavefront scans the lanes' sums
// (shuffles), the sixteen wave totals cross through LDS, and the carry moves on.
__global__ __launch_bounds__(kEqScanThreads) void eq_scan_kernel(const uint32_t* __restrict__ q, int n, unsigned long long* __restrict__ Q,
                                                                  unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long wave_tot[kEqScanThreads / kWave];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += kEqScanThreads * kEqScanPer) {
        const int i0 = base + (int)threadIdx.x * kEqScanPer;
        unsigned long long v[kEqScanPer];
        unsigned long long run = 0;
#pragma unroll
        for (int k = 0; k < kEqScanPer; ++k) {
            run += i0 + k < n ? (unsigned long long)q[i0 + k] : 0ull;
            v[k] = run;
        }
        unsigned long long incl = run;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += o;
        }
        if (lane == kWave - 1) wave_tot[wave] = incl;
        __syncthreads();
        unsigned long long before = carry, all = 0;
#pragma unroll
        for (int wv = 0; wv < kEqScanThreads / kWave; ++wv) {
            const unsigned long long t = wave_tot[wv];
            if (wv < wave) before += t;
            all += t;
        }
        const unsigned long long excl = before + (incl - run);
#pragma unroll
        for (int k = 0; k < kEqScanPer; ++k)
            if (i0 + k < n) Q[i0 + k] = excl + v[k];
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kEqWG) void eq_sample_kernel(const float* __restrict__ pts, const float* __restrict__ normals,
                                                          const float* __restrict__ r2, const unsigned long long* __restrict__ Q, int n,
                                                          int M, uint32_t seed, float c, float* __restrict__ samples,
                                                          int64_t* __restrict__ src_index, float* __restrict__ rho2)
{
    const int j = blockIdx.x * kEqWG + threadIdx.x;
    if (j >= M) return;
    const unsigned long long Qt = Q[n - 1];
    if (Qt == 0ull) {      // nothing to sample from: defined bytes, and `total` tells the caller
        samples[3 * (size_t)j + 0] = 0.f; samples[3 * (size_t)j + 1] = 0.f; samples[3 * (size_t)j + 2] = 0.f;
        src_index[j] = -1;
        rho2[j] = 0.f;
        return;
    }
    const unsigned long long u = eq_alloc((uint64_t)j, Qt, (uint64_t)M, eq_xi(seed, 0u, 0u));
    int lo = 0, hi = n - 1;      // the first i with Q[i] > u; Q[n-1] = Qt > u
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (Q[mid] > u) hi = mid;
        else lo = mid + 1;
    }
    const size_t i = (size_t)lo;
    const float p[3] = {pts[3 * i + 0], pts[3 * i + 1], pts[3 * i + 2]};
    const float nr[3] = {normals[3 * i + 0], normals[3 * i + 1], normals[3 * i + 2]};
    const float rr = r2[i];
    float x[3];
    eq_place(p, nr, rr, c, eq_xi(seed, (uint32_t)j, 1u), eq_xi(seed, (uint32_t)j, 2u), x);
    samples[3 * (size_t)j + 0] = x[0]; samples[3 * (size_t)j + 1] = x[1]; samples[3 * (size_t)j + 2] = x[2];
    src_index[j] = (int64_t)lo;
    rho2[j] = rr;
}

// the sum of a sample's eight lanes, the same bits in each of them: xor tree 4, 2, 1
__device__ __forceinline__ double eq_group_sum(double v)
{
#pragma unroll
    for (int m = kEqLanes / 2; m >= 1; m >>= 1) v += shfl_xor_f64(v, m);
    return v;
}

__global__ __launch_bounds__(kEqWG) void eq_project_kernel(const float* __restrict__ samples, const float* __restrict__ rho2, int M,
                                                           const char* __restrict__ ws, int n, float* __restrict__ out,
                                                           int32_t* __restrict__ nb_count)
{
    const GridWs w = grid_ws(n);
    const float4* __restrict__ P4s = reinterpret_cast<const float4*>(ws + w.off_p4s);
    const int* __restrict__ start = reinterpret_cast<const int*>(ws + w.off_start);
    const Grid g = load_grid(reinterpret_cast<const unsigned int*>(ws + w.off_bbox), -1.0f, n);
    const int sub = threadIdx.x & (kEqLanes - 1);
    const int j = blockIdx.x * kEqPerWG + (int)(threadIdx.x / kEqLanes);
    const bool live = j < M;
    const size_t jj = live ? (size_t)j : 0;
    const float fx = samples[3 * jj + 0], fy = samples[3 * jj + 1], fz = samples[3 * jj + 2];
    const float rr = rho2[jj];
    // cells that can hold a point within sqrt(rho2) (slack covers the rounding of the cell map)
    const float r = sqrtf(rr) * 1.001f + 1e-6f;
    const int x0 = cell_axis(fx - r, g.minx, g.invx, g.nx), x1 = cell_axis(fx + r, g.minx, g.invx, g.nx);
    const int y0 = cell_axis(fy - r, g.miny, g.invy, g.ny), y1 = cell_axis(fy + r, g.miny, g.invy, g.ny);
    const int z0 = cell_axis(fz - r, g.minz, g.invz, g.nz), z1 = cell_axis(fz + r, g.minz, g.invz, g.nz);
    // pass 1: sum w, sum w e with e = p - x (exact in fp64: both are f32)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int cnt = 0;
    if (live)
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int cbase = (z * g.ny + y) * g.nx;
                const int beg = start[cbase + x0], end = start[cbase + x1 + 1];   // cells of one x-row are contiguous
                for (int k = beg + sub; k < end; k += kEqLanes) {
                    const float4 t = P4s[k];
                    const float d2 = eq_d2(fx - t.x, fy - t.y, fz - t.z);
                    if (d2 < rr) {
                        const double wt = eq_weight(d2, rr);
                        s0 += wt;
                        s1 += wt * ((double)t.x - (double)fx);
                        s2 += wt * ((double)t.y - (double)fy);
                        s3 += wt * ((double)t.z - (double)fz);
                        ++cnt;
                    }
                }
            }
    s0 = eq_group_sum(s0); s1 = eq_group_sum(s1); s2 = eq_group_sum(s2); s3 = eq_group_sum(s3);
#pragma unroll
    for (int m = kEqLanes / 2; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, kWave);
    const bool fit = live && cnt >= 3;      // (cnt >= 1 makes s0 > 0: every weight is positive)
    const double m0 = fit ? s1 / s0 : 0.0, m1 = fit ? s2 / s0 : 0.0, m2 = fit ? s3 / s0 : 0.0;
    // pass 2: the weighted covariance about the weighted mean
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (fit)
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                const int cbase = (z * g.ny + y) * g.nx;
                const int beg = start[cbase + x0], end = start[cbase + x1 + 1];
                for (int k = beg + sub; k < end; k += kEqLanes) {
                    const float4 t = P4s[k];
                    const float d2 = eq_d2(fx - t.x, fy - t.y, fz - t.z);
                    if (d2 < rr) {
                        const double wt = eq_weight(d2, rr);
                        const double ex = ((double)t.x - (double)fx) - m0, ey = ((double)t.y - (double)fy) - m1,
                                     ez = ((double)t.z - (double)fz) - m2;
                        c[0] += wt * (ex * ex); c[1] += wt * (ex * ey); c[2] += wt * (ex * ez);
                        c[3] += wt * (ey * ey); c[4] += wt * (ey * ez); c[5] += wt * (ez * ez);
                    }
                }
            }
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = eq_group_sum(c[k]);
    if (!live || sub != 0) return;
    double px = (double)fx, py = (double)fy, pz = (double)fz;
    if (fit && !(c[0] == 0.0 && c[1] == 0.0 && c[2] == 0.0 && c[3] == 0.0 && c[4] == 0.0 && c[5] == 0.0)) {
        double nrm[3];
        covariance_normal(c, nrm);
        const double along = (m0 * nrm[0] + m1 * nrm[1]) + m2 * nrm[2];      // -(x - mu) . n
        px += along * nrm[0]; py += along * nrm[1]; pz += along * nrm[2];
    }
    out[3 * (size_t)j + 0] = (float)px; out[3 * (size_t)j + 1] = (float)py; out[3 * (size_t)j + 2] = (float)pz;
    if (nb_count) nb_count[j] = cnt;
}

// the argument rules the entries share; NaN fails the range test
static int eq_check(const char* who, int n, int num_points, int knn)
{
    UMEREG_REQUIRE(n > 0 && num_points > 0, "%s: empty cloud or no samples (n %d, num_points %d)", who, n, num_points);
    UMEREG_REQUIRE(n <= UMEREG_EQUALIZE_MAX_POINTS && num_points <= UMEREG_EQUALIZE_MAX_POINTS,
                   "%s: n and num_points must not exceed 2^22 (got %d, %d)", who, n, num_points);
    UMEREG_REQUIRE(knn >= UMEREG_EQUALIZE_MIN_KNN && knn <= UMEREG_EQUALIZE_MAX_KNN, "%s: knn must be in [%d, %d] (got %d)", who,
                   UMEREG_EQUALIZE_MIN_KNN, UMEREG_EQUALIZE_MAX_KNN, knn);
    return UMEREG_OK;
}

static int eq_check_radius(const char* who, float max_radius)
{
    UMEREG_REQUIRE(max_radius >= UMEREG_EQUALIZE_MIN_RADIUS && max_radius <= UMEREG_EQUALIZE_MAX_RADIUS,
                   "%s: max_radius %g outside [1e-3, 1e3]", who, (double)max_radius);
    return UMEREG_OK;
}

// fewer than three points: every q is 0, so Qt == 0 whatever the coordinates
static int eq_check_samplable(const char* who, int n)
{
    UMEREG_REQUIRE(n >= 3, "%s: Qt == 0: a cloud of %d points has no surfel with an area (3 are the least)", who, n);
    return UMEREG_OK;
}

static int eq_surfels(const float* pts, int n, int knn, float max_radius, float* normals, float* r2, uint32_t* q, char* ws,
                      hipStream_t st)
{
    const EqWs w = eq_ws(n, 1, knn);
    const int K = eq_k(n, knn);
    float* dists = (float*)(ws + w.off_dists);
    int64_t* idx = (int64_t*)(ws + w.off_idx);
    if (int rc = umereg_knn_points_f32(pts, pts, 1, n, n, K, dists, idx, ws, w.knn_bytes, st)) return rc;
    const float rmax2 = max_radius * max_radius;
    const float s = (float)(65536.0 / ((double)max_radius * (double)max_radius));
    hipLaunchKernelGGL(eq_surfel_kernel, dim3((n + kEqWG - 1) / kEqWG), dim3(kEqWG), 0, st, pts, idx, dists, n, K, rmax2, s, normals, r2, q);
    UMEREG_CHECK_LAUNCH("eq_surfel_kernel");
    return UMEREG_OK;
}

static int eq_sample(const float* pts, const float* normals, const float* r2, const uint32_t* q, int n, int num_points, int knn,
                     uint32_t seed, float* samples, int64_t* src_index, float* rho2, uint64_t* total, char* ws, hipStream_t st)
{
    unsigned long long* Q = (unsigned long long*)ws;
    hipLaunchKernelGGL(eq_scan_kernel, dim3(1), dim3(kEqScanThreads), 0, st, q, n, Q, (unsigned long long*)total);
    UMEREG_CHECK_LAUNCH("eq_scan_kernel");
    const float c = (float)(0.5 * sqrt(3.14159265358979323846 / (double)eq_k(n, knn)));
    hipLaunchKernelGGL(eq_sample_kernel, dim3((num_points + kEqWG - 1) / kEqWG), dim3(kEqWG), 0, st, pts, normals, r2, Q, n, num_points,
                       seed, c, samples, src_index, rho2);
    UMEREG_CHECK_LAUNCH("eq_sample_kernel");
    return UMEREG_OK;
}

static int eq_project(const float* samples, const float* rho2, const float* pts, int num_points, int n, float* projected,
                      int32_t* nb_count, char* ws, hipStream_t st)
{
    if (int rc = launch_prep(pts, ws, 1, n, -1.0f, st)) return rc;      // kNN-mode grid for K = 1, the ICP's
    hipLaunchKernelGGL(eq_project_kernel, dim3((num_points + kEqPerWG - 1) / kEqPerWG), dim3(kEqWG), 0, st, samples, rho2, num_points,
                       (const char*)ws, n, projected, nb_count);
    UMEREG_CHECK_LAUNCH("eq_project_kernel");
    return UMEREG_OK;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_equalize_workspace_bytes(int n, int num_points, int knn)
{
    if (n <= 0 || num_points <= 0 || n > UMEREG_EQUALIZE_MAX_POINTS || num_points > UMEREG_EQUALIZE_MAX_POINTS ||
        knn < UMEREG_EQUALIZE_MIN_KNN || knn > UMEREG_EQUALIZE_MAX_KNN)
        return 0;
    return eq_ws(n, num_points, knn).total;
}

UMEREG_API int umereg_equalize_surfels_f32(const float* pts, int n, int knn, float max_radius, float* normals, float* r2, uint32_t* q,
                                           void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(pts && normals && r2 && q, "equalize_surfels: null pointer");
    if (int rc = eq_check("equalize_surfels", n, 1, knn)) return rc;
    if (int rc = eq_check_radius("equalize_surfels", max_radius)) return rc;
    if (int rc = check_device()) return rc;
    UMEREG_REQUIRE_WORKSPACE("equalize_surfels", workspace, workspace_bytes, umereg_equalize_workspace_bytes(n, 1, knn));
    return eq_surfels(pts, n, knn, max_radius, normals, r2, q, (char*)workspace, (hipStream_t)stream);
}

UMEREG_API int umereg_equalize_sample_f32(const float* pts, const float* normals, const float* r2, const uint32_t* q, int n, int num_points,
                                          int knn, uint32_t seed, float* samples, int64_t* src_index, float* rho2, uint64_t* total,
                                          void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(pts && normals && r2 && q && samples && src_index && rho2 && total, "equalize_sample: null pointer");
    if (int rc = eq_check("equalize_sample", n, num_points, knn)) return rc;
    if (int rc = eq_check_samplable("equalize_sample", n)) return rc;
    if (int rc = check_device()) return rc;
    UMEREG_REQUIRE_WORKSPACE("equalize_sample", workspace, workspace_bytes, umereg_equalize_workspace_bytes(n, 1, knn));
    return eq_sample(pts, normals, r2, q, n, num_points, knn, seed, samples, src_index, rho2, total, (char*)workspace, (hipStream_t)stream);
}

UMEREG_API int umereg_equalize_project_f32(const float* samples, const float* rho2, const float* pts, int num_points, int n,
                                           float* projected, int32_t* nb_count, void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(samples && rho2 && pts && projected, "equalize_project: null pointer");
    if (int rc = eq_check("equalize_project", n, num_points, UMEREG_EQUALIZE_MIN_KNN)) return rc;
    if (int rc = check_device()) return rc;
    UMEREG_REQUIRE_WORKSPACE("equalize_project", workspace, workspace_bytes,
                             umereg_equalize_workspace_bytes(n, 1, UMEREG_EQUALIZE_MIN_KNN));
    return eq_project(samples, rho2, pts, num_points, n, projected, nb_count, (char*)workspace, (hipStream_t)stream);
}

UMEREG_API int umereg_equalize_cloud_f32(const float* pts, int n, int num_points, int knn, float max_radius, int project, uint32_t seed,
                                         float* out, int64_t* src_index, uint64_t* total, void* workspace, size_t workspace_bytes,
                                         void* stream)
{
    UMEREG_REQUIRE(pts && out && src_index && total, "equalize_cloud: null pointer");
    if (int rc = eq_check("equalize_cloud", n, num_points, knn)) return rc;
    if (int rc = eq_check_radius("equalize_cloud", max_radius)) return rc;
    if (int rc = eq_check_samplable("equalize_cloud", n)) return rc;
    if (int rc = check_device()) return rc;
    UMEREG_REQUIRE_WORKSPACE("equalize_cloud", workspace, workspace_bytes, umereg_equalize_workspace_bytes(n, num_points, knn));
    char* ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const EqWs w = eq_ws(n, num_points, knn);
    float* normals = (float*)(ws + w.off_normals);
    float* r2 = (float*)(ws + w.off_r2);
    uint32_t* q = (uint32_t*)(ws + w.off_q);
    float* rho2 = (float*)(ws + w.off_rho2);
    float* samples = project ? (float*)(ws + w.off_samples) : out;
    if (int rc = eq_surfels(pts, n, knn, max_radius, normals, r2, q, ws, st)) return rc;
    if (int rc = eq_sample(pts, normals, r2, q, n, num_points, knn, seed, samples, src_index, rho2, total, ws, st)) return rc;
    if (project)
        if (int rc = eq_project(samples, rho2, pts, num_points, n, out, nullptr, ws, st)) return rc;
    return UMEREG_OK;
}
