/*
 * oracle/ume_oracle.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Plain-C CPU restatement of the heavy loops on UMERegRobust's registration hot
 * path.  It is the CHECKER for the HIP kernels, never the product: only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this file's
 * shared object.  The product (umeregrobust_amd/) never links, imports or calls
 * it and has no CPU fallback.
 *
 * Parity status
 *   - orc_ball_query_f32 restates pytorch3d==0.7.7 `ball_query` semantics
 *     (reference requirements.txt:3; pytorch3d is NOT vendored in /root/reference
 *     and is not installable here).  No test or golden vector in the reference
 *     pins it => "parity unpinned" at the pytorch3d boundary; the published
 *     semantics are restated below and every reference call site
 *     (evaluate.py:51, utils/loc_utils.py:38,72,100,...) is consistent with them.
 *   - everything downstream (moments, projector distance, RTUME solve) is pinned
 *     against the reference's own Python executed in the build container
 *     (oracle/gen_golden.py -> tests/golden/ npz files).
 *
 * Build: see oracle/Makefile (gcc -O2 -ffp-contract=off -fopenmp).
 * -ffp-contract=off matters: the fp32 squared distance must be formed as
 * ((dx*dx)+(dy*dy))+(dz*dz) with one rounding per operation, like the scalar C++
 * loop of pytorch3d's CPU path, or neighbourhood indices are not bit-exact.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORC_API __attribute__((visibility("default")))

/* --------------------------------------------------------------------------
 * a1  pytorch3d.ops.ball_query as called at reference evaluate.py:51
 *     (and utils/loc_utils.py:383-384).
 *
 * Semantics restated from pytorch3d 0.7.7 (csrc/ball_query/ball_query_cpu.cpp):
 *   idx initialised to -1, dists to 0;  for each query i < lengths1, scan
 *   j = 0 .. lengths2-1 in index order, dist2 = sum_d (p1[i][d]-p2[j][d])^2
 *   accumulated left to right in fp32, accept when dist2 < radius*radius
 *   (strict, radius2 formed in fp32), write slot `count`, stop at count == K.
 *   With return_nn=True the python wrapper gathers p2[idx] with -1 -> 0.
 * p1 [n1,3], p2 [n2,3] row-major fp32; idx i64 [n1,K]; dists [n1,K] or NULL;
 * nn [n1,K,3] or NULL.  One batch element per call.
 * -------------------------------------------------------------------------- */
ORC_API int orc_ball_query_f32(const float* p1, const float* p2, int64_t n1, int64_t n2,
                               int64_t len1, int64_t len2, int K, float radius,
                               int64_t* idx, float* dists, float* nn)
{
    const float r2 = radius * radius;
    if (len1 < 0 || len1 > n1) len1 = n1;
    if (len2 < 0 || len2 > n2) len2 = n2;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n1; ++i) {
        int64_t* oi = idx + i * K;
        for (int k = 0; k < K; ++k) oi[k] = -1;
        if (dists) memset(dists + i * K, 0, sizeof(float) * (size_t)K);
        if (nn) memset(nn + i * K * 3, 0, sizeof(float) * (size_t)K * 3);
        if (i >= len1) continue;
        const float qx = p1[3 * i], qy = p1[3 * i + 1], qz = p1[3 * i + 2];
        int cnt = 0;
        for (int64_t j = 0; j < len2 && cnt < K; ++j) {
            const float dx = qx - p2[3 * j];
            const float dy = qy - p2[3 * j + 1];
            const float dz = qz - p2[3 * j + 2];
            float d2 = dx * dx;
            d2 = d2 + dy * dy;
            d2 = d2 + dz * dz;
            if (d2 < r2) {
                oi[cnt] = j;
                if (dists) dists[i * K + cnt] = d2;
                if (nn) {
                    float* o = nn + (i * K + cnt) * 3;
                    o[0] = p2[3 * j]; o[1] = p2[3 * j + 1]; o[2] = p2[3 * j + 2];
                }
                ++cnt;
            }
        }
    }
    return 0;
}

/* --------------------------------------------------------------------------
 * a1, CONTRACTED form: the same scan with the squared distance as nvcc compiles pytorch3d's CUDA kernel
 * (csrc/ball_query/ball_query.cu: `dist2 += diff * diff` over the three coordinates, -fmad=true by default):
 *   d2 = fma(dz, dz, fma(dy, dy, dx * dx))
 * -- one rounding less per term than the CPU form above.  The reference's published numbers were produced by
 * this form (a CUDA build of pytorch3d); `north_star` asks for the CPU form, which is the default everywhere.
 * Checker of the opt-in UMEREG_BALL_FMA / UMEREG_MOMENTS_FMA_DIST modes of the library only.
 * -------------------------------------------------------------------------- */
ORC_API int orc_ball_query_fma_f32(const float* p1, const float* p2, int64_t n1, int64_t n2,
                                   int64_t len1, int64_t len2, int K, float radius,
                                   int64_t* idx, float* dists, float* nn)
{
    const float r2 = radius * radius;
    if (len1 < 0 || len1 > n1) len1 = n1;
    if (len2 < 0 || len2 > n2) len2 = n2;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n1; ++i) {
        int64_t* oi = idx + i * K;
        for (int k = 0; k < K; ++k) oi[k] = -1;
        if (dists) memset(dists + i * K, 0, sizeof(float) * (size_t)K);
        if (nn) memset(nn + i * K * 3, 0, sizeof(float) * (size_t)K * 3);
        if (i >= len1) continue;
        const float qx = p1[3 * i], qy = p1[3 * i + 1], qz = p1[3 * i + 2];
        int cnt = 0;
        for (int64_t j = 0; j < len2 && cnt < K; ++j) {
            const float dx = qx - p2[3 * j];
            const float dy = qy - p2[3 * j + 1];
            const float dz = qz - p2[3 * j + 2];
            const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));      /* (fmaf: correctly rounded whatever the target supports) */
            if (d2 < r2) {
                oi[cnt] = j;
                if (dists) dists[i * K + cnt] = d2;
                if (nn) {
                    float* o = nn + (i * K + cnt) * 3;
                    o[0] = p2[3 * j]; o[1] = p2[3 * j + 1]; o[2] = p2[3 * j + 2];
                }
                ++cnt;
            }
        }
    }
    return 0;
}

/* --------------------------------------------------------------------------
 * a1+a2  evaluate.py:50-60  my_ume_generation
 *   F1 = sum_k f_k p_k^T (32x3),  F0 = sum_k f_k (32x1),
 *   F = [F0,F1] / (sum_c F0[c] + 1e-6)                -> f32 [n_kp, d, 4]
 * over the ball-query neighbourhood above (absolute coordinates, not centred).
 *
 * accum = 0 : fp32 accumulation in neighbour order (one rounding per op), the
 *             arithmetic class of the reference (torch fp32 matmul / sum; its
 *             exact summation order is a BLAS detail and is not reproducible).
 * accum = 1 : fp64 accumulation + fp64 normalisation, rounded once to fp32
 *             ("truth-rounded"); this is what the HIP kernel computes.
 * nn_count (i32 [n_kp]) optional: number of neighbours used (<= K).
 * -------------------------------------------------------------------------- */
ORC_API int orc_ume_moments_f32(const float* pts, const float* kpts, const float* feat,
                                int64_t N, int64_t n_kp, int d, int K, float radius, int accum,
                                float* F, int32_t* nn_count)
{
    const float r2 = radius * radius;
    if (d > 64) return -1;
#pragma omp parallel
    {
        int64_t* list = (int64_t*)malloc(sizeof(int64_t) * (size_t)K);
#pragma omp for schedule(dynamic, 16)
        for (int64_t i = 0; i < n_kp; ++i) {
            const float qx = kpts[3 * i], qy = kpts[3 * i + 1], qz = kpts[3 * i + 2];
            int cnt = 0;
            for (int64_t j = 0; j < N && cnt < K; ++j) {
                const float dx = qx - pts[3 * j];
                const float dy = qy - pts[3 * j + 1];
                const float dz = qz - pts[3 * j + 2];
                float d2 = dx * dx;
                d2 = d2 + dy * dy;
                d2 = d2 + dz * dz;
                if (d2 < r2) list[cnt++] = j;
            }
            if (nn_count) nn_count[i] = cnt;
            float* Fo = F + i * d * 4;
            if (accum == 0) {
                float a[64][4];
                memset(a, 0, sizeof(a));
                for (int k = 0; k < cnt; ++k) {
                    const int64_t j = list[k];
                    const float x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
                    const float* f = feat + j * d;
                    for (int c = 0; c < d; ++c) {
                        a[c][0] = a[c][0] + f[c];
                        a[c][1] = a[c][1] + f[c] * x;
                        a[c][2] = a[c][2] + f[c] * y;
                        a[c][3] = a[c][3] + f[c] * z;
                    }
                }
                float s = 0.f;
                for (int c = 0; c < d; ++c) s = s + a[c][0];
                s = s + 1e-6f;
                for (int c = 0; c < d; ++c)
                    for (int m = 0; m < 4; ++m) Fo[c * 4 + m] = a[c][m] / s;
            } else {
                double a[64][4];
                memset(a, 0, sizeof(a));
                for (int k = 0; k < cnt; ++k) {
                    const int64_t j = list[k];
                    const double x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
                    const float* f = feat + j * d;
                    for (int c = 0; c < d; ++c) {
                        const double fc = f[c];
                        a[c][0] += fc;
                        a[c][1] += fc * x;
                        a[c][2] += fc * y;
                        a[c][3] += fc * z;
                    }
                }
                double s = 0.0;
                for (int c = 0; c < d; ++c) s += a[c][0];
                s += 1e-6;
                for (int c = 0; c < d; ++c)
                    for (int m = 0; m < 4; ++m) Fo[c * 4 + m] = (float)(a[c][m] / s);
            }
        }
        free(list);
    }
    return 0;
}

/* --------------------------------------------------------------------------
 * a3  utils/loc_utils.py:8-15  ume_cdist, fp64 "truth" form used to bound BOTH
 * the reference's fp32 result and the HIP kernel's:
 *   Q = orth(F) by Householder in fp64,  D = sqrt(max(4 - |Q1^T Q2|_F^2, 0))
 * (= |Q1Q1^T - Q2Q2^T|_F / sqrt(2) for rank-4 bases).
 * The reference-faithful fp32 projector/cdist restatement lives in oracle.py
 * (numpy LAPACK/BLAS, the same libraries torch CPU dispatches to).
 * -------------------------------------------------------------------------- */
static void householder_q_f64(const float* A32, int rows, double* Q /* rows x 4 */)
{
    /* LAPACK dgeqr2 + dorg2r conventions (H = I - tau v v^T, v[0] = 1, tau = 0 for a
       zero tail), so rank-deficient inputs degrade the same way torch.linalg.qr does. */
    double A[64][4], tau[4];
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < 4; ++c) A[r][c] = A32[r * 4 + c];
    for (int k = 0; k < 4; ++k) {
        double alpha = A[k][k], xn = 0.0;
        for (int r = k + 1; r < rows; ++r) xn += A[r][k] * A[r][k];
        xn = sqrt(xn);
        if (xn == 0.0) { tau[k] = 0.0; continue; }
        double beta = -copysign(hypot(alpha, xn), alpha);
        tau[k] = (beta - alpha) / beta;
        double sc = 1.0 / (alpha - beta);
        for (int r = k + 1; r < rows; ++r) A[r][k] *= sc;
        A[k][k] = beta;
        for (int c = k + 1; c < 4; ++c) {
            double w = A[k][c];
            for (int r = k + 1; r < rows; ++r) w += A[r][k] * A[r][c];
            w *= tau[k];
            A[k][c] -= w;
            for (int r = k + 1; r < rows; ++r) A[r][c] -= w * A[r][k];
        }
    }
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < 4; ++c) Q[r * 4 + c] = (r == c) ? 1.0 : 0.0;
    for (int k = 3; k >= 0; --k) {
        if (tau[k] == 0.0) continue;
        for (int c = 0; c < 4; ++c) {
            double w = Q[k * 4 + c];
            for (int r = k + 1; r < rows; ++r) w += A[r][k] * Q[r * 4 + c];
            w *= tau[k];
            Q[k * 4 + c] -= w;
            for (int r = k + 1; r < rows; ++r) Q[r * 4 + c] -= w * A[r][k];
        }
    }
}

ORC_API int orc_orthobasis_f64(const float* ume, int64_t n, int d, double* Q)
{
    if (d > 64) return -1;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) householder_q_f64(ume + i * d * 4, d, Q + i * d * 4);
    return 0;
}

ORC_API int orc_ume_cdist_f64(const float* ume1, const float* ume2, int64_t n1, int64_t n2, int d,
                              double* D /* [n1,n2] */)
{
    if (d > 64) return -1;
    double* Q1 = (double*)malloc(sizeof(double) * (size_t)(n1 * d * 4));
    double* Q2 = (double*)malloc(sizeof(double) * (size_t)(n2 * d * 4));
    if (!Q1 || !Q2) { free(Q1); free(Q2); return -2; }
    orc_orthobasis_f64(ume1, n1, d, Q1);
    orc_orthobasis_f64(ume2, n2, d, Q2);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n1; ++i) {
        const double* a = Q1 + i * d * 4;
        for (int64_t j = 0; j < n2; ++j) {
            const double* b = Q2 + j * d * 4;
            double s = 0.0;
            for (int p = 0; p < 4; ++p)
                for (int q = 0; q < 4; ++q) {
                    double c = 0.0;
                    for (int r = 0; r < d; ++r) c += a[r * 4 + p] * b[r * 4 + q];
                    s += c * c;
                }
            double v = 4.0 - s;
            D[i * n2 + j] = v > 0.0 ? sqrt(v) : 0.0;
        }
    }
    free(Q1); free(Q2);
    return 0;
}

/* --------------------------------------------------------------------------
 * a3+a4 without the matrix: the fp64 truth of orc_ume_cdist_f64 reduced per row,
 * so that a 10 000 x 10 000 match can be checked in O(n1 + n2) memory.
 * Per row i, over all columns j of D2[i,j] = max(4 - |Q1_i^T Q2_j|_F^2, 0) (the
 * same statements, in the same order, as orc_ume_cdist_f64 -- D = sqrt(D2) there):
 *   argmin[i]  first j of the row minimum (= np.argmin of that row),
 *   d2min[i]   the smallest D2, d2sec[i] the second smallest (a duplicate of the
 *              minimum counts: an exact tie gives d2sec == d2min; +inf if n2 == 1),
 *   d_at[i]    D[i, cols[i]] (optional; cols NULL -> d_at untouched).
 * -------------------------------------------------------------------------- */
ORC_API int orc_ume_match_f64(const float* ume1, const float* ume2, int64_t n1, int64_t n2, int d,
                              const int64_t* cols, int64_t* argmin, double* d2min, double* d2sec, double* d_at)
{
    if (d > 64 || n1 < 0 || n2 < 1) return -1;
    if (cols)
        for (int64_t i = 0; i < n1; ++i)
            if (cols[i] < 0 || cols[i] >= n2) return -3;
    double* Q1 = (double*)malloc(sizeof(double) * (size_t)(n1 * d * 4 + 1));
    double* Q2 = (double*)malloc(sizeof(double) * (size_t)(n2 * d * 4));
    if (!Q1 || !Q2) { free(Q1); free(Q2); return -2; }
    orc_orthobasis_f64(ume1, n1, d, Q1);
    orc_orthobasis_f64(ume2, n2, d, Q2);
#pragma omp parallel for schedule(dynamic, 8)
    for (int64_t i = 0; i < n1; ++i) {
        const double* a = Q1 + i * d * 4;
        double b1 = INFINITY, b2 = INFINITY;
        int64_t bj = 0;
        for (int64_t j = 0; j < n2; ++j) {
            const double* b = Q2 + j * d * 4;
            double s = 0.0;
            for (int p = 0; p < 4; ++p)
                for (int q = 0; q < 4; ++q) {
                    double c = 0.0;
                    for (int r = 0; r < d; ++r) c += a[r * 4 + p] * b[r * 4 + q];
                    s += c * c;
                }
            double v = 4.0 - s;
            v = v > 0.0 ? v : 0.0;
            if (v < b1) { b2 = b1; b1 = v; bj = j; }
            else if (v < b2) b2 = v;
            if (cols && j == cols[i] && d_at) d_at[i] = sqrt(v);
        }
        argmin[i] = bj;
        d2min[i] = b1;
        d2sec[i] = b2;
    }
    free(Q1); free(Q2);
    return 0;
}

/* --------------------------------------------------------------------------
 * f1 support: pytorch3d.ops.knn_points (K nearest, squared distances, ascending;
 * ties -> lower index first -- upstream tie order is unspecified, parity unpinned)
 * as called at utils/loc_utils.py:580,623 and evaluate.py:272,274.
 * p1 [n1,3], p2 [n2,3]; dists f32 [n1,K]; idx i64 [n1,K].  Requires K <= n2.
 * -------------------------------------------------------------------------- */
ORC_API int orc_knn_points_f32(const float* p1, const float* p2, int64_t n1, int64_t n2, int K,
                               float* dists, int64_t* idx)
{
    if (K > n2 || K > 256) return -1;
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < n1; ++i) {
        float bd[256]; int64_t bi[256]; int cnt = 0;
        const float qx = p1[3 * i], qy = p1[3 * i + 1], qz = p1[3 * i + 2];
        for (int64_t j = 0; j < n2; ++j) {
            const float dx = qx - p2[3 * j];
            const float dy = qy - p2[3 * j + 1];
            const float dz = qz - p2[3 * j + 2];
            float d2 = dx * dx;
            d2 = d2 + dy * dy;
            d2 = d2 + dz * dz;
            if (cnt == K && !(d2 < bd[K - 1])) continue;
            int p = cnt < K ? cnt : K - 1;
            while (p > 0 && bd[p - 1] > d2) { bd[p] = bd[p - 1]; bi[p] = bi[p - 1]; --p; }
            bd[p] = d2; bi[p] = j;
            if (cnt < K) ++cnt;
        }
        for (int k = 0; k < K; ++k) { dists[i * K + k] = bd[k]; idx[i * K + k] = bi[k]; }
    }
    return 0;
}

/* The K smallest (d2, index) of the fp32 squared distances ((dx*dx) + (dy*dy)) + (dz*dz) from q to tp[0..Nt), ascending
 * (ties -> lower index): the brute-force selection of orc_pc_corr_cost_f32 and orc_corr_judge_f32.  -> how many (min(K, Nt)). */
static int knn_select_f32(const float* q, const float* tp, int64_t Nt, int K, float* bd, int64_t* bi)
{
    int cnt = 0;
    for (int64_t j = 0; j < Nt; ++j) {
        const float dx = q[0] - tp[3 * j];
        const float dy = q[1] - tp[3 * j + 1];
        const float dz = q[2] - tp[3 * j + 2];
        float d2 = dx * dx;
        d2 = d2 + dy * dy;
        d2 = d2 + dz * dz;
        if (cnt == K && !(d2 < bd[K - 1])) continue;
        int p = cnt < K ? cnt : K - 1;
        while (p > 0 && bd[p - 1] > d2) { bd[p] = bd[p - 1]; bi[p] = bi[p - 1]; --p; }
        bd[p] = d2; bi[p] = j;
        if (cnt < K) ++cnt;
    }
    return cnt;
}

/* --------------------------------------------------------------------------
 * f1: pc_corr_cost_pytorch3d -> pc_corr_pytorch3d -> pc_corr (reference utils/loc_utils.py:592-637, P=None,
 * use_norm=False) for M hypotheses in one call -- the same arithmetic as oracle.py's numpy restatement
 * (pc_corr_cost, pinned to golden G7), written as loops so that the CPU baseline / recall check of bench.py can
 * afford thousands of hypotheses:
 *   source_transformed = p R^T + t                                   (:629)
 *   q_nn_to_p = knn_points(source_transformed, target, K)            (:623; ties -> lower index, see above)
 *   dist = |p' - q_nn|, weight = 1 / (1 + (dist / sigma)^2)          (:593, :588-589, :596)
 *   val = sum_c vals_p[n][c] * vals_q[nn][c]                         (:603)
 *   score = sum_{n,k} weight * val / Ns                              (:610, :612)
 * T [M,4,4] row-major fp32 (rotation block + translation column); sp [Ns,3]; tp [Nt,3]; vp [Ns,d]; vq [Nt,d].
 * The per-point terms are fp32 like the reference's; the final sum over (n,k) is accumulated in fp64 (the
 * reference's fp32 torch.sum is a pairwise reduction whose order is not reproducible; tests bound the difference).
 * -------------------------------------------------------------------------- */
ORC_API int orc_pc_corr_cost_f32(const float* T, int64_t M, const float* sp, int64_t Ns, const float* tp, int64_t Nt,
                                 const float* vp, const float* vq, int d, int K, float sigma, float* scores)
{
    if (K > Nt || K > 256 || K < 1) return -1;
    double* per_point = (double*)malloc(sizeof(double) * (size_t)(M * Ns));
    if (!per_point) return -2;
#pragma omp parallel for schedule(dynamic, 32)
    for (int64_t w = 0; w < M * Ns; ++w) {
        const int64_t h = w / Ns, n = w % Ns;
        const float* Th = T + h * 16;
        const float x = sp[3 * n], y = sp[3 * n + 1], z = sp[3 * n + 2];
        float q[3];
        for (int a = 0; a < 3; ++a) {
            float v = Th[4 * a] * x;
            v = v + Th[4 * a + 1] * y;
            v = v + Th[4 * a + 2] * z;
            q[a] = v + Th[4 * a + 3];
        }
        float bd[256]; int64_t bi[256];
        const int cnt = knn_select_f32(q, tp, Nt, K, bd, bi);
        double s = 0.0;
        for (int k = 0; k < cnt; ++k) {
            const float dist = sqrtf(bd[k]);
            const float r = dist / sigma;
            const float wgt = 1.0f / (1.0f + r * r);
            const float* a = vp + n * d;
            const float* b = vq + bi[k] * d;
            float val = 0.f;
            for (int c = 0; c < d; ++c) val = val + a[c] * b[c];
            s += (double)(wgt * val);
        }
        per_point[w] = s;
    }
    for (int64_t h = 0; h < M; ++h) {
        double s = 0.0;
        for (int64_t n = 0; n < Ns; ++n) s += per_point[h * Ns + n];
        scores[h] = (float)(s / (double)Ns);
    }
    free(per_point);
    return 0;
}

/* --------------------------------------------------------------------------
 * f1, judged per neighbour: the images, neighbour sets and exact sums of pc_corr_cost for a chosen subset of hypotheses.
 *
 * form 0  the reference form of orc_pc_corr_cost_f32:  q = ((T0 x + T1 y) + T2 z) + T3, one rounding per operation;
 * form 1  the form of every HIP route (corr_leftover.hip, corr_lattice.hip, corr_consensus.hip):
 *             q = fmaf(T2, z, fmaf(T1, y, T0 * x)) + T3          (fmaf: correctly rounded, whatever the target supports)
 * Then d2 = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32 and the K smallest by (d2, index): ties -> lower index.  Both are defined
 * fp32 functions, so the neighbour sets are bit-exact.
 *
 * orc_corr_images_f32:   q [M,Ns,3] of the chosen form.
 * orc_corr_judge_f32:    per hypothesis h (brute force, Ns x Nt per hypothesis):
 *   idx [M,Ns,K] i64, d2 [M,Ns,K] f32 (either may be NULL)  the neighbour sets, ascending by (d2, index);
 *   label [M] f64   sum over (n,k) of <vp[n], vq[nn]> in fp64: the exact integer when the features are small integers;
 *   score [M] f64   sum over (n,k) of w * <vp, vq> / Ns, w = 1 / (1 + d2 / sigma^2) from the fp32 d2, everything in fp64;
 *   absum [M] f64   sum over (n,k) of w * sum_c |vp_c vq_c| (the magnitude that bounds fp32 rounding of the same sum).
 * T [M,4,4] row-major fp32; sp [Ns,3]; tp [Nt,3]; vp [Ns,d]; vq [Nt,d].  K <= min(Nt, 256).
 * -------------------------------------------------------------------------- */
static inline void corr_image(const float* Th, const float* p, int form, float* q)
{
    for (int a = 0; a < 3; ++a) {
        if (form == 1) {
            q[a] = fmaf(Th[4 * a + 2], p[2], fmaf(Th[4 * a + 1], p[1], Th[4 * a] * p[0])) + Th[4 * a + 3];
        } else {
            float v = Th[4 * a] * p[0];
            v = v + Th[4 * a + 1] * p[1];
            v = v + Th[4 * a + 2] * p[2];
            q[a] = v + Th[4 * a + 3];
        }
    }
}

ORC_API int orc_corr_images_f32(const float* T, int64_t M, const float* sp, int64_t Ns, int form, float* q)
{
    if (form != 0 && form != 1) return -1;
#pragma omp parallel for schedule(static)
    for (int64_t w = 0; w < M * Ns; ++w) corr_image(T + (w / Ns) * 16, sp + 3 * (w % Ns), form, q + 3 * w);
    return 0;
}

ORC_API int orc_corr_judge_f32(const float* T, int64_t M, const float* sp, int64_t Ns, const float* tp, int64_t Nt,
                               const float* vp, const float* vq, int d, int K, double sigma, int form,
                               int64_t* idx, float* d2out, double* label, double* score, double* absum)
{
    if (K > Nt || K > 256 || K < 1 || (form != 0 && form != 1)) return -1;
    double* acc = (double*)malloc(sizeof(double) * (size_t)(M * Ns) * 3);
    if (!acc) return -2;
    const double inv_s2 = 1.0 / (sigma * sigma);
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t w = 0; w < M * Ns; ++w) {
        const int64_t h = w / Ns, n = w % Ns;
        float q[3];
        corr_image(T + h * 16, sp + 3 * n, form, q);
        float bd[256]; int64_t bi[256];
        const int cnt = knn_select_f32(q, tp, Nt, K, bd, bi);
        double lab = 0.0, s = 0.0, a = 0.0;
        for (int k = 0; k < cnt; ++k) {
            const float* x = vp + n * d;
            const float* y = vq + bi[k] * d;
            double val = 0.0, mag = 0.0;
            for (int c = 0; c < d; ++c) {
                const double t = (double)x[c] * (double)y[c];          /* exact: a product of two floats */
                val += t;
                mag += fabs(t);
            }
            const double wgt = 1.0 / (1.0 + (double)bd[k] * inv_s2);
            lab += val;
            s += wgt * val;
            a += wgt * mag;
        }
        for (int k = 0; k < K; ++k) {
            if (idx) idx[w * K + k] = k < cnt ? bi[k] : -1;
            if (d2out) d2out[w * K + k] = k < cnt ? bd[k] : NAN;
        }
        acc[3 * w] = lab; acc[3 * w + 1] = s; acc[3 * w + 2] = a;
    }
    for (int64_t h = 0; h < M; ++h) {
        double lab = 0.0, s = 0.0, a = 0.0;
        for (int64_t n = 0; n < Ns; ++n) {
            lab += acc[3 * (h * Ns + n)];
            s += acc[3 * (h * Ns + n) + 1];
            a += acc[3 * (h * Ns + n) + 2];
        }
        if (label) label[h] = lab;
        if (score) score[h] = s / (double)Ns;
        if (absum) absum[h] = a;
    }
    free(acc);
    return 0;
}

/* --------------------------------------------------------------------------
 * a3+a4 as the "f16r" matcher's refine pass computes it (match_f16r.hip,
 * match_refine_kernel), restated term for term on the split-f16 planes the
 * library itself wrote (oracle.decode_split_f16):
 *   qa[i]  [32,4]  row i's basis as the refine holds it: (double)hi + (double)lo,
 *   vb[j]  [32,4]  column j's basis as the refine reads it: (double)((float)hi + (float)lo),
 *   dot[a][b] = fma(qa[k][a], vb[k][b], dot[a][b]) for k = 0..31 in order,
 *   s = fma(dot[a][b], dot[a][b], s) for a = 0..3, b = 0..3 (b inner),
 *   d2 = (float)fmax(4 - s, 0), key = (bits(d2), j), the minimum key wins:
 *   ties in fp32 go to the lower index.
 * Per row i:
 *   argmin[i], key[i]          the winning j and its d2 (fp32),
 *   arg2[i], key2[i]           the runner-up by the same key (n2 == 1: -1, +inf),
 *   d64[i], d64sec[i]          fmax(4 - s, 0) in fp64 at argmin[i], and its minimum over every other j,
 *   coarse_win[i], coarse_max[i] (ah, bh non-NULL) the hi-only score sum_ab (sum_k hi[k][a] hi[k][b])^2
 *                              (fp64; the products are exact) at argmin[i], and its row maximum.
 * fma() must round once: the hot loop is compiled for the FMA unit when the host has one
 * and calls libm's (correctly rounded) fma otherwise.
 * -------------------------------------------------------------------------- */
#define ORC_SPLIT_ROW_BODY(FMA)                                                                  \
    do {                                                                                         \
        const double* a = qa + i * 128;                                                          \
        const double* ha = ah ? ah + i * 128 : NULL;                                             \
        uint64_t bk = UINT64_MAX, bk2 = UINT64_MAX;                                              \
        double bd64 = INFINITY, sec64 = INFINITY, cmax = -INFINITY, cwin = 0.0;                  \
        for (int64_t j = 0; j < n2; ++j) {                                                       \
            const double* b = vb + j * 128;                                                      \
            double dot[4][4] = {{0.0}};                                                          \
            for (int k = 0; k < 32; ++k)                                                         \
                for (int bb = 0; bb < 4; ++bb)                                                   \
                    for (int aa = 0; aa < 4; ++aa) dot[aa][bb] = FMA(a[k * 4 + aa], b[k * 4 + bb], dot[aa][bb]); \
            double s = 0.0;                                                                      \
            for (int aa = 0; aa < 4; ++aa)                                                       \
                for (int bb = 0; bb < 4; ++bb) s = FMA(dot[aa][bb], dot[aa][bb], s);             \
            const double v = fmax(4.0 - s, 0.0);                                                 \
            const float f = (float)v;                                                            \
            uint32_t fb;                                                                         \
            memcpy(&fb, &f, 4);                                                                  \
            const uint64_t key = ((uint64_t)fb << 32) | (uint64_t)j;                             \
            double c = 0.0;                                                                      \
            if (ha) {                                                                            \
                const double* hb = bh + j * 128;                                                 \
                for (int aa = 0; aa < 4; ++aa)                                                   \
                    for (int bb = 0; bb < 4; ++bb) {                                             \
                        double e = 0.0;                                                          \
                        for (int k = 0; k < 32; ++k) e += ha[k * 4 + aa] * hb[k * 4 + bb];       \
                        c += e * e;                                                              \
                    }                                                                            \
                if (c > cmax) cmax = c;                                                          \
            }                                                                                    \
            if (key < bk) {                                                                      \
                bk2 = bk; bk = key;                                                              \
                sec64 = fmin(sec64, bd64); bd64 = v; cwin = c;                                   \
            } else {                                                                             \
                if (key < bk2) bk2 = key;                                                        \
                sec64 = fmin(sec64, v);                                                          \
            }                                                                                    \
        }                                                                                        \
        argmin[i] = (int64_t)(bk & 0xffffffffu);                                                 \
        uint32_t kb = (uint32_t)(bk >> 32);                                                      \
        memcpy(&key1[i], &kb, 4);                                                                \
        if (bk2 == UINT64_MAX) { arg2[i] = -1; key2[i] = INFINITY; }                             \
        else { arg2[i] = (int64_t)(bk2 & 0xffffffffu); kb = (uint32_t)(bk2 >> 32); memcpy(&key2[i], &kb, 4); } \
        d64[i] = bd64;                                                                           \
        d64sec[i] = sec64;                                                                       \
        if (ha) { coarse_win[i] = cwin; coarse_max[i] = cmax; }                                  \
    } while (0)

#define ORC_SPLIT_ARGS const double* qa, const double* vb, const double* ah, const double* bh, int64_t n1, int64_t n2, \
    int64_t* argmin, float* key1, int64_t* arg2, float* key2, double* d64, double* d64sec, double* coarse_win, double* coarse_max

__attribute__((target("fma,avx2"), optimize("O3"))) static void orc_match_split_rows_fma(ORC_SPLIT_ARGS)
{
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t i = 0; i < n1; ++i) ORC_SPLIT_ROW_BODY(__builtin_fma);
}

static void orc_match_split_rows_libm(ORC_SPLIT_ARGS)
{
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t i = 0; i < n1; ++i) ORC_SPLIT_ROW_BODY(fma);
}

ORC_API int orc_match_split_f64(ORC_SPLIT_ARGS)
{
    if (n1 < 0 || n2 < 1 || n2 >= ((int64_t)1 << 32) || (ah == NULL) != (bh == NULL)) return -1;
    if (ah && (!coarse_win || !coarse_max)) return -1;
    __builtin_cpu_init();
    if (__builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2")) orc_match_split_rows_fma(qa, vb, ah, bh, n1, n2, argmin, key1, arg2, key2, d64, d64sec, coarse_win, coarse_max);
    else orc_match_split_rows_libm(qa, vb, ah, bh, n1, n2, argmin, key1, arg2, key2, d64, d64sec, coarse_win, coarse_max);
    return 0;
}
