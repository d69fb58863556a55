// ume_grad.hip -- backward passes of the UME moment matrix and of the subspace distance (include/umereg_ume_grad.h):
// what UMEContrastiveLoss (reference loss.py:49-118) needs below torch's autograd.
//
// ---- moments ---------------------------------------------------------------------------------------------------------
// dfeat[j] = (sum_{i : j in N(i)} Gr_i) . [1, p_j].  Three kernels:
//   mom_rowsum_kernel    rs[j] = sum_c feat[j][c]                                  (normalised form only; fp64)
//   mom_gr_kernel        one wave per keypoint: the valid length of its list and the bounding box of the listed points,
//                        s_i = sum_{j in N(i)} rs[j], Gr_i (fp64 [32][4])
//   mom_scatter_kernel   one wave per POINT j: 64 keypoints at a time test "j in N(i)" (p_j inside the list's box first -- a
//                        necessary condition by construction, no radius involved -- then a binary search of the ascending
//                        list the forward wrote), and the members' Gr_i are added in ascending i.
// No inverse list is built and nothing is added atomically: the order of every sum is the keypoint order.
//
// ---- subspace distance -----------------------------------------------------------------------------------------------
// M1_i = sum_j w_ij Q2_j (Q2_j^T Q1_i).  With A = Q1 as [4 n1][32] (row 4 i + a = column a of Q1_i) and B = Q2 as [4 n2][32]:
//   S^T = B A^T (32 x 32 tile: rows (j, b), columns (i, a)),  S'^T = S^T scaled by w_ij per 4 x 4 block,  M^T += B^T S'^T.
// v_mfma_f32_32x32x2_f32 (A[i = l&31][k = l>>5], B[k = l>>5][j = l&31], C row = (reg&3) + 8 (reg>>2) + 4 (l>>5), col = l&31):
// the accumulator of the first product, register r of lane l, is S^T[row 8 (r>>2) + 4 (l>>5) + (r&3)][col l&31] -- exactly
// the B operand (k = that row, for the lane's half) of a second MFMA whose A operand is B^T[d = l&31][k].  So the 16
// registers of S'^T feed the second product as they are: no LDS, no cross-lane move.  The 4 x 4 block of a register is
// j_local = 2 (r>>2) + (l>>5), i_local = (l&31)>>2: four weights per lane and tile.
// A wave keeps kRowTiles tiles of A (their B operands of the first product, 16 registers each) and the matching M^T
// accumulators, and streams tiles of B (the next tile is fetched while the current one is multiplied), read once as [32][4 n2] (first product: A operand, coalesced over (j, b)) and once
// as [4 n2][32] (second product: A operand, coalesced over d).  The column range is cut into splits (a function of the
// sizes only); the partial M of a split goes to scratch and the finish adds the splits in order, in fp64.
//   cdist_prep_kernel    fp64 Householder Q (householder.h) and R = Q^T F per keypoint; Q as f32 in both orders, Q and R fp64
//   cdist_bwd_kernel     the contraction above
//   cdist_finish_kernel  dF = -2 (M - Q Q^T M) R^{-T} per keypoint, fp64, one 32-lane group per keypoint (lane = row)
#include "common.h"
#include "householder.h"
#include "ume_grad_plan.h"
#include "umereg_ume_grad.h"

namespace umereg {

using f32x16g = __attribute__((ext_vector_type(16))) float;

constexpr int kGradWaves = 4;      // waves per workgroup (kRowTiles, kRowKp: ume_grad_plan.h)

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += shfl_xor_f64(v, m);
    return v;
}

// ---- moments ---------------------------------------------------------------------------------------------------------

__global__ void mom_rowsum_kernel(const float* __restrict__ feat, size_t rows, double* __restrict__ rs)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= rows) return;
    const float4* f = (const float4*)(feat + j * 32);
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float4 v = f[q];
        s += (double)v.x; s += (double)v.y; s += (double)v.z; s += (double)v.w;
    }
    rs[j] = s;
}

// box[2 bi] = {min x, y, z of the listed points, valid length as bits}, box[2 bi + 1] = {max x, y, z, 0} (an empty list: +inf / -inf)
__global__ __launch_bounds__(kWave* kGradWaves) void mom_gr_kernel(const float* __restrict__ pts, const int64_t* __restrict__ nn_idx,
                                                                  const float* __restrict__ F, const float* __restrict__ dF,
                                                                  const double* __restrict__ rs, int N, int n, int K,
                                                                  size_t n_lists, int normalize, float4* __restrict__ box,
                                                                  double* __restrict__ Gr)
{
    const size_t bi = (size_t)blockIdx.x * kGradWaves + (threadIdx.x >> 6);
    if (bi >= n_lists) return;
    const int lane = lane_id();
    const int64_t* row = nn_idx + bi * K;
    const size_t b = bi / n;
    int cnt = 0;
    double s = 0.0;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int e = lane; e < K; e += kWave) {
        const int64_t j = row[e];
        if (j >= 0 && j < N) {
            ++cnt;
            if (normalize) s += rs[b * N + j];
            const float* p = pts + (b * N + j) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mn[k] = fminf(mn[k], p[k]);
                mx[k] = fmaxf(mx[k], p[k]);
            }
        }
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        cnt += __shfl_xor(cnt, m, kWave);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], m, kWave));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], m, kWave));
        }
    }
    if (lane == 0) {
        box[2 * bi] = make_float4(mn[0], mn[1], mn[2], __int_as_float(cnt));
        box[2 * bi + 1] = make_float4(mx[0], mx[1], mx[2], 0.f);
    }
    const float2 g = ((const float2*)(dF + bi * 128))[lane];     // entries 2 lane, 2 lane + 1: channel lane>>1, columns 2 (lane&1) + {0, 1}
    double g0 = g.x, g1 = g.y;
    if (normalize) {
        s = wave_sum_f64(s);
        const float2 f = ((const float2*)(F + bi * 128))[lane];
        const double inner = wave_sum_f64(g0 * (double)f.x + g1 * (double)f.y);
        const double inv = 1.0 / (s + 1e-6);
        g0 *= inv;
        g1 *= inv;
        if ((lane & 1) == 0) g0 -= inner * inv;
    }
    ((double2*)(Gr + bi * 128))[lane] = make_double2(g0, g1);
}

__global__ __launch_bounds__(kWave* kGradWaves) void mom_scatter_kernel(const float* __restrict__ pts,
                                                                       const int64_t* __restrict__ nn_idx,
                                                                       const float4* __restrict__ box,
                                                                       const double* __restrict__ Gr, int N, int n, int K,
                                                                       size_t n_points, float* __restrict__ dfeat)
{
    const size_t bj = (size_t)blockIdx.x * kGradWaves + (threadIdx.x >> 6);
    if (bj >= n_points) return;
    const int lane = lane_id();
    const size_t b = bj / N;
    const int j = (int)(bj - b * N);
    const float* p = pts + bj * 3;
    const float px = p[0], py = p[1], pz = p[2];
    double a0 = 0.0, a1 = 0.0;
    for (int i0 = 0; i0 < n; i0 += kWave) {
        const int i = i0 + lane;
        bool member = false;
        if (i < n) {
            const float4 bl = box[2 * (b * n + i)], bh = box[2 * (b * n + i) + 1];
            if (px >= bl.x && px <= bh.x && py >= bl.y && py <= bh.y && pz >= bl.z && pz <= bh.z) {     // (never an empty list)
                const int64_t* row = nn_idx + (b * n + i) * K;
                int lo = 0, hi = __float_as_int(bl.w) - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (row[mid] < j) lo = mid + 1; else hi = mid;
                }
                member = row[lo] == j;
            }
        }
        unsigned long long mask = __ballot(member);
        while (mask) {
            const int t = __builtin_ctzll(mask);
            mask &= mask - 1;
            const double2 g = ((const double2*)(Gr + (b * n + i0 + t) * 128))[lane];
            a0 += g.x;
            a1 += g.y;
        }
    }
    const double h0 = (lane & 1) ? (double)py : 1.0;
    const double h1 = (lane & 1) ? (double)pz : (double)px;
    const double v = a0 * h0 + a1 * h1;
    const double o = shfl_xor_f64(v, 1);
    if ((lane & 1) == 0) dfeat[bj * 32 + (lane >> 1)] = (float)(v + o);
}

// ---- subspace distance -----------------------------------------------------------------------------------------------

// one 32-lane group per keypoint slot i in [0, np): lane = row d.  Slots >= n are zero padding of the f32 bases.
__global__ __launch_bounds__(kWave* kGradWaves) void cdist_prep_kernel(const float* __restrict__ ume, int n, int np,
                                                                      float* __restrict__ Qrow, float* __restrict__ Qcol,
                                                                      double* __restrict__ Q64, double* __restrict__ R64)
{
    const int i = (blockIdx.x * (kWave * kGradWaves) + threadIdx.x) >> 5;
    if (i >= np) return;
    const int d = threadIdx.x & 31;
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const float4 f = ((const float4*)ume)[(size_t)i * 32 + d];
        const double a[4] = {f.x, f.y, f.z, f.w};
        householder_q_32x4(a, q, d);
        // R = Q^T F (upper triangular up to rounding; the finish reads the upper triangle)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double v = group32_sum(q[r] * a[c]);
                if (d == 0) R64[(size_t)i * 16 + r * 4 + c] = v;
            }
        ((double4*)Q64)[(size_t)i * 32 + d] = make_double4(q[0], q[1], q[2], q[3]);
    }
    const size_t ld = (size_t)4 * np;
#pragma unroll
    for (int a = 0; a < 4; ++a) Qrow[((size_t)4 * i + a) * 32 + d] = (float)q[a];
    *(float4*)(Qcol + (size_t)d * ld + 4 * i) = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
}

// Arow: [4 npA][32] of the side whose gradient this is; Brow [4 npB][32] / Bcol [32][ldb = 4 npB] of the other side.
// weight of (i, j): W[i * si + j * sj] of D and dD (si, sj = n2, 1 for side 1; 1, n2 for side 2).
__global__ __launch_bounds__(kWave* kGradWaves) void cdist_bwd_kernel(const float* __restrict__ Arow, const float* __restrict__ Brow,
                                                                     const float* __restrict__ Bcol, int ldb,
                                                                     const float* __restrict__ D, const float* __restrict__ dD,
                                                                     size_t si, size_t sj, int nA, int nB, int n_rt, int n_jt,
                                                                     int tiles_per_split, int n_work, float* __restrict__ Mpart,
                                                                     size_t part_stride)
{
    const int w = blockIdx.x * kGradWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= n_work) return;
    const int lane = lane_id();
    const int c = lane & 31, h = lane >> 5;
    const int rt = w % n_rt, sp = w / n_rt;
    const int jt0 = sp * tiles_per_split;
    const int jt1 = min(jt0 + tiles_per_split, n_jt);

    // B operands of the first product: A^T[d = 16 h + s][col c] of each kept tile (the contraction runs over d in the order
    // s = 0..15 with the lane half picking d = s or 16 + s; both operands use the same order)
    float qa[kRowTiles][16];
#pragma unroll
    for (int t = 0; t < kRowTiles; ++t) {
        const float4* src = (const float4*)(Arow + ((size_t)(rt * kRowTiles + t) * 32 + c) * 32 + 16 * h);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = src[q];
            qa[t][4 * q + 0] = v.x; qa[t][4 * q + 1] = v.y; qa[t][4 * q + 2] = v.z; qa[t][4 * q + 3] = v.w;
        }
    }
    f32x16g mt[kRowTiles];
#pragma unroll
    for (int t = 0; t < kRowTiles; ++t) mt[t] = f32x16g{0};

    // the operands of a tile of B and the D / dD entries of its 4 x 4 blocks; tile jt + 1 is fetched while tile jt is multiplied
    struct Tile {
        float b1[16], b2[16], dv[kRowTiles][4], gv[kRowTiles][4];
    };
    auto fetch = [&](int jt, Tile& T) {
#pragma unroll
        for (int s = 0; s < 16; ++s) T.b1[s] = Bcol[(size_t)(16 * h + s) * ldb + jt * 32 + c];
#pragma unroll
        for (int r = 0; r < 16; ++r) T.b2[r] = Brow[((size_t)jt * 32 + 8 * (r >> 2) + 4 * h + (r & 3)) * 32 + c];
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) {
            const int i = (rt * kRowTiles + t) * 8 + (c >> 2);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = jt * 8 + 2 * q + h;
                const bool in = i < nA && j < nB;
                const size_t o = in ? (size_t)i * si + (size_t)j * sj : 0;
                const float dist = D[o], g = dD[o];
                T.dv[t][q] = in ? dist : 0.f;      // outside the matrix: no weight
                T.gv[t][q] = g;
            }
        }
    };
    Tile cur, nxt;
    fetch(jt0, cur);
    for (int jt = jt0; jt < jt1; ++jt) {
        fetch(min(jt + 1, jt1 - 1), nxt);
        f32x16g st[kRowTiles];
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t) st[t] = f32x16g{0};
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) st[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.b1[s], qa[t][s], st[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < kRowTiles; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float wij = cur.dv[t][q] > UMEREG_UME_CDIST_BWD_DMIN ? cur.gv[t][q] / (2.0f * cur.dv[t][q]) : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) st[t][4 * q + r] *= wij;
            }
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int t = 0; t < kRowTiles; ++t) mt[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.b2[r], st[t][r], mt[t], 0, 0, 0);
        cur = nxt;
    }

    // M^T register r of lane l: d = 8 (r>>2) + 4 h + (r&3), row (i, a) = c of tile t
#pragma unroll
    for (int t = 0; t < kRowTiles; ++t) {
        float* dst = Mpart + (size_t)sp * part_stride + ((size_t)(rt * kRowTiles + t) * 32 + c) * 32 + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(float4*)(dst + 8 * q) = make_float4(mt[t][4 * q + 0], mt[t][4 * q + 1], mt[t][4 * q + 2], mt[t][4 * q + 3]);
    }
}

__global__ __launch_bounds__(kWave* kGradWaves) void cdist_finish_kernel(const float* __restrict__ Mpart, size_t part_stride,
                                                                        int splits, const double* __restrict__ Q64,
                                                                        const double* __restrict__ R64, int n,
                                                                        float* __restrict__ dume)
{
    const int i = (blockIdx.x * (kWave * kGradWaves) + threadIdx.x) >> 5;
    if (i >= n) return;
    const int d = threadIdx.x & 31;
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < splits; ++s)
#pragma unroll
        for (int a = 0; a < 4; ++a) m[a] += (double)Mpart[(size_t)s * part_stride + ((size_t)4 * i + a) * 32 + d];
    const double4 qv = ((const double4*)Q64)[(size_t)i * 32 + d];
    const double q[4] = {qv.x, qv.y, qv.z, qv.w};
    // Y = M - Q (Q^T M)
    double y[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        double t[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) t[a] = group32_sum(q[a] * m[b]);
        y[b] = m[b] - (q[0] * t[0] + q[1] * t[1] + q[2] * t[2] + q[3] * t[3]);
    }
    // X R^T = Y, R upper triangular:  Y[d][b] = sum_{c >= b} X[d][c] R[b][c]  ->  back substitution from c = 3
    const double* R = R64 + (size_t)i * 16;
    double x[4];
#pragma unroll
    for (int b = 3; b >= 0; --b) {
        double v = y[b];
#pragma unroll
        for (int cc = b + 1; cc < 4; ++cc) v -= x[cc] * R[b * 4 + cc];
        x[b] = v / R[b * 4 + b];
    }
    ((float4*)dume)[(size_t)i * 32 + d] = make_float4((float)(-2.0 * x[0]), (float)(-2.0 * x[1]), (float)(-2.0 * x[2]), (float)(-2.0 * x[3]));
}

// ---- host side -------------------------------------------------------------------------------------------------------

// (pad_kp and bwd_plan, the rule of the splits: ume_grad_plan.h)

struct SideLayout {
    size_t qrow, qcol, q64, r64;   // byte offsets
};
struct CdistLayout {
    SideLayout s[2];
    size_t mpart, total;
};

static CdistLayout cdist_layout(int n1, int n2)
{
    CdistLayout L;
    size_t off = 0;
    const int n[2] = {n1, n2};
    for (int k = 0; k < 2; ++k) {
        const size_t np = pad_kp(n[k]);
        L.s[k].qrow = off; off = align_up(off + np * 128 * sizeof(float), 256);
        L.s[k].qcol = off; off = align_up(off + np * 128 * sizeof(float), 256);
        L.s[k].q64 = off;  off = align_up(off + np * 128 * sizeof(double), 256);
        L.s[k].r64 = off;  off = align_up(off + np * 16 * sizeof(double), 256);
    }
    const BwdPlan p1 = bwd_plan(n1, n2), p2 = bwd_plan(n2, n1);
    const size_t m1 = (size_t)p1.splits * pad_kp(n1) * 128 * sizeof(float);
    const size_t m2 = (size_t)p2.splits * pad_kp(n2) * 128 * sizeof(float);
    L.mpart = off;
    L.total = align_up(off + (m1 > m2 ? m1 : m2), 256);
    return L;
}

constexpr int kMaxKp = 1 << 22;          // keypoints per side of one distance call
constexpr long long kMaxPoints = 1ll << 31;

static bool moments_sizes_ok(int B, int N, int n)
{
    return B > 0 && N > 0 && n > 0 && (long long)B * N < kMaxPoints && (long long)B * n < kMaxPoints;
}

struct MomLayout {
    size_t rs, box, gr, total;
};
static MomLayout mom_layout(int B, int N, int n)
{
    MomLayout L;
    size_t off = 0;
    L.rs = off;    off = align_up(off + (size_t)B * N * sizeof(double), 256);
    L.box = off;   off = align_up(off + (size_t)B * n * 2 * sizeof(float4), 256);
    L.gr = off;    off = align_up(off + (size_t)B * n * 128 * sizeof(double), 256);
    L.total = off;
    return L;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_ume_moments_bwd_scratch_bytes(int B, int N, int n)
{
    if (!moments_sizes_ok(B, N, n)) return 0;
    return mom_layout(B, N, n).total;
}

UMEREG_API int umereg_ume_moments_bwd_f32(const float* pts, const float* feat, const int64_t* nn_idx, const float* F, const float* dF,
                                          int B, int N, int n, int K, int normalize, float* dfeat, void* scratch,
                                          size_t scratch_bytes, void* stream)
{
    UMEREG_REQUIRE(pts && nn_idx && dF && dfeat && scratch, "ume_moments_bwd: null pointer");
    UMEREG_REQUIRE(!normalize || (feat && F), "ume_moments_bwd: null pointer (the normalised form reads feat and F)");
    UMEREG_REQUIRE(moments_sizes_ok(B, N, n), "ume_moments_bwd: B, N, n must be positive and B N, B n below 2^31 (got %d, %d, %d)", B,
                   N, n);
    UMEREG_REQUIRE(K > 0 && K <= UMEREG_UME_GRAD_MAX_K, "ume_moments_bwd: K must be in [1, %d] (got %d)", UMEREG_UME_GRAD_MAX_K, K);
    const MomLayout L = mom_layout(B, N, n);
    UMEREG_REQUIRE(scratch_bytes >= L.total, "ume_moments_bwd: scratch too small (%zu < %zu bytes)", scratch_bytes, L.total);
    UMEREG_REQUIRE(((uintptr_t)scratch & 255) == 0 && ((uintptr_t)feat & 15) == 0 && ((uintptr_t)F & 7) == 0 && ((uintptr_t)dF & 7) == 0 &&
                       ((uintptr_t)nn_idx & 7) == 0 && ((uintptr_t)pts & 3) == 0 && ((uintptr_t)dfeat & 3) == 0,
                   "ume_moments_bwd: misaligned pointer (scratch: 256 bytes, feat: 16)");
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)scratch;
    double* rs = (double*)(base + L.rs);
    float4* box = (float4*)(base + L.box);
    double* Gr = (double*)(base + L.gr);
    const size_t n_points = (size_t)B * N, n_lists = (size_t)B * n;
    if (normalize) {
        hipLaunchKernelGGL(mom_rowsum_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, st, feat, n_points, rs);
        UMEREG_CHECK_LAUNCH("mom_rowsum_kernel");
    }
    hipLaunchKernelGGL(mom_gr_kernel, dim3((unsigned)((n_lists + kGradWaves - 1) / kGradWaves)), dim3(kWave * kGradWaves), 0, st, pts,
                       nn_idx, F, dF, rs, N, n, K, n_lists, normalize ? 1 : 0, box, Gr);
    UMEREG_CHECK_LAUNCH("mom_gr_kernel");
    hipLaunchKernelGGL(mom_scatter_kernel, dim3((unsigned)((n_points + kGradWaves - 1) / kGradWaves)), dim3(kWave * kGradWaves), 0, st,
                       pts, nn_idx, box, Gr, N, n, K, n_points, dfeat);
    UMEREG_CHECK_LAUNCH("mom_scatter_kernel");
    return UMEREG_OK;
}

UMEREG_API size_t umereg_ume_cdist_bwd_scratch_bytes(int n1, int n2)
{
    if (n1 <= 0 || n2 <= 0 || n1 > kMaxKp || n2 > kMaxKp) return 0;
    return cdist_layout(n1, n2).total;
}

UMEREG_API int umereg_ume_cdist_bwd_f32(const float* ume1, const float* ume2, const float* D, const float* dD, int n1, int n2,
                                        float* dume1, float* dume2, void* scratch, size_t scratch_bytes, void* stream)
{
    UMEREG_REQUIRE(ume1 && ume2 && D && dD && scratch, "ume_cdist_bwd: null pointer");
    UMEREG_REQUIRE(dume1 || dume2, "ume_cdist_bwd: nothing to compute (dume1 and dume2 both null)");
    UMEREG_REQUIRE(n1 > 0 && n2 > 0 && n1 <= kMaxKp && n2 <= kMaxKp, "ume_cdist_bwd: n1, n2 must be in [1, %d] (got %d, %d)", kMaxKp,
                   n1, n2);
    const CdistLayout L = cdist_layout(n1, n2);
    UMEREG_REQUIRE(scratch_bytes >= L.total, "ume_cdist_bwd: scratch too small (%zu < %zu bytes)", scratch_bytes, L.total);
    UMEREG_REQUIRE(((uintptr_t)scratch & 255) == 0 && ((uintptr_t)ume1 & 15) == 0 && ((uintptr_t)ume2 & 15) == 0 &&
                       ((uintptr_t)dume1 & 15) == 0 && ((uintptr_t)dume2 & 15) == 0 && ((uintptr_t)D & 3) == 0 && ((uintptr_t)dD & 3) == 0,
                   "ume_cdist_bwd: misaligned pointer (scratch: 256 bytes, UME matrices: 16)");
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)scratch;
    const float* ume[2] = {ume1, ume2};
    float* out[2] = {dume1, dume2};
    const int n[2] = {n1, n2};
    for (int k = 0; k < 2; ++k) {
        const int np = pad_kp(n[k]);
        hipLaunchKernelGGL(cdist_prep_kernel, dim3((unsigned)(((size_t)np * 32 + kWave * kGradWaves - 1) / (kWave * kGradWaves))),
                           dim3(kWave * kGradWaves), 0, st, ume[k], n[k], np, (float*)(base + L.s[k].qrow), (float*)(base + L.s[k].qcol),
                           (double*)(base + L.s[k].q64), (double*)(base + L.s[k].r64));
        UMEREG_CHECK_LAUNCH("cdist_prep_kernel");
    }
    float* Mpart = (float*)(base + L.mpart);
    for (int k = 0; k < 2; ++k) {
        if (!out[k]) continue;
        const int o = 1 - k;
        const BwdPlan p = bwd_plan(n[k], n[o]);
        const size_t part_stride = (size_t)pad_kp(n[k]) * 128;
        const size_t si = k == 0 ? (size_t)n2 : 1, sj = k == 0 ? 1 : (size_t)n2;
        hipLaunchKernelGGL(cdist_bwd_kernel, dim3((p.n_work + kGradWaves - 1) / kGradWaves), dim3(kWave * kGradWaves), 0, st,
                           (const float*)(base + L.s[k].qrow), (const float*)(base + L.s[o].qrow), (const float*)(base + L.s[o].qcol),
                           4 * pad_kp(n[o]), D, dD, si, sj, n[k], n[o], p.n_rt, p.n_jt, p.tiles_per_split, p.n_work, Mpart, part_stride);
        UMEREG_CHECK_LAUNCH("cdist_bwd_kernel");
        hipLaunchKernelGGL(cdist_finish_kernel, dim3((unsigned)(((size_t)n[k] * 32 + kWave * kGradWaves - 1) / (kWave * kGradWaves))),
                           dim3(kWave * kGradWaves), 0, st, Mpart, part_stride, p.splits, (const double*)(base + L.s[k].q64),
                           (const double*)(base + L.s[k].r64), n[k], out[k]);
        UMEREG_CHECK_LAUNCH("cdist_finish_kernel");
    }
    return UMEREG_OK;
}
