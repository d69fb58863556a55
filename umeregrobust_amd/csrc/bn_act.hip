// bn_act.hip -- y = act(batch_norm(x) [+ residual]) forward and backward, and the gradient scale of the f16 training path
// (include/umereg_bn_act.h).  Memory-bound per-channel operators: a lane owns 4 adjacent channels (one 16-byte load per row), a
// workgroup pass covers `unit` whole rows, the per-channel sums are fp64 over the slab tree of bn_act_plan.h, and each apply kernel
// re-adds the (at most 256) slab partials itself instead of a third launch.
#include "bn_act_plan.h"
#include "common.h"
#include "umereg_bn_act.h"

namespace umereg {

namespace {

constexpr int kBnCells = 4 * kBnThreads;    // unit x C never exceeds this
// Rows a lane loads before it uses the first: every streaming loop below fills an array of this many 16-byte loads and only then
// computes.  Written as `load; use` per row, the compiler waits for each load before it issues the next (one `s_waitcnt vmcnt(0)` per
// `global_load_dwordx4` in the ISA) and the kernels run at one row's latency per row.  A row past the end re-reads a valid row and its
// terms are replaced by zeros, so the sums keep their order and their bits.
constexpr int kBnBatch = 4;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// One slab's two sums per channel: sh[0][r][c] and sh[1][r][c] hold row lane r's sums; channel c's are added over r in ascending
// order and written to part[slab][0 / 1][c].
__device__ __forceinline__ void bn_slab_store(const double* a, const double* b, bool active, int r, int q, int unit, int C, double* sh,
                                              double* __restrict__ part)
{
    if (active) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sh[r * C + 4 * q + j] = a[j];
            sh[(unit + r) * C + 4 * q + j] = b[j];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += kBnThreads) {
        const int which = i / C, c = i % C;
        double s = 0.0;
        for (int k = 0; k < unit; ++k) s += sh[(which * unit + k) * C + c];
        part[((size_t)blockIdx.x * 2 + which) * C + c] = s;
    }
}

// forward statistics of slab blockIdx.x: S1 = sum (x - p), S2 = sum (x - p)^2 about the pivot p = row 0
__global__ __launch_bounds__(kBnThreads) void bn_stats_kernel(const float* __restrict__ x, int ld, int n, int C, int slab,
                                                              double* __restrict__ part)
{
    __shared__ double sh[2 * kBnCells];
    const int lanes = C >> 2, unit = kBnThreads / lanes;
    const int q = threadIdx.x % lanes, r = threadIdx.x / lanes;
    const bool active = r < unit;
    const long long row0 = (long long)blockIdx.x * slab;
    const long long row1 = row0 + slab < n ? row0 + slab : n;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        const float4 p = ld4(x + 4 * q);
        const double p0 = p.x, p1 = p.y, p2 = p.z, p3 = p.w;
        for (long long row = row0 + r; row < row1; row += (long long)kBnBatch * unit) {
            float4 v[kBnBatch];
#pragma unroll
            for (int j = 0; j < kBnBatch; ++j) {
                const long long rj = row + (long long)j * unit;
                v[j] = ld4(x + (size_t)(rj < row1 ? rj : row) * ld + 4 * q);
            }
#pragma unroll
            for (int j = 0; j < kBnBatch; ++j) {
                const bool in = row + (long long)j * unit < row1;
                const double d0 = in ? (double)v[j].x - p0 : 0.0, d1 = in ? (double)v[j].y - p1 : 0.0;
                const double d2 = in ? (double)v[j].z - p2 : 0.0, d3 = in ? (double)v[j].w - p3 : 0.0;
                s1[0] += d0, s1[1] += d1, s1[2] += d2, s1[3] += d3;
                s2[0] = fma(d0, d0, s2[0]), s2[1] = fma(d1, d1, s2[1]), s2[2] = fma(d2, d2, s2[2]), s2[3] = fma(d3, d3, s2[3]);
            }
        }
    }
    bn_slab_store(s1, s2, active, r, q, unit, C, sh, part);
}

// backward sums of slab blockIdx.x: sum g and sum g (x - mean), g = dy (y > 0) or dy
__global__ __launch_bounds__(kBnThreads) void bn_bwd_reduce_kernel(const float* __restrict__ dy, int ld_dy, const float* __restrict__ x,
                                                                   int ld_x, const float* __restrict__ y, int ld_y,
                                                                   const float* __restrict__ mean, int n, int C, int slab, int relu,
                                                                   double* __restrict__ part)
{
    __shared__ double sh[2 * kBnCells];
    const int lanes = C >> 2, unit = kBnThreads / lanes;
    const int q = threadIdx.x % lanes, r = threadIdx.x / lanes;
    const bool active = r < unit;
    const long long row0 = (long long)blockIdx.x * slab;
    const long long row1 = row0 + slab < n ? row0 + slab : n;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        const float4 m = ld4(mean + 4 * q);
        const double m0 = m.x, m1 = m.y, m2 = m.z, m3 = m.w;
        for (long long row = row0 + r; row < row1; row += (long long)kBnBatch * unit) {
            float4 gg[kBnBatch], vv[kBnBatch], oo[kBnBatch];
#pragma unroll
            for (int j = 0; j < kBnBatch; ++j) {
                const long long rj = row + (long long)j * unit;
                const size_t rc = (size_t)(rj < row1 ? rj : row);
                gg[j] = ld4(dy + rc * ld_dy + 4 * q);
                vv[j] = ld4(x + rc * ld_x + 4 * q);
                if (relu) oo[j] = ld4(y + rc * ld_y + 4 * q);
            }
#pragma unroll
            for (int j = 0; j < kBnBatch; ++j) {
                const bool in = row + (long long)j * unit < row1;
                float4 g = gg[j];
                if (relu) {
                    const float4 o = oo[j];
                    g.x = o.x > 0.f ? g.x : 0.f, g.y = o.y > 0.f ? g.y : 0.f, g.z = o.z > 0.f ? g.z : 0.f, g.w = o.w > 0.f ? g.w : 0.f;
                }
                const double g0 = in ? (double)g.x : 0.0, g1 = in ? (double)g.y : 0.0, g2 = in ? (double)g.z : 0.0, g3 = in ? (double)g.w : 0.0;
                const double d0 = in ? (double)vv[j].x - m0 : 0.0, d1 = in ? (double)vv[j].y - m1 : 0.0;
                const double d2 = in ? (double)vv[j].z - m2 : 0.0, d3 = in ? (double)vv[j].w - m3 : 0.0;
                s1[0] += g0, s1[1] += g1, s1[2] += g2, s1[3] += g3;
                s2[0] = fma(g0, d0, s2[0]), s2[1] = fma(g1, d1, s2[1]), s2[2] = fma(g2, d2, s2[2]), s2[3] = fma(g3, d3, s2[3]);
            }
        }
    }
    bn_slab_store(s1, s2, active, r, q, unit, C, sh, part);
}

// The slab partials of both sums, added per channel: W = kBnThreads / C runs of consecutive slabs, each in ascending order, then the
// run sums in ascending order.  Valid in threads < C (channel = thread); sh: [2][W][C] doubles.  Every thread must call it.
__device__ __forceinline__ void bn_sum_partials(const double* __restrict__ part, int slabs, int C, double* sh, double& a, double& b)
{
    const int W = kBnThreads / C, g = threadIdx.x / C, c = threadIdx.x % C;
    const int run = (slabs + W - 1) / W;
    if (g < W) {
        double s1 = 0.0, s2 = 0.0;
        const int lo = g * run, hi = lo + run < slabs ? lo + run : slabs;
        for (int s = lo; s < hi; s += kBnBatch) {
            double u[kBnBatch], w[kBnBatch];
#pragma unroll
            for (int j = 0; j < kBnBatch; ++j) {
                const size_t sj = (size_t)(s + j < hi ? s + j : s);
                u[j] = part[(sj * 2) * C + c];
                w[j] = part[(sj * 2 + 1) * C + c];
            }
#pragma unroll
            for (int j = 0; j < kBnBatch; ++j) {
                s1 += s + j < hi ? u[j] : 0.0;
                s2 += s + j < hi ? w[j] : 0.0;
            }
        }
        sh[g * C + c] = s1;
        sh[(W + g) * C + c] = s2;
    }
    __syncthreads();
    a = b = 0.0;
    if ((int)threadIdx.x < C)
        for (int k = 0; k < W; ++k) {
            a += sh[k * C + c];
            b += sh[(W + k) * C + c];
        }
}

struct BnFwdArgs {
    const float *x, *res, *gamma, *beta;
    float *y, *rmean, *rvar, *smean, *sinv;
    long long* nbt;
    const double* part;
    int ld_x, ld_res, ld_y, n, C, slabs, train, relu;
    double eps, momentum;
};

__global__ __launch_bounds__(kBnThreads) void bn_fwd_apply_kernel(BnFwdArgs a)
{
    __shared__ double shd[2 * kBnThreads];
    __shared__ __attribute__((aligned(16))) float sc[kBnMaxC], sf[kBnMaxC];
    const int t = threadIdx.x, C = a.C;
    double S1 = 0.0, S2 = 0.0;
    if (a.train) bn_sum_partials(a.part, a.slabs, C, shd, S1, S2);
    if (t < C) {
        float mean_f, inv_f;
        if (a.train) {
            const double n = (double)a.n, m1 = S1 / n;
            const double mean = (double)a.x[t] + m1;
            double var = S2 / n - m1 * m1;
            if (var < 0.0) var = 0.0;
            mean_f = (float)mean;
            inv_f = (float)(1.0 / sqrt(var + a.eps));
            if (blockIdx.x == 0 && a.rmean) {
                a.rmean[t] = (float)((1.0 - a.momentum) * (double)a.rmean[t] + a.momentum * mean);
                a.rvar[t] = (float)((1.0 - a.momentum) * (double)a.rvar[t] + a.momentum * (var * (n / (n - 1.0))));
                if (t == 0) *a.nbt += 1;
            }
        } else {
            mean_f = a.rmean[t];
            inv_f = (float)(1.0 / sqrt((double)a.rvar[t] + a.eps));
        }
        if (blockIdx.x == 0) {
            a.smean[t] = mean_f;
            a.sinv[t] = inv_f;
        }
        const float scale = a.gamma[t] * inv_f;
        sc[t] = scale;
        sf[t] = fmaf(-mean_f, scale, a.beta[t]);
    }
    __syncthreads();
    const int lanes = C >> 2, unit = kBnThreads / lanes, q = t % lanes, r = t / lanes;
    if (r >= unit) return;
    const float4 s = ld4(sc + 4 * q), f = ld4(sf + 4 * q);
    const long long step = (long long)gridDim.x * unit;
    for (long long row = (long long)blockIdx.x * unit + r; row < a.n; row += kBnBatch * step) {
        float4 vv[kBnBatch], ee[kBnBatch];
#pragma unroll
        for (int j = 0; j < kBnBatch; ++j) {
            const long long rj = row + j * step;
            const size_t rc = (size_t)(rj < a.n ? rj : row);
            vv[j] = ld4(a.x + rc * a.ld_x + 4 * q);
            if (a.res) ee[j] = ld4(a.res + rc * a.ld_res + 4 * q);
        }
#pragma unroll
        for (int j = 0; j < kBnBatch; ++j) {
            const long long rj = row + j * step;
            if (rj >= a.n) break;
            const float4 v = vv[j];
            float4 o;
            o.x = fmaf(v.x, s.x, f.x), o.y = fmaf(v.y, s.y, f.y), o.z = fmaf(v.z, s.z, f.z), o.w = fmaf(v.w, s.w, f.w);
            if (a.res) o.x += ee[j].x, o.y += ee[j].y, o.z += ee[j].z, o.w += ee[j].w;
            if (a.relu) o.x = o.x < 0.f ? 0.f : o.x, o.y = o.y < 0.f ? 0.f : o.y, o.z = o.z < 0.f ? 0.f : o.z, o.w = o.w < 0.f ? 0.f : o.w;
            st4(a.y + (size_t)rj * a.ld_y + 4 * q, o);
        }
    }
}

struct BnBwdArgs {
    const float *dy, *x, *y, *gamma, *smean, *sinv;
    float *dx, *dres, *dgamma, *dbeta;
    const double* part;
    int ld_dy, ld_x, ld_y, ld_dx, ld_dres, n, C, slabs, train, relu, sums;
};

// dx = a g + c2 x + c3 with a = gamma invstd, c2 = -a invstd dgamma / n, c3 = -a dbeta / n - c2 mean (train); dx = a g (eval)
__global__ __launch_bounds__(kBnThreads) void bn_bwd_apply_kernel(BnBwdArgs a)
{
    __shared__ double shd[2 * kBnThreads];
    __shared__ __attribute__((aligned(16))) float sa[kBnMaxC], s2[kBnMaxC], s3[kBnMaxC];
    const int t = threadIdx.x, C = a.C;
    double Sb = 0.0, Sg = 0.0;
    if (a.sums) bn_sum_partials(a.part, a.slabs, C, shd, Sb, Sg);
    if (t < C) {
        const double inv = (double)a.sinv[t], mean = (double)a.smean[t];
        const double ca = (double)a.gamma[t] * inv;
        double c2 = 0.0, c3 = 0.0;
        if (a.sums) {
            const double dgamma = Sg * inv;
            if (blockIdx.x == 0) {
                a.dbeta[t] = (float)Sb;
                a.dgamma[t] = (float)dgamma;
            }
            if (a.train) {
                const double n = (double)a.n;
                c2 = -(ca * inv) * (dgamma / n);
                c3 = -ca * (Sb / n) - c2 * mean;
            }
        }
        sa[t] = (float)ca, s2[t] = (float)c2, s3[t] = (float)c3;
    }
    __syncthreads();
    const int lanes = C >> 2, unit = kBnThreads / lanes, q = t % lanes, r = t / lanes;
    if (r >= unit) return;
    const float4 ca = ld4(sa + 4 * q), c2 = ld4(s2 + 4 * q), c3 = ld4(s3 + 4 * q);
    const long long step = (long long)gridDim.x * unit;
    const bool need_x = a.dx && a.train;
    for (long long row = (long long)blockIdx.x * unit + r; row < a.n; row += kBnBatch * step) {
        float4 gg[kBnBatch], oo[kBnBatch], vv[kBnBatch];
#pragma unroll
        for (int j = 0; j < kBnBatch; ++j) {
            const long long rj = row + j * step;
            const size_t rc = (size_t)(rj < a.n ? rj : row);
            gg[j] = ld4(a.dy + rc * a.ld_dy + 4 * q);
            if (a.relu) oo[j] = ld4(a.y + rc * a.ld_y + 4 * q);
            if (need_x) vv[j] = ld4(a.x + rc * a.ld_x + 4 * q);
        }
#pragma unroll
        for (int j = 0; j < kBnBatch; ++j) {
            const long long rj = row + j * step;
            if (rj >= a.n) break;
            float4 g = gg[j];
            if (a.relu) {
                const float4 o = oo[j];
                g.x = o.x > 0.f ? g.x : 0.f, g.y = o.y > 0.f ? g.y : 0.f, g.z = o.z > 0.f ? g.z : 0.f, g.w = o.w > 0.f ? g.w : 0.f;
            }
            if (a.dres) st4(a.dres + (size_t)rj * a.ld_dres + 4 * q, g);
            if (a.dx) {
                float4 d;
                if (a.train) {
                    const float4 v = vv[j];
                    d.x = fmaf(v.x, c2.x, fmaf(g.x, ca.x, c3.x)), d.y = fmaf(v.y, c2.y, fmaf(g.y, ca.y, c3.y));
                    d.z = fmaf(v.z, c2.z, fmaf(g.z, ca.z, c3.z)), d.w = fmaf(v.w, c2.w, fmaf(g.w, ca.w, c3.w));
                } else {
                    d.x = g.x * ca.x, d.y = g.y * ca.y, d.z = g.z * ca.z, d.w = g.w * ca.w;
                }
                st4(a.dx + (size_t)rj * a.ld_dx + 4 * q, d);
            }
        }
    }
}

// ---- gradient scale ---------------------------------------------------------------------------------------------------------------
// max |dy| as the unsigned maximum of the bit patterns with the sign cleared: ordered like the magnitudes for finite values, infinity
// above them and every NaN above infinity, so a NaN anywhere comes through.

__device__ __forceinline__ unsigned gs_block_max(unsigned m, unsigned* sh)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, d, kWave);
        m = o > m ? o : m;
    }
    if (lane_id() == 0) sh[threadIdx.x / kWave] = m;
    __syncthreads();
    m = sh[0];
    for (int w = 1; w < kBnThreads / kWave; ++w) m = sh[w] > m ? sh[w] : m;
    return m;
}

__device__ __forceinline__ unsigned gs_abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

__global__ __launch_bounds__(kBnThreads) void gs_partial_kernel(const float* __restrict__ dy, size_t count, unsigned* __restrict__ part)
{
    __shared__ unsigned sh[kBnThreads / kWave];
    const size_t base = (size_t)blockIdx.x * kGsChunk;
    unsigned m = 0;
    constexpr int kLoads = kGsChunk / (4 * kBnThreads);
    if (base + kGsChunk <= count) {         // a whole chunk: every load issued before the first is used
        float4 v[kLoads];
#pragma unroll
        for (int j = 0; j < kLoads; ++j) v[j] = ld4(dy + base + 4 * threadIdx.x + (size_t)j * 4 * kBnThreads);
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const unsigned a = gs_abs_bits(v[j].x), b = gs_abs_bits(v[j].y), c = gs_abs_bits(v[j].z), d = gs_abs_bits(v[j].w);
            const unsigned ab = a > b ? a : b, cd = c > d ? c : d, q = ab > cd ? ab : cd;
            m = q > m ? q : m;
        }
    } else for (int i = 4 * threadIdx.x; i < kGsChunk; i += 4 * kBnThreads) {
        const size_t e = base + i;
        if (e + 3 < count) {
            const float4 v = ld4(dy + e);
            const unsigned a = gs_abs_bits(v.x), b = gs_abs_bits(v.y), c = gs_abs_bits(v.z), d = gs_abs_bits(v.w);
            const unsigned ab = a > b ? a : b, cd = c > d ? c : d, q = ab > cd ? ab : cd;
            m = q > m ? q : m;
        } else {
            for (int j = 0; j < 4; ++j)
                if (e + j < count) {
                    const unsigned a = gs_abs_bits(dy[e + j]);
                    m = a > m ? a : m;
                }
        }
    }
    m = gs_block_max(m, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(kBnThreads) void gs_finish_kernel(const unsigned* __restrict__ part, size_t parts, int32_t* __restrict__ out_e,
                                                               float* __restrict__ out_up, float* __restrict__ out_down)
{
    __shared__ unsigned sh[kBnThreads / kWave];
    unsigned m = 0;
    for (size_t i = threadIdx.x; i < parts; i += kGsWidth) m = part[i] > m ? part[i] : m;
    m = gs_block_max(m, sh);
    if (threadIdx.x == 0) {
        int e = 0;
        if (m != 0 && m < 0x7f800000u) {
            // a normal maximum has floor(log2) = exponent field - 127; a subnormal one lies below 2^-126 and e is held at 126
            e = m < 0x00800000u ? 126 : 14 - ((int)(m >> 23) - 127);
            e = e > 126 ? 126 : e < -126 ? -126 : e;
        }
        *out_e = e;
        *out_up = __uint_as_float((unsigned)(e + 127) << 23);
        *out_down = __uint_as_float((unsigned)(127 - e) << 23);
    }
}

bool bn_rows_ok(const void* p, int ld, int C) { return ld >= C && ld % 4 == 0 && !((uintptr_t)p & 15); }

unsigned bn_apply_grid(int n, int unit)
{
    const long long blocks = ((long long)n + 4LL * unit - 1) / (4LL * unit);      // four rows per lane before the grid wraps
    return (unsigned)(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks);
}

}  // namespace

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_bn_act_scratch_bytes(int n, int C)
{
    if (n <= 0 || !bn_channels_ok(C)) return 0;
    return bn_scratch_bytes(n, C);
}

UMEREG_API int umereg_bn_act_forward_f32(const float* x, int ld_x, const float* residual, int ld_res, int n, int C, const float* gamma,
                                         const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                         int train, int relu, double eps, double momentum, float* y, int ld_y, float* save_mean,
                                         float* save_invstd, void* scratch, size_t scratch_bytes, void* stream)
{
    const char* who = "bn_act_forward";
    UMEREG_REQUIRE(x && gamma && beta && y && save_mean && save_invstd, "%s: null pointer", who);
    UMEREG_REQUIRE(n > 0, "%s: n must be positive (got %d)", who, n);
    UMEREG_REQUIRE(bn_channels_ok(C), "%s: C = %d must be a multiple of 32 up to %d", who, C, UMEREG_BN_ACT_MAX_CH);
    UMEREG_REQUIRE(!(train && n == 1), "%s: train mode needs more than one value per channel (n = 1)", who);
    UMEREG_REQUIRE(bn_rows_ok(x, ld_x, C) && bn_rows_ok(y, ld_y, C) && (!residual || bn_rows_ok(residual, ld_res, C)),
                   "%s: rows must be 16-byte aligned with a stride that is a multiple of 4 and at least C", who);
    UMEREG_REQUIRE(y != x && y != residual, "%s: y may alias neither x nor the residual", who);
    UMEREG_REQUIRE(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, "%s: eps %g / momentum %g out of range", who, eps, momentum);
    if (train) {
        const bool all = running_mean && running_var && num_batches_tracked, none = !running_mean && !running_var && !num_batches_tracked;
        UMEREG_REQUIRE(all || none, "%s: running_mean, running_var and num_batches_tracked go together", who);
        UMEREG_REQUIRE_WORKSPACE(who, scratch, scratch_bytes, bn_scratch_bytes(n, C));
    } else {
        UMEREG_REQUIRE(running_mean && running_var, "%s: eval mode reads running_mean and running_var", who);
    }
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const BnPlan p = bn_plan(n, C);
    if (train) {
        hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)p.slabs), dim3(kBnThreads), 0, st, x, ld_x, n, C, p.slab, (double*)scratch);
        UMEREG_CHECK_LAUNCH("bn_stats_kernel");
    }
    BnFwdArgs a;
    a.x = x, a.res = residual, a.gamma = gamma, a.beta = beta, a.y = y, a.rmean = running_mean, a.rvar = running_var;
    a.smean = save_mean, a.sinv = save_invstd, a.nbt = (long long*)num_batches_tracked, a.part = (const double*)scratch;
    a.ld_x = ld_x, a.ld_res = ld_res, a.ld_y = ld_y, a.n = n, a.C = C, a.slabs = p.slabs, a.train = train ? 1 : 0, a.relu = relu ? 1 : 0;
    a.eps = eps, a.momentum = momentum;
    hipLaunchKernelGGL(bn_fwd_apply_kernel, dim3(bn_apply_grid(n, p.unit)), dim3(kBnThreads), 0, st, a);
    UMEREG_CHECK_LAUNCH("bn_fwd_apply_kernel");
    return UMEREG_OK;
}

UMEREG_API int umereg_bn_act_backward_f32(const float* dy, int ld_dy, const float* x, int ld_x, const float* y, int ld_y, int n, int C,
                                          const float* gamma, const float* save_mean, const float* save_invstd, int train, int relu,
                                          float* dx, int ld_dx, float* dres, int ld_dres, float* dgamma, float* dbeta, void* scratch,
                                          size_t scratch_bytes, void* stream)
{
    const char* who = "bn_act_backward";
    UMEREG_REQUIRE(dy && x && gamma && save_mean && save_invstd && (y || !relu), "%s: null pointer", who);
    UMEREG_REQUIRE(n > 0, "%s: n must be positive (got %d)", who, n);
    UMEREG_REQUIRE(bn_channels_ok(C), "%s: C = %d must be a multiple of 32 up to %d", who, C, UMEREG_BN_ACT_MAX_CH);
    UMEREG_REQUIRE(!(train && n == 1), "%s: train mode needs more than one value per channel (n = 1)", who);
    UMEREG_REQUIRE(!dgamma == !dbeta, "%s: dgamma and dbeta go together", who);
    const bool sums = dgamma != nullptr;
    UMEREG_REQUIRE(sums || !train, "%s: train mode needs dgamma and dbeta (dx depends on them)", who);
    UMEREG_REQUIRE(sums || dx || dres, "%s: nothing to compute", who);
    UMEREG_REQUIRE(bn_rows_ok(dy, ld_dy, C) && bn_rows_ok(x, ld_x, C) && (!relu || bn_rows_ok(y, ld_y, C)) && (!dx || bn_rows_ok(dx, ld_dx, C)) &&
                       (!dres || bn_rows_ok(dres, ld_dres, C)),
                   "%s: rows must be 16-byte aligned with a stride that is a multiple of 4 and at least C", who);
    UMEREG_REQUIRE((!dx || (dx != dy && dx != x && dx != y)) && (!dres || (dres != dy && dres != x && dres != y)) && (!dx || dx != dres),
                   "%s: outputs may not alias inputs or each other", who);
    if (sums) UMEREG_REQUIRE_WORKSPACE(who, scratch, scratch_bytes, bn_scratch_bytes(n, C));
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const BnPlan p = bn_plan(n, C);
    if (sums) {
        hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((unsigned)p.slabs), dim3(kBnThreads), 0, st, dy, ld_dy, x, ld_x, y, ld_y, save_mean, n,
                           C, p.slab, relu ? 1 : 0, (double*)scratch);
        UMEREG_CHECK_LAUNCH("bn_bwd_reduce_kernel");
    }
    BnBwdArgs a;
    a.dy = dy, a.x = x, a.y = y, a.gamma = gamma, a.smean = save_mean, a.sinv = save_invstd, a.dx = dx, a.dres = dres, a.dgamma = dgamma;
    a.dbeta = dbeta, a.part = (const double*)scratch, a.ld_dy = ld_dy, a.ld_x = ld_x, a.ld_y = ld_y, a.ld_dx = ld_dx, a.ld_dres = ld_dres;
    a.n = n, a.C = C, a.slabs = p.slabs, a.train = train ? 1 : 0, a.relu = relu ? 1 : 0, a.sums = sums ? 1 : 0;
    // without dx and dres the apply kernel still finishes the sums: one workgroup
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(dx || dres ? bn_apply_grid(n, p.unit) : 1u), dim3(kBnThreads), 0, st, a);
    UMEREG_CHECK_LAUNCH("bn_bwd_apply_kernel");
    return UMEREG_OK;
}

UMEREG_API size_t umereg_grad_scale_scratch_bytes(size_t count)
{
    if (count > ((size_t)1 << 40)) return 0;
    const size_t parts = gs_partials(count);
    return (parts ? parts : 1) * 4;
}

UMEREG_API int umereg_grad_scale_f32(const float* dy, size_t count, int32_t* out_e, float* out_up, float* out_down, void* scratch,
                                     size_t scratch_bytes, void* stream)
{
    const char* who = "grad_scale";
    UMEREG_REQUIRE(out_e && out_up && out_down && (dy || count == 0), "%s: null pointer", who);
    UMEREG_REQUIRE(count <= ((size_t)1 << 40), "%s: %zu elements are more than 2^40", who, count);
    UMEREG_REQUIRE(!((uintptr_t)dy & 15), "%s: dy must be 16-byte aligned", who);
    UMEREG_REQUIRE_WORKSPACE(who, scratch, scratch_bytes, umereg_grad_scale_scratch_bytes(count));
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t parts = gs_partials(count);
    if (parts) {
        hipLaunchKernelGGL(gs_partial_kernel, dim3((unsigned)parts), dim3(kBnThreads), 0, st, dy, count, (unsigned*)scratch);
        UMEREG_CHECK_LAUNCH("gs_partial_kernel");
    }
    hipLaunchKernelGGL(gs_finish_kernel, dim3(1), dim3(kBnThreads), 0, st, (const unsigned*)scratch, parts, out_e, out_up, out_down);
    UMEREG_CHECK_LAUNCH("gs_finish_kernel");
    return UMEREG_OK;
}
