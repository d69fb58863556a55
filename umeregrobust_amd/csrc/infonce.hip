// infonce.hip -- the fused InfoNCE point-wise loss, forward and backward (include/umereg_infonce.h has the contract; the tile constants
// and the workspace layout are csrc/infonce_plan.h).  No S x S tensor is formed and nothing is gathered into HBM: every kernel reads
// the caller's [B, N, 32] / [B, M, 32] features and [B, N, 3] points through `matches`.
//
// A workgroup owns kInfoNceRows = 32 samples (the OWN side, in registers) and walks all S samples of the other side (the WALKED
// side) in steps of kInfoNceCols = 128, staged in LDS: 36-float feature rows and one float4 (x, y, z, lse) per sample.  Wave w takes
// samples 32 w .. 32 w + 31 of a step.  The logit tile is computed transposed on v_mfma_f32_32x32x2_f32,
//     X[walked r][own c] = sum_k walked[r][k] own[c][k]
// (A[i = l&31][k = l>>5], B[k = l>>5][j = l&31], C row = (reg&3) + 8 (reg>>2) + 4 (l>>5), col = l&31), so lane l keeps ONE own
// sample c = l&31 and 16 walked samples in its accumulator: the mask, the exp and the row sum never leave the registers, and the two
// lane halves and the four waves are combined once at the end.  Instruction s contracts channels s (lane half 0) and 16 + s (half 1),
// in all three passes, so a logit has the same bits wherever it is recomputed (a product does not care which factor is A).
//
//   infonce_fwd_kernel      own = anchors, walked = positives.  Running maximum and sum per lane; the finish (fp64) writes
//                           row_stats and the workgroup's row sum.
//   infonce_loss_kernel     one workgroup adds the row sums in workgroup order.
//   infonce_bwd_kernel      pass 0, row owner:    own = anchors,   walked = positives: dA_s = c sum_t w_st p_t + ...
//                           pass 1, column owner: own = positives, walked = anchors (their lse staged beside their positions):
//                           dP_t = c sum_s w_st a_s + ...   Either pass chains the logit tile into the gradient product, as
//                           ume_cdist_bwd does: the accumulator X, turned into w in place, is the B operand (k = its walked row) of
//                           G^T[d][own c] += walked^T[d][r] w[r][c], whose A operand is read from the staged rows.  The workgroups of
//                           a pass also zero that pass's output tensor, so the scatter that follows only adds.  Two launches, rows
//                           first: the row pass also writes each row's sum_t w_st (= 1 - w_s0 without the cancellation), which the
//                           column pass reads for the positive term of its own samples.
//   infonce_scatter_kernel  per-sample gradients -> dsrc / dtgt.  The lowest sample that names a row owns it and adds the samples
//                           that name it in ascending order; the S row indices of a batch element are scanned from LDS.
#include "common.h"
#include "umereg_infonce.h"
#include "infonce_plan.h"

namespace umereg {

using f32x16n = __attribute__((ext_vector_type(16))) float;

struct InfoNceIn {
    const float* src_feat;
    const float* src_pts;
    const float* tgt_feat;
    const int64_t* matches;
    int B, N, M, S, n_blk;
    float inv_tau, r2;
    double tau;
};

// rows (i, j) of sample (b, s); false (and rows 0, never to be read) when either lies outside its tensor
__device__ __forceinline__ bool infonce_rows(const InfoNceIn& p, int b, int s, int& i, int& j)
{
    const int64_t* m = p.matches + ((size_t)b * p.S + s) * 2;
    const int64_t a = m[0], c = m[1];
    const bool ok = a >= 0 && a < p.N && c >= 0 && c < p.M;
    i = ok ? (int)a : 0;
    j = ok ? (int)c : 0;
    return ok;
}

__device__ __forceinline__ const float* infonce_anchor(const InfoNceIn& p, int b, int i) { return p.src_feat + ((size_t)b * p.N + i) * 32; }
__device__ __forceinline__ const float* infonce_positive(const InfoNceIn& p, int b, int j) { return p.tgt_feat + ((size_t)b * p.M + j) * 32; }

// Stage samples t0 .. t0 + 127 of the walked side: thread (row = tid >> 1, half = tid & 1) copies 16 channels.  A sample past S or
// with a row out of range is staged as zero features at a NaN position: no comparison with it is ever `far`.
template <bool kWalkAnchors>
__device__ __forceinline__ void infonce_stage(const InfoNceIn& p, int b, int t0, const float* __restrict__ row_stats, float* feat,
                                              float4* aux)
{
    const int row = threadIdx.x >> 1, half = threadIdx.x & 1;
    const int t = t0 + row;
    int i = 0, j = 0;
    const bool ok = t < p.S && infonce_rows(p, b, t, i, j);
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) {
        const float4* src = (const float4*)((kWalkAnchors ? infonce_anchor(p, b, i) : infonce_positive(p, b, j)) + 16 * half);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = src[q];
    }
    float4* dst = (float4*)(feat + row * kInfoNceLdsStride + 16 * half);
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = v[q];
    if (half == 0) {
        const float nan = __builtin_nanf("");
        float4 x = make_float4(nan, nan, nan, 0.f);
        if (ok) {
            const float* xp = p.src_pts + ((size_t)b * p.N + i) * 3;
            x.x = xp[0];
            x.y = xp[1];
            x.z = xp[2];
            if (kWalkAnchors) x.w = row_stats[((size_t)b * p.S + t) * 2];
        }
        aux[row] = x;
    }
}

// the own side of lane (c, h): channels 16 h .. 16 h + 15 of its sample's feature row, and the sample's position (NaN: none)
struct InfoNceOwn {
    float q[16];
    float x, y, z;
    int i, j;
    bool ok;
};

template <bool kOwnAnchors>
__device__ __forceinline__ void infonce_own(const InfoNceIn& p, int b, int s, int h, InfoNceOwn& o)
{
    o.ok = s < p.S && infonce_rows(p, b, s, o.i, o.j);
    const float nan = __builtin_nanf("");
    o.x = o.y = o.z = nan;
#pragma unroll
    for (int k = 0; k < 16; ++k) o.q[k] = 0.f;
    if (o.ok) {
        const float4* src = (const float4*)((kOwnAnchors ? infonce_anchor(p, b, o.i) : infonce_positive(p, b, o.j)) + 16 * h);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = src[q];
            o.q[4 * q + 0] = v.x; o.q[4 * q + 1] = v.y; o.q[4 * q + 2] = v.z; o.q[4 * q + 3] = v.w;
        }
        const float* xp = p.src_pts + ((size_t)b * p.N + o.i) * 3;
        o.x = xp[0];
        o.y = xp[1];
        o.z = xp[2];
    }
}

// <a, p>, |a|^2, |p|^2 of sample (i, j) in fp64; lane half h adds channels 16 h .. 16 h + 15 and the halves are exchanged
__device__ __forceinline__ void infonce_dots(const InfoNceIn& p, int b, bool ok, int i, int j, int h, double& ap, double& aa, double& pp)
{
    ap = aa = pp = 0.0;
    if (ok) {
        const float* a = infonce_anchor(p, b, i) + 16 * h;
        const float* q = infonce_positive(p, b, j) + 16 * h;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const double av = a[k], pv = q[k];
            ap = fma(av, pv, ap);
            aa = fma(av, av, aa);
            pp = fma(pv, pv, pp);
        }
    }
    ap += shfl_xor_f64(ap, 32);
    aa += shfl_xor_f64(aa, 32);
    pp += shfl_xor_f64(pp, 32);
}

// X[walked row 8 (r>>2) + 4 h + (r&3) of the wave's 32][own c], register r
__device__ __forceinline__ f32x16n infonce_logits(const float* feat, int wave, int c, int h, const float (&own)[16])
{
    const float4* src = (const float4*)(feat + (wave * 32 + c) * kInfoNceLdsStride + 16 * h);
    float w[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = src[q];
        w[4 * q + 0] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    f32x16n st = {0};
#pragma unroll
    for (int s = 0; s < 16; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s], own[s], st, 0, 0, 0);
    return st;
}

__device__ __forceinline__ bool infonce_far(const float4& xt, const InfoNceOwn& o, float r2)
{
    const float dx = o.x - xt.x, dy = o.y - xt.y, dz = o.z - xt.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 > r2;     // false for a NaN position
}

__global__ __launch_bounds__(kInfoNceThreads) void infonce_fwd_kernel(InfoNceIn p, float* __restrict__ row_stats, double* __restrict__ part)
{
    __shared__ __align__(16) float lds[kInfoNceLdsBytes / 4];
    float* feat = lds;
    float4* aux = (float4*)(lds + kInfoNceCols * kInfoNceLdsStride);
    const int b = blockIdx.x / p.n_blk, blk = blockIdx.x % p.n_blk;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id(), c = lane & 31, h = lane >> 5;
    const int s = blk * kInfoNceRows + c;

    InfoNceOwn own;
    infonce_own<true>(p, b, s, h, own);

    float m = -INFINITY, l = 0.f;       // running maximum of the kept l / tau of this lane's 16-sample strips, and sum of exp(. - m)
    for (int t0 = 0; t0 < p.S; t0 += kInfoNceCols) {
        if (t0) __syncthreads();
        infonce_stage<false>(p, b, t0, nullptr, feat, aux);
        __syncthreads();
        if (t0 + wave * 32 >= p.S) continue;
        const f32x16n st = infonce_logits(feat, wave, c, h, own.q);
        float z[16];
        float tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float4 xt = aux[wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3)];
            z[r] = infonce_far(xt, own, p.r2) ? st[r] * p.inv_tau : -INFINITY;
            tm = fmaxf(tm, z[r]);
        }
        if (tm > m) {       // (m = -inf: l is 0 and stays 0)
            l *= expf(m - tm);
            m = tm;
        }
        if (m > -INFINITY) {
#pragma unroll
            for (int r = 0; r < 16; ++r) l += expf(z[r] - m);    // exp(-inf) = 0 for what the mask removed
        }
    }

    // combine: 8 (wave, half) partials per row, in that order, with the positive term, in fp64
    __syncthreads();
    float* cm = lds;
    float* cl = lds + 8 * 32;
    cm[(wave * 2 + h) * 32 + c] = m;
    cl[(wave * 2 + h) * 32 + c] = l;
    __syncthreads();
    if (wave != 0) return;
    double ap, aa, pp;
    infonce_dots(p, b, own.ok, own.i, own.j, h, ap, aa, pp);
    double row = 0.0;
    if (s < p.S) {
        double lse = __builtin_nan(""), pos = __builtin_nan("");
        if (own.ok) {
            pos = ap / fmax(sqrt(aa) * sqrt(pp), 1e-8);
            const double zpos = pos / p.tau;
            double mx = zpos;
#pragma unroll
            for (int k = 0; k < 8; ++k) mx = fmax(mx, (double)cm[k * 32 + c]);
            double sum = exp(zpos - mx);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float lk = cl[k * 32 + c];
                if (lk > 0.f) sum += (double)lk * exp((double)cm[k * 32 + c] - mx);
            }
            lse = mx + log(sum);
            row = lse - zpos;
        } else {
            row = lse;
        }
        if (h == 0) *(float2*)(row_stats + ((size_t)b * p.S + s) * 2) = make_float2((float)lse, (float)pos);
    }
    // the 32 rows of the workgroup, one fixed tree (both lane halves hold the same 32 values)
#pragma unroll
    for (int k = 1; k < 32; k <<= 1) row += shfl_xor_f64(row, k);
    if (lane == 0) part[blockIdx.x] = row;
}

__global__ __launch_bounds__(256) void infonce_loss_kernel(const double* __restrict__ part, int n, double count, float* __restrict__ loss)
{
    __shared__ double red[256];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += part[i];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / count);
}

// kCol = false: dA of the workgroup's 32 samples (own = anchors); true: dP (own = positives).  out: f32 [B][S][32] per-sample
// gradients; zero: `n_zero` float4 of the pass's scatter target, cleared by the pass's workgroups (blocks_in_pass of them).
// nmass f32 [B][S]: the negatives' share of each row, 1 - w_s0 = sum_t w_st.  The row pass adds it up beside its product (1 - exp(.)
// from row_stats would cancel where a row's loss is small) and writes it; the column pass, launched after it, reads it for its own
// samples.  want_g = false (row pass only): nmass alone, no gradient product and no `out`.
template <bool kCol>
__device__ __forceinline__ void infonce_bwd_pass(const InfoNceIn& p, const float* __restrict__ row_stats, const float* __restrict__ dloss,
                                                 float scale, float* __restrict__ out, float* __restrict__ nmass, bool want_g,
                                                 float4* __restrict__ zero, size_t n_zero, float* lds)
{
    for (size_t k = (size_t)blockIdx.x * kInfoNceThreads + threadIdx.x; k < n_zero; k += (size_t)gridDim.x * kInfoNceThreads)
        zero[k] = make_float4(0.f, 0.f, 0.f, 0.f);

    float* feat = lds;
    float4* aux = (float4*)(lds + kInfoNceCols * kInfoNceLdsStride);
    const int b = blockIdx.x / p.n_blk, blk = blockIdx.x % p.n_blk;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id(), c = lane & 31, h = lane >> 5;
    const int s0 = blk * kInfoNceRows;
    const int s = s0 + c;

    InfoNceOwn own;
    infonce_own<!kCol>(p, b, s, h, own);
    const float own_lse = (!kCol && own.ok) ? row_stats[((size_t)b * p.S + s) * 2] : 0.f;

    f32x16n g = {0};        // G^T[d = 8 (r>>2) + 4 h + (r&3)][own c]
    float nw = 0.f;         // row pass: this lane's share of sum_t w_st of its own sample
    for (int t0 = 0; t0 < p.S; t0 += kInfoNceCols) {
        if (t0) __syncthreads();
        infonce_stage<kCol>(p, b, t0, row_stats, feat, aux);
        __syncthreads();
        if (t0 + wave * 32 >= p.S) continue;
        f32x16n st = infonce_logits(feat, wave, c, h, own.q);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float4 xt = aux[wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3)];
            const float e = st[r] * p.inv_tau - (kCol ? xt.w : own_lse);
            st[r] = infonce_far(xt, own, p.r2) ? expf(e) : 0.f;
            if (!kCol) nw += st[r];
        }
        if (!want_g) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float a2 = feat[(wave * 32 + 8 * (r >> 2) + 4 * h + (r & 3)) * kInfoNceLdsStride + c];
            g = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, st[r], g, 0, 0, 0);
        }
    }

    // the four waves' G as [wave][own c][d], per own sample the two coefficients of the positive term, and the 8 shares of nmass
    __syncthreads();
    float* comb = lds;
    float* coef = lds + kInfoNceWaves * 32 * 32;
    float* nwp = coef + 2 * 32;
    if (!kCol) nwp[(wave * 2 + h) * 32 + c] = nw;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *(float4*)(comb + (wave * 32 + c) * 32 + 8 * q + 4 * h) = make_float4(g[4 * q + 0], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
    if (wave == 0) {
        double ap, aa, pp;
        infonce_dots(p, b, own.ok, own.i, own.j, h, ap, aa, pp);
        float k_other = 0.f, k_self = 0.f;
        if (own.ok) {
            // pos = ap / den: d pos / d self = other / den - pos self / |self|^2 (the second term only where den is not the floor);
            // the finish multiplies both by w_s0 - 1 = -nmass
            const double nn = sqrt(aa) * sqrt(pp), den = fmax(nn, 1e-8), pos = ap / den;
            k_other = (float)(1.0 / den);
            k_self = nn > 1e-8 ? (float)(-pos / (kCol ? pp : aa)) : 0.f;
        }
        if (h == 0) {
            coef[2 * c + 0] = k_other;
            coef[2 * c + 1] = k_self;
        }
    }
    __syncthreads();
    const int c2 = threadIdx.x >> 3, dq = threadIdx.x & 7;
    const int s2 = s0 + c2;
    if (s2 >= p.S) return;
    float nm;
    if (kCol) {
        nm = nmass[(size_t)b * p.S + s2];
    } else {
        nm = nwp[c2];
#pragma unroll
        for (int k = 1; k < 2 * kInfoNceWaves; ++k) nm += nwp[k * 32 + c2];
    }
    int i2 = 0, j2 = 0;
    const bool ok2 = infonce_rows(p, b, s2, i2, j2);
    if (!kCol && dq == 0) nmass[(size_t)b * p.S + s2] = ok2 ? nm : 0.f;
    if (!want_g) return;
    float4 acc = *(const float4*)(comb + c2 * 32 + 4 * dq);
#pragma unroll
    for (int w = 1; w < kInfoNceWaves; ++w) {
        const float4 v = *(const float4*)(comb + (w * 32 + c2) * 32 + 4 * dq);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    float4 res = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok2) {
        const float4 av = *(const float4*)(infonce_anchor(p, b, i2) + 4 * dq);
        const float4 pv = *(const float4*)(infonce_positive(p, b, j2) + 4 * dq);
        const float4 self = kCol ? pv : av, other = kCol ? av : pv;
        const float ko = -nm * coef[2 * c2 + 0], ks = -nm * coef[2 * c2 + 1];
        const float cg = dloss[0] * scale;
        res.x = cg * ((acc.x + ko * other.x) + ks * self.x);
        res.y = cg * ((acc.y + ko * other.y) + ks * self.y);
        res.z = cg * ((acc.z + ko * other.z) + ks * self.z);
        res.w = cg * ((acc.w + ko * other.w) + ks * self.w);
    }
    *(float4*)(out + ((size_t)b * p.S + s2) * 32 + 4 * dq) = res;
}

// pass 0: the row pass (out = dA, zero = dsrc or NULL with n_zero = 0); pass 1: the column pass (out = dP, zero = dtgt)
__global__ __launch_bounds__(kInfoNceThreads) void infonce_bwd_kernel(InfoNceIn p, const float* __restrict__ row_stats,
                                                                     const float* __restrict__ dloss, float scale, int pass,
                                                                     float* __restrict__ out, float* __restrict__ nmass, int want_g,
                                                                     float4* __restrict__ zero, size_t n_zero)
{
    __shared__ __align__(16) float lds[kInfoNceLdsBytes / 4];
    if (pass == 0)
        infonce_bwd_pass<false>(p, row_stats, dloss, scale, out, nmass, want_g != 0, zero, n_zero, lds);
    else
        infonce_bwd_pass<true>(p, row_stats, dloss, scale, out, nmass, true, zero, n_zero, lds);
}

// blockIdx.z + side0 is the side: 0 = dA -> dsrc through matches[..][0], 1 = dP -> dtgt through matches[..][1]
__global__ __launch_bounds__(kInfoNceThreads) void infonce_scatter_kernel(const int64_t* __restrict__ matches, int S, int N, int M,
                                                                         int side0, const float* __restrict__ dA,
                                                                         const float* __restrict__ dP, float* __restrict__ dsrc,
                                                                         float* __restrict__ dtgt)
{
    __shared__ int idx[kInfoNceMaxS];
    const int side = blockIdx.z + side0, b = blockIdx.y;
    const int range = side ? M : N;
    const float* in = (side ? dP : dA) + (size_t)b * S * 32;
    float* out = (side ? dtgt : dsrc) + (size_t)b * range * 32;
    for (int t = threadIdx.x; t < S; t += kInfoNceThreads) {
        const int64_t v = matches[((size_t)b * S + t) * 2 + side];
        idx[t] = (v >= 0 && v < range) ? (int)v : -1;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    constexpr int per_wave = kInfoNceScatterRows / kInfoNceWaves;
    for (int k = 0; k < per_wave; ++k) {
        const int s = blockIdx.x * kInfoNceScatterRows + wave * per_wave + k;      // wave-uniform
        if (s >= S) break;
        const int my = idx[s];
        if (my < 0) continue;
        bool owner = true;
        float acc = 0.f;
        for (int c0 = 0; c0 < S && owner; c0 += kWave) {
            const int t = c0 + lane;
            unsigned long long mask = __ballot(t < S && idx[t] == my);
            while (mask) {
                const int tt = c0 + __builtin_ctzll(mask);
                mask &= mask - 1;
                if (tt < s) {       // a lower sample names the row: it adds this one
                    owner = false;
                    break;
                }
                acc += in[(size_t)tt * 32 + (lane & 31)];
            }
        }
        if (owner && lane < 32) out[(size_t)my * 32 + lane] = acc;
    }
}

static int infonce_check(const char* who, const float* src_feat, const float* src_pts, const float* tgt_feat, const int64_t* matches,
                         int B, int N, int M, int S, float tau, float neg_dist)
{
    UMEREG_REQUIRE(src_feat && src_pts && tgt_feat && matches, "%s: null pointer", who);
    UMEREG_REQUIRE(infonce_sizes_ok(B, N, M, S), "%s: B, N, M must be positive and S in [1, %d] (got B = %d, N = %d, M = %d, S = %d)", who,
                   kInfoNceMaxS, B, N, M, S);
    UMEREG_REQUIRE(tau > 0.f && tau < INFINITY, "%s: tau must be positive and finite (got %g)", who, (double)tau);
    UMEREG_REQUIRE(neg_dist >= 0.f && neg_dist < INFINITY, "%s: neg_dist must be non-negative and finite (got %g)", who, (double)neg_dist);
    UMEREG_REQUIRE(((uintptr_t)src_feat & 15) == 0 && ((uintptr_t)tgt_feat & 15) == 0 && ((uintptr_t)src_pts & 3) == 0 &&
                       ((uintptr_t)matches & 7) == 0,
                   "%s: misaligned pointer (features: 16 bytes, matches: 8)", who);
    return UMEREG_OK;
}

static InfoNceIn infonce_in(const float* src_feat, const float* src_pts, const float* tgt_feat, const int64_t* matches, int B, int N, int M,
                            int S, float tau, float neg_dist)
{
    InfoNceIn p;
    p.src_feat = src_feat;
    p.src_pts = src_pts;
    p.tgt_feat = tgt_feat;
    p.matches = matches;
    p.B = B;
    p.N = N;
    p.M = M;
    p.S = S;
    p.n_blk = infonce_row_blocks(S);
    p.inv_tau = (float)(1.0 / (double)tau);
    p.r2 = (float)((double)neg_dist * (double)neg_dist);
    p.tau = (double)tau;
    return p;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_infonce_workspace_bytes(int B, int N, int M, int S)
{
    if (!infonce_sizes_ok(B, N, M, S)) return 0;
    return infonce_layout(B, S).total;
}

UMEREG_API int umereg_infonce_fwd_f32(const float* src_feat, const float* src_pts, const float* tgt_feat, const int64_t* matches, int B,
                                      int N, int M, int S, float tau, float neg_dist, float* row_stats, float* loss, void* workspace,
                                      size_t workspace_bytes, void* stream)
{
    if (int rc = infonce_check("infonce_fwd", src_feat, src_pts, tgt_feat, matches, B, N, M, S, tau, neg_dist)) return rc;
    UMEREG_REQUIRE(row_stats && loss, "infonce_fwd: null pointer");
    UMEREG_REQUIRE(((uintptr_t)row_stats & 7) == 0 && ((uintptr_t)loss & 3) == 0, "infonce_fwd: misaligned pointer (row_stats: 8 bytes)");
    const InfoNceLayout L = infonce_layout(B, S);
    UMEREG_REQUIRE_WORKSPACE("infonce_fwd", workspace, workspace_bytes, L.total);
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const InfoNceIn p = infonce_in(src_feat, src_pts, tgt_feat, matches, B, N, M, S, tau, neg_dist);
    double* part = (double*)((char*)workspace + L.part);
    const int n_wg = B * p.n_blk;
    hipLaunchKernelGGL(infonce_fwd_kernel, dim3((unsigned)n_wg), dim3(kInfoNceThreads), 0, st, p, row_stats, part);
    UMEREG_CHECK_LAUNCH("infonce_fwd_kernel");
    hipLaunchKernelGGL(infonce_loss_kernel, dim3(1), dim3(256), 0, st, (const double*)part, n_wg, (double)B * (double)S, loss);
    UMEREG_CHECK_LAUNCH("infonce_loss_kernel");
    return UMEREG_OK;
}

UMEREG_API int umereg_infonce_bwd_f32(const float* src_feat, const float* src_pts, const float* tgt_feat, const int64_t* matches, int B,
                                      int N, int M, int S, float tau, float neg_dist, const float* row_stats, const float* dloss,
                                      float* dsrc, float* dtgt, void* workspace, size_t workspace_bytes, void* stream)
{
    if (int rc = infonce_check("infonce_bwd", src_feat, src_pts, tgt_feat, matches, B, N, M, S, tau, neg_dist)) return rc;
    UMEREG_REQUIRE(row_stats && dloss, "infonce_bwd: null pointer");
    UMEREG_REQUIRE(dsrc || dtgt, "infonce_bwd: nothing to compute (dsrc and dtgt both null)");
    UMEREG_REQUIRE(((uintptr_t)row_stats & 7) == 0 && ((uintptr_t)dloss & 3) == 0 && ((uintptr_t)dsrc & 15) == 0 &&
                       ((uintptr_t)dtgt & 15) == 0,
                   "infonce_bwd: misaligned pointer (row_stats: 8 bytes, gradients: 16)");
    const InfoNceLayout L = infonce_layout(B, S);
    UMEREG_REQUIRE_WORKSPACE("infonce_bwd", workspace, workspace_bytes, L.total);
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const InfoNceIn p = infonce_in(src_feat, src_pts, tgt_feat, matches, B, N, M, S, tau, neg_dist);
    float* dA = (float*)((char*)workspace + L.da);
    float* dP = (float*)((char*)workspace + L.dp);
    const int first = dsrc ? 0 : 1, count = (dsrc ? 1 : 0) + (dtgt ? 1 : 0);
    const float scale = (float)(1.0 / ((double)B * (double)S * (double)tau));
    float* nmass = (float*)((char*)workspace + L.nm);
    // the row pass always runs: it makes nmass, which the column pass reads; without dsrc it makes nothing else
    hipLaunchKernelGGL(infonce_bwd_kernel, dim3((unsigned)(B * p.n_blk)), dim3(kInfoNceThreads), 0, st, p, row_stats, dloss, scale, 0, dA,
                       nmass, dsrc ? 1 : 0, (float4*)dsrc, dsrc ? (size_t)B * N * 8 : (size_t)0);
    UMEREG_CHECK_LAUNCH("infonce_bwd_kernel (rows)");
    if (dtgt) {
        hipLaunchKernelGGL(infonce_bwd_kernel, dim3((unsigned)(B * p.n_blk)), dim3(kInfoNceThreads), 0, st, p, row_stats, dloss, scale, 1,
                           dP, nmass, 1, (float4*)dtgt, (size_t)B * M * 8);
        UMEREG_CHECK_LAUNCH("infonce_bwd_kernel (columns)");
    }
    const unsigned sblk = (unsigned)((S + kInfoNceScatterRows - 1) / kInfoNceScatterRows);
    // (B as gridDim.y: the scatter is cut into calls of at most 65535 batch elements)
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = B - b0 < 65535 ? B - b0 : 65535;
        hipLaunchKernelGGL(infonce_scatter_kernel, dim3(sblk, (unsigned)nb, (unsigned)count), dim3(kInfoNceThreads), 0, st,
                           matches + (size_t)b0 * S * 2, S, N, M, first, (const float*)(dA + (size_t)b0 * S * 32),
                           (const float*)(dP + (size_t)b0 * S * 32), dsrc ? dsrc + (size_t)b0 * N * 32 : nullptr,
                           dtgt ? dtgt + (size_t)b0 * M * 32 : nullptr);
        UMEREG_CHECK_LAUNCH("infonce_scatter_kernel");
    }
    return UMEREG_OK;
}
