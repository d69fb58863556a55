// ume_moments.hip -- a1+a2 (fused ball query + feature gather + UME moments) for gfx950.  Replaces
// evaluate.my_ume_generation (reference evaluate.py:50-60).
//
//   moments 8 neighbours x 8 channel-quads per step: each lane loads one 16 B slice of a
//           neighbour's 128 B feature row (1 KiB per wave-load, whole rows) and its xyz, and keeps
//           4 channels x {1,x,y,z} fp64 accumulators; the 8 neighbour slots are folded with
//           xor-shuffles, the normaliser is a wave reduction, the 32x4 fp32 result leaves as
//           8 lanes x 64 B.  fp64 accumulation makes the result independent of neighbour order
//           to ~1e-16, i.e. the correctly rounded fp32 moment matrix.
// The reference's [n_kp,K,32] gathered intermediate (960 MB at KITTI size) never exists.
// The structure it searches is built by grid.hip; the search is ball_search.h.
#include "ball_search.h"

namespace umereg {

// ---- a1+a2: fused ball query + gather + UME moments -------------------------------------------
// value of lane 8g (the first lane of every aligned group of 8) in all 8 lanes of the group: quad_perm [0,0,0,0]
// spreads it over its quad, row_shr:4 restricted to banks 1 and 3 (lanes 4-7, 12-15 of a row) copies quad 0 / 2 of
// every row onto quad 1 / 3
__device__ __forceinline__ float bcast8(float v)
{
    int x = __float_as_int(v);
    x = __builtin_amdgcn_mov_dpp(x, 0x00, 0xf, 0xf, true);                       // quad_perm [0,0,0,0]
    x = __builtin_amdgcn_update_dpp(x, x, 0x114, 0xf, 0xa, false);              // row_shr:4, bank_mask 0b1010
    return __int_as_float(x);
}

constexpr int kMomUnroll = 4;  // 4 x 8 = 32 neighbours in flight per wave (8 measured no faster, and costs 2 waves/SIMD)

// kAcc = 1 (UMEREG_MOMENTS_ACC_VALU): every neighbour term accumulated in fp64 on the vector pipe (order-independent to 1e-16, the
// correctly rounded fp32 matrix) -- the default of rounds 1-3, bit-identical to today's kAcc = 2 on every input tried.
// kAcc = 0 (UMEREG_MOMENTS_ACC_F32, opt-in): the neighbour sums in packed fp32 on KEYPOINT-CENTRED coordinates -- sum f (p - c)^T
// with |p - c| <= radius instead of |p| <= 50 m, the term  c (sum f)^T  added back once, in fp64, together with the fold of the 8
// neighbour slots, the normaliser and the division: 8 v_pk_add / v_pk_fma + 3 subtractions per lane and neighbour instead of 16 fp64
// operations + 7 conversions.  Measured on MI355X (tools/exp_mom_acc.py, KT pair): 101 us against 111 us -- 9 %, not the 40 % the
// instruction count suggests: v_pk_fma_f32 issues at half rate here, so 8 packed FMAs cost what 16 fp64 FMAs do and only the
// conversions are saved -- for a result 2.6e-5 (row-relative maximum; median 1e-7) from the fp64 evaluation instead of 0, 4.6e-4 on
// saturated balls of random features, where the normaliser sum_c sum f cancels (the reference's own fp32 sums: 1.6e-4 / 8.7e-4).
// Three per cent of a pair for two orders of magnitude of accuracy: it stays an option, not the default.
// kAcc = 2 (the default since round 4; kAcc = 1, the loop of rounds 1-3, stays behind UMEREG_MOMENTS_ACC_VALU): the same fp64 sums on the matrix pipe -- v_mfma_f64_4x4x4_4b_f64, four blocks of
// D(4x4) += A(4x4) B(4x4) per instruction.  Operand lanes (measured, tools/probe/mfma_f64_layout.hip): A lane = 16 k + 4 b + i,
// B lane = 16 k + 4 b + j, D lane = 16 i + 4 b + j.  A group of 8 neighbours: lane l = 16 k + r loads the 16-byte slice (channel quad
// cq = r & 7) of neighbour slot ns = 4 (r >> 3) + k -- the loads of today, permuted -- and ONE coordinate word j = l & 3 of the same
// neighbour ({1, x, y, z}[j]); MFMA m = 0..3 takes the slice's m-th channel as A and that word as B, so that row (b, i) of D_m
// accumulates channel 4 cq + m against {1, x, y, z} over the neighbour slots of its half (r >> 3).  fp32 x fp32 products are exact in
// fp64 and the sums are fp64: the arithmetic class of kAcc = 1 in another order.  Per 8 neighbours: 5 conversions + 4 MFMAs (256 FMAs
// each) instead of 16 FMA + 7 conversions + 6 broadcast moves per lane; 4 accumulator registers pairs instead of 16; the fold of the
// two halves is one exchange across lane bit 3.  The matrix pipe's f64 rate equals the vector pipe's on this part (64.6 TFLOP/s
// measured), so what is saved is the conversions and moves, not the FMAs: see DESIGN 3.1 for the measurement.
// kDesc: the two clouds of a ragged pair (PairDesc, grid.h): size and feature table of cloud b from words 15 / 6-7 of its bounding-box
// record (grid_scan_kernel put them there), keypoint indices from the int32 copy pack_points_kernel made; feat4 / kp_index are unused.
template <int kAcc, bool kFma = false, bool kDesc = false>
__global__ __launch_bounds__(256) void ume_moments_kernel(
    const char* __restrict__ ws, size_t ws_stride, const float* __restrict__ kpts,
    const int64_t* __restrict__ kp_index, const float4* __restrict__ feat4, int N, int n_kp, int K, int cap,
    float radius, int flags, float* __restrict__ F, int32_t* __restrict__ nn_count,
    int64_t* __restrict__ nn_idx)
{
    const bool ordered = flags & UMEREG_MOMENTS_ORDERED;
    extern __shared__ int lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int b = blockIdx.y;
    const GridWs w = grid_ws(N);
    const char* wb = ws + b * ws_stride;
    int kp;
    if (ordered) {
        // XCD-aware: workgroup `blockIdx.x` runs on XCD blockIdx.x % 8 (observed dispatch rule, used
        // for speed only); give XCD x the x-th contiguous slab of the cell-sorted keypoint order.
        const int nblk = gridDim.x, xcd = blockIdx.x & 7, q = nblk >> 3, r = nblk & 7;
        const int lblk = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (blockIdx.x >> 3);
        const int slot = lblk * (blockDim.x >> 6) + wave;
        if (slot >= n_kp) return;
        kp = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(wb + w.off_kperm)[slot]);
    } else {
        kp = blockIdx.x * (blockDim.x >> 6) + wave;
        if (kp >= n_kp) return;
    }
    int* lst = lds + wave * cap;
    const float4* Pb = reinterpret_cast<const float4*>(wb + w.off_p4o);
    const float4* P4s = reinterpret_cast<const float4*>(wb + w.off_p4s);
    const int* start = reinterpret_cast<const int*>(wb + w.off_start);
    const Grid g = load_grid(reinterpret_cast<const unsigned int*>(wb + w.off_bbox), radius, N);
    // a ragged pair (kDesc): this cloud's feature table where the caller left it, n_live <= N points
    const unsigned int* __restrict__ rec = reinterpret_cast<const unsigned int*>(wb + w.off_bbox);
    const int n_live = kDesc ? (int)rec[15] : N;
    // (a native vector type: HIP's float4 is a class, whose assignment cannot bind a reference into address space 1)
    typedef float f4v __attribute__((ext_vector_type(4)));
    const UMEREG_GLOBAL_AS f4v* fb = global_ptr(kDesc ? reinterpret_cast<const f4v*>(((unsigned long long)rec[7] << 32) | rec[6])
                                                      : reinterpret_cast<const f4v*>(feat4) + (size_t)b * N * 8);
    auto feat_slice = [&](size_t k) __attribute__((always_inline)) { const f4v t = fb[k]; return make_float4(t.x, t.y, t.z, t.w); };
    float qx, qy, qz;
    if (kDesc || kp_index) {   // keypoint = point kp_index[kp] of this cloud (fused gather, evaluate.py:201-202)
        // (a ragged pair's indices: the int32 copy in the workspace, not the record's int64 list -- a base pointer loaded out of a record
        // cost this kernel 9 vector registers and its seventh wavefront per SIMD)
        const int64_t ki = kDesc ? (int64_t)reinterpret_cast<const int*>(wb + w.off_kpi)[kp] : kp_index[(size_t)b * n_kp + kp];
        if (ki < 0 || ki >= n_live) {
            // an index outside the cloud (stale, or the -1 padding the reference's own code produces) must not read out of
            // bounds: the keypoint's matrix is all NaN -- loud downstream, where torch indexing would have raised
            for (int e = lane; e < 128; e += kWave) F[((size_t)b * n_kp + kp) * 128 + e] = __int_as_float(0x7fc00000);
            if (nn_count && lane == 0) nn_count[(size_t)b * n_kp + kp] = 0;
            if (nn_idx) for (int e = lane; e < K; e += kWave) nn_idx[((size_t)b * n_kp + kp) * K + e] = -1;
            return;
        }
        const float4 qp = Pb[ki];
        qx = qp.x; qy = qp.y; qz = qp.z;
    } else {
        const float* q = kpts + ((size_t)b * n_kp + kp) * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    const int nbits = 32 - __clz(N > 1 ? N - 1 : 1);

    const int count = ball_search_grid<kFma>(P4s, start, g, qx, qy, qz, radius * radius, K, n_live, nbits, lst, cap, lane);

    if (nn_count && lane == 0) nn_count[(size_t)b * n_kp + kp] = count;
    if (nn_idx) {   // optional parity output, ascending like ball_query
        sort_kept(lst, count, lane);
        int64_t* o = nn_idx + ((size_t)b * n_kp + kp) * K;
        for (int e = lane; e < K; e += kWave) o[e] = e < count ? (int64_t)lst[e] : (int64_t)-1;
    }

    constexpr bool kF64 = kAcc != 0;
#ifndef UMEREG_MOM_ABLATE
#define UMEREG_MOM_ABLATE 0   // timing experiments only (results are wrong by construction): 1 = no gather / accumulation (the search alone);
                              // matrix-pipe path: 2 = the accumulate loop without its gathers (list reads, conversions and MFMAs on made-up
                              // operands), 4 = with the gathers but without conversions / MFMAs (five fp32 adds per group instead), 6 = both
                              // (the loop's list reads and control flow alone) -- profiles/r06/mom_split.txt
#endif
#ifndef UMEREG_MOM_MFMA_UNROLL
#define UMEREG_MOM_MFMA_UNROLL 4      // groups of 8 neighbours whose loads are in flight together (tools/exp_mom_acc.py measures alternatives)
#endif
    if (kAcc == 2) {
        // ---- fp64 sums on the matrix pipe (see above) ----
        constexpr int kMU = UMEREG_MOM_MFMA_UNROLL;
        const int mk = lane >> 4, mr = lane & 15, mcq = mr & 7, mns = 4 * (mr >> 3) + mk, mj = lane & 3;
        const float* Pf = reinterpret_cast<const float*>(Pb);
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        auto mtrip = [&](int e0, bool ragged, auto U_) __attribute__((always_inline)) {
            constexpr int kU = decltype(U_)::value;
            float4 ff[kU];
            float pc[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const unsigned int jn = (unsigned int)lst[min(e0 + u * 8 + mns, count - 1)];
                if (UMEREG_MOM_ABLATE & 2) {
                    const float v = __uint_as_float(0x3f800000u | (jn & 0xffffu));
                    ff[u] = make_float4(v, v + 1.f, v + 2.f, v + 3.f);
                    pc[u] = v;
                    continue;
                }
                ff[u] = feat_slice((size_t)jn * 8 + mcq);
                pc[u] = Pf[(size_t)jn * 4 + (mj > 0 ? mj - 1 : 0)];
            }
            if (UMEREG_MOM_ABLATE & 4) {
                float t = 0.f;
#pragma unroll
                for (int u = 0; u < kU; ++u) t += ((ff[u].x + ff[u].y) + (ff[u].z + ff[u].w)) + pc[u];
                acc[0] += (double)t;
                return;
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                if (ragged) {
                    const bool v = e0 + u * 8 + mns < count;
                    ff[u].x = v ? ff[u].x : 0.f; ff[u].y = v ? ff[u].y : 0.f;
                    ff[u].z = v ? ff[u].z : 0.f; ff[u].w = v ? ff[u].w : 0.f;
                }
                const double bq = mj == 0 ? 1.0 : (double)pc[u];
                acc[0] = __builtin_amdgcn_mfma_f64_4x4x4f64((double)ff[u].x, bq, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_4x4x4f64((double)ff[u].y, bq, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f64_4x4x4f64((double)ff[u].z, bq, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f64_4x4x4f64((double)ff[u].w, bq, acc[3], 0, 0, 0);
            }
        };
        const int mfull = (UMEREG_MOM_ABLATE & 1) ? 0 : (count / (8 * kMU)) * (8 * kMU);
        for (int e0 = 0; e0 < mfull; e0 += 8 * kMU) mtrip(e0, false, std::integral_constant<int, kMU>{});
        if (!(UMEREG_MOM_ABLATE & 1))
        for (int e0 = mfull; e0 < count; e0 += 8) mtrip(e0, e0 + 8 > count, std::integral_constant<int, 1>{});
        // D lane = 16 i + 4 b + j: channel 4 ((4 b + i) & 7) + m, column j, the neighbour half b >> 1 -- the halves differ in lane bit 3
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m] += shfl_xor_f64(acc[m], 8);
        // normaliser: sum over the 32 channels of column 0 (evaluate.py:59): the j = 0 lanes of the lower half, all four m
        const bool lower = (lane & 8) == 0;
        double s = (lower && mj == 0) ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : 0.0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) s += shfl_xor_f64(s, m);
        const double inv_den = (flags & UMEREG_MOMENTS_RAW) ? 1.0 : 1.0 / (s + 1e-6);
        if (lower) {
            const int di = lane >> 4, db = (lane >> 2) & 1, dcq = 4 * db + di;      // (b < 2 here: (4 b + i) & 7 = 4 b + i)
            float* o = F + (((size_t)b * n_kp + kp) * 32 + 4 * dcq) * 4 + mj;
#pragma unroll
            for (int m = 0; m < 4; ++m) o[m * 4] = (float)(acc[m] * inv_den);
        }
        return;
    }
    const int slot = lane >> 3;  // neighbour slot 0..7
    const int qd = lane & 7;     // channel quad: channels 4*qd .. 4*qd+3
    double a0[4] = {0, 0, 0, 0}, ax[4] = {0, 0, 0, 0}, ay[4] = {0, 0, 0, 0}, az[4] = {0, 0, 0, 0};
    typedef float f2v __attribute__((ext_vector_type(2)));
    f2v b0[2] = {{0.f, 0.f}, {0.f, 0.f}}, bx[2] = {{0.f, 0.f}, {0.f, 0.f}}, by[2] = {{0.f, 0.f}, {0.f, 0.f}}, bz[2] = {{0.f, 0.f}, {0.f, 0.f}};
    // One trip = 8 slots x kMomUnroll neighbours.  No per-element branches: the list index is clamped (slots past
    // the end re-read the last neighbour) and, in the single ragged trip, their features are zeroed by selects;
    // the LDS reads and the gathers of a trip are all issued before the first use.  (Prefetching the next trip
    // while accumulating the current one was measured: 0.151 vs 0.125 ms -- the extra registers cost a wave per SIMD.)
    auto trip = [&](int e0, bool ragged, auto U_) __attribute__((always_inline)) {
        constexpr int kU = decltype(U_)::value;
        unsigned int jj[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) jj[u] = (unsigned int)lst[min(e0 + u * 8 + slot, count - 1)];
        float4 pp[kU], ff[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            // the 8 lanes of a slot need the SAME neighbour's coordinates: one of them loads (the gather returns 128 B per
            // wave instead of 1 KiB), the others get them by two DPP moves per word (lane 0 of the quad, then quad 0 -> quad 1)
            pp[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qd == 0) pp[u] = Pb[jj[u]];
            ff[u] = feat_slice((size_t)jj[u] * 8 + qd);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            pp[u].x = bcast8(pp[u].x);
            pp[u].y = bcast8(pp[u].y);
            pp[u].z = bcast8(pp[u].z);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (ragged) {
                const bool v = e0 + u * 8 + slot < count;
                ff[u].x = v ? ff[u].x : 0.f; ff[u].y = v ? ff[u].y : 0.f;
                ff[u].z = v ? ff[u].z : 0.f; ff[u].w = v ? ff[u].w : 0.f;
            }
            if (kF64) {
                const double x = pp[u].x, y = pp[u].y, z = pp[u].z;
                const double f[4] = {ff[u].x, ff[u].y, ff[u].z, ff[u].w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    a0[c] += f[c];
                    ax[c] = fma(f[c], x, ax[c]);
                    ay[c] = fma(f[c], y, ay[c]);
                    az[c] = fma(f[c], z, az[c]);
                }
            } else {
                const float dx = pp[u].x - qx, dy = pp[u].y - qy, dz = pp[u].z - qz;
                const f2v f01 = {ff[u].x, ff[u].y}, f23 = {ff[u].z, ff[u].w};
                const f2v dx2 = {dx, dx}, dy2 = {dy, dy}, dz2 = {dz, dz};
                b0[0] += f01;
                b0[1] += f23;
                bx[0] = __builtin_elementwise_fma(f01, dx2, bx[0]);
                bx[1] = __builtin_elementwise_fma(f23, dx2, bx[1]);
                by[0] = __builtin_elementwise_fma(f01, dy2, by[0]);
                by[1] = __builtin_elementwise_fma(f23, dy2, by[1]);
                bz[0] = __builtin_elementwise_fma(f01, dz2, bz[0]);
                bz[1] = __builtin_elementwise_fma(f23, dz2, bz[1]);
            }
        }
    };
    // full trips of 8 x kMomUnroll neighbours, then the tail in trips of 8 (a single ragged 32-neighbour trip wasted half a
    // trip per keypoint on average)
    const int full = (UMEREG_MOM_ABLATE & 1) ? 0 : count & ~(8 * kMomUnroll - 1);
    for (int e0 = 0; e0 < full; e0 += 8 * kMomUnroll) trip(e0, false, std::integral_constant<int, kMomUnroll>{});
    if (!(UMEREG_MOM_ABLATE & 1))
        for (int e0 = full; e0 < count; e0 += 8) trip(e0, e0 + 8 > count, std::integral_constant<int, 1>{});
    if (!kF64) {
        a0[0] = b0[0].x; a0[1] = b0[0].y; a0[2] = b0[1].x; a0[3] = b0[1].y;
        ax[0] = bx[0].x; ax[1] = bx[0].y; ax[2] = bx[1].x; ax[3] = bx[1].y;
        ay[0] = by[0].x; ay[1] = by[0].y; ay[2] = by[1].x; ay[3] = by[1].y;
        az[0] = bz[0].x; az[1] = bz[0].y; az[2] = bz[1].x; az[3] = bz[1].y;
    }
    // fold the 8 neighbour slots (lanes that share qd differ in bits 3..5)
#pragma unroll
    for (int m = 8; m < 64; m <<= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a0[c] += shfl_xor_f64(a0[c], m);
            ax[c] += shfl_xor_f64(ax[c], m);
            ay[c] += shfl_xor_f64(ay[c], m);
            az[c] += shfl_xor_f64(az[c], m);
        }
    }
    if (!kF64) {
        // back from keypoint-centred to absolute coordinates: sum f p^T = sum f (p - c)^T + (sum f) c^T
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            ax[c] = fma(a0[c], (double)qx, ax[c]);
            ay[c] = fma(a0[c], (double)qy, ay[c]);
            az[c] = fma(a0[c], (double)qz, az[c]);
        }
    }
    // normaliser: sum over the 32 channels of F0 (evaluate.py:59), + 1e-6
    double s = (a0[0] + a0[1]) + (a0[2] + a0[3]);
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) s += shfl_xor_f64(s, m);
    // UMEREG_MOMENTS_RAW: the un-normalised matrix of generate_ume_from_keypoints2 (utils/loc_utils.py:160-162)
    // one fp64 division per keypoint, then 16 multiplications: a * (1 / den) differs from a / den by <= 1 ulp of fp64 before
    // the rounding to fp32 (the 16 IEEE divisions were 230 of the kernel's ~3 000 instructions per keypoint)
    const double inv_den = (flags & UMEREG_MOMENTS_RAW) ? 1.0 : 1.0 / (s + 1e-6);
    if (slot == 0) {
        float4* o = reinterpret_cast<float4*>(F + (((size_t)b * n_kp + kp) * 32 + 4 * qd) * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            o[c] = make_float4((float)(a0[c] * inv_den), (float)(ax[c] * inv_den), (float)(ay[c] * inv_den),
                               (float)(az[c] * inv_den));
    }
}

// ---- host side ---------------------------------------------------------------------------------
// the moment kernel's launch; desc (device pointer, optional): the two clouds of a ragged pair (B = 2, N = the capacity)
int launch_moments(const void* packed, const float* kpts, const int64_t* kp_index, const float* feat, int B, int N, int n_kp, int K,
                   float radius, int flags, float* F, int32_t* nn_count, int64_t* nn_idx, hipStream_t st, const PairDesc* desc)
{
    int cap, waves;
    lds_plan(K, &cap, &waves);
    dim3 grid((n_kp + waves - 1) / waves, B);
    UMEREG_REQUIRE(!((flags & UMEREG_MOMENTS_ACC_F32) && (flags & UMEREG_MOMENTS_ACC_VALU)), "ume_moments: ACC_F32 and ACC_VALU exclude each other");
    UMEREG_REQUIRE(!((flags & UMEREG_MOMENTS_FMA_DIST) && (flags & (UMEREG_MOMENTS_ACC_F32 | UMEREG_MOMENTS_ACC_VALU))),
                   "ume_moments: FMA_DIST goes with the default accumulation only");
#define UMEREG_LAUNCH_MOMENTS(...)                                                                                                    \
    hipLaunchKernelGGL((ume_moments_kernel<__VA_ARGS__>), grid, dim3(kWave * waves), (size_t)waves * cap * sizeof(int), st,               \
                       (const char*)packed, grid_ws(N).total, kpts, kp_index, (const float4*)feat, N, n_kp, K, cap, radius, flags, F,   \
                       nn_count, nn_idx)
    UMEREG_REQUIRE(!desc || !(flags & (UMEREG_MOMENTS_FMA_DIST | UMEREG_MOMENTS_ACC_F32 | UMEREG_MOMENTS_ACC_VALU)),
                   "ume_moments: a ragged pair runs the default kernel only");
    if (desc)                                     // (the record itself was consumed by the structure build: see kDesc)
        UMEREG_LAUNCH_MOMENTS(2, false, true);
    else if (flags & UMEREG_MOMENTS_FMA_DIST)     // (opt-in: its own instantiation of the default accumulation, nothing added to the product kernel)
        UMEREG_LAUNCH_MOMENTS(2, true);
    else if (!(flags & (UMEREG_MOMENTS_ACC_F32 | UMEREG_MOMENTS_ACC_VALU)))
        UMEREG_LAUNCH_MOMENTS(2);
    else if (!(flags & UMEREG_MOMENTS_ACC_F32))
        UMEREG_LAUNCH_MOMENTS(1);
    else
        UMEREG_LAUNCH_MOMENTS(0);
#undef UMEREG_LAUNCH_MOMENTS
    UMEREG_CHECK_LAUNCH("ume_moments_kernel");
    return UMEREG_OK;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API int umereg_ume_moments_packed_f32(const void* packed, const float* kpts, const int64_t* kp_index,
                                             const float* feat, int B, int N, int n_kp, int feat_dim, int K,
                                             float radius, int flags, float* F, int32_t* nn_count, int64_t* nn_idx,
                                             void* stream)
{
    UMEREG_REQUIRE(packed && (kpts || kp_index) && feat && F, "ume_moments: null pointer (packed/kpts|kp_index/feat/F)");
    UMEREG_REQUIRE(feat_dim == UMEREG_FEAT_DIM,
                   "ume_moments: feature dim must be 32 like the reference (evaluate.py:55), got %d", feat_dim);
    UMEREG_REQUIRE(B > 0 && N > 0 && n_kp > 0, "ume_moments: B, N, n_kp must be positive (got %d, %d, %d)", B, N, n_kp);
    UMEREG_REQUIRE(K > 0 && K <= kMaxBallK, "ume_moments: K must be in [1, 7680] (got %d)", K);
    UMEREG_REQUIRE(radius > 0.f, "ume_moments: radius must be positive");
    UMEREG_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)F & 15) == 0 && ((uintptr_t)packed & 15) == 0,
                   "ume_moments: packed, feat and F must be 16-byte aligned");
    if (int rc = check_device()) return rc;
    return launch_moments(packed, kpts, kp_index, feat, B, N, n_kp, K, radius, flags, F, nn_count, nn_idx, (hipStream_t)stream, nullptr);
}

UMEREG_API int umereg_ume_moments_f32(const float* pts, const float* kpts, const float* feat, int B,
                                      int N, int n_kp, int feat_dim, int K, float radius, float* F,
                                      int32_t* nn_count, int64_t* nn_idx, void* workspace,
                                      size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(pts, "ume_moments: null pts");
    if (!workspace || workspace_bytes < umereg_ume_moments_workspace_bytes(B, N)) {
        set_error("ume_moments: workspace too small (%zu < %zu)", workspace_bytes,
                  umereg_ume_moments_workspace_bytes(B, N));
        return UMEREG_EWORKSPACE;
    }
    if (int rc = umereg_pack_points_f32(pts, B, N, radius, workspace, workspace_bytes, stream)) return rc;
    const bool ordered = keypoint_order_pays(N, n_kp);
    if (ordered)
        if (int rc = umereg_ume_keypoint_order(workspace, kpts, nullptr, B, N, n_kp, radius, stream)) return rc;
    return umereg_ume_moments_packed_f32(workspace, kpts, nullptr, feat, B, N, n_kp, feat_dim, K, radius, ordered ? UMEREG_MOMENTS_ORDERED : 0, F,
                                         nn_count, nn_idx, stream);
}
