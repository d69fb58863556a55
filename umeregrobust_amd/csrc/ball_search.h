// ball_search.h -- the ball search over the uniform grid (grid.h, built by grid.hip), shared by a1 (ball_query.hip) and a1+a2
// (ume_moments.hip): device-inline code, and the host rules that size its LDS list.
//
//   search  one 64-lane wavefront per query; lanes stride each run (coalesced 1 KiB dwordx4 loads);
//           d2 = ((dx*dx)+(dy*dy))+(dz*dz), one rounding per operation (-ffp-contract=off), strict
//           d2 < r*r: the same predicate, bit for bit, as the reference loop.  "First K by index"
//           is kept exact by a streaming top-K on the ORIGINAL index: hits are appended to a per-wave
//           LDS list (ballot + mbcnt); when the list fills, a radix select finds the K-th smallest
//           index, the list is compacted to those K and later hits above the threshold are dropped.
#pragma once
#include <algorithm>
#include <type_traits>

#include "grid.h"

namespace umereg {

// ---- streaming top-K by original index ---------------------------------------------------------
// K-th smallest (1-based) of lst[0..cnt) -- distinct non-negative ints < 2^nbits -- by radix select.
__device__ __forceinline__ int select_kth(const int* lst, int cnt, int K, int nbits, int lane)
{
    int prefix = 0, need = K;
    for (int bit = nbits - 1; bit >= 0; --bit) {
        int zeros = 0;
        for (int e0 = 0; e0 < cnt; e0 += kWave) {
            const int e = e0 + lane;
            const int v = e < cnt ? lst[e] : -1;
            const bool z = e < cnt && ((v ^ prefix) >> (bit + 1)) == 0 && ((v >> bit) & 1) == 0;
            zeros += __popcll(__ballot(z));
        }
        if (need > zeros) { prefix |= 1 << bit; need -= zeros; }
    }
    return prefix;
}

// keep the entries <= thr (in place); returns the new count
__device__ __forceinline__ int compact_le(int* lst, int cnt, int thr, int lane)
{
    int out = 0;
    for (int e0 = 0; e0 < cnt; e0 += kWave) {
        const int e = e0 + lane;
        const int v = e < cnt ? lst[e] : 0x7fffffff;
        const bool keep = e < cnt && v <= thr;
        const unsigned long long m = __ballot(keep);
        __builtin_amdgcn_wave_barrier();
        if (keep) lst[out + mbcnt(m)] = v;   // out + prefix <= e: never clobbers an unread entry
        out += __popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
    return out;
}

// The same two steps with the list held in REGISTERS (lists of up to kSelRegs x 64 entries, i.e. wherever lds_plan's smallest list
// Kpad + (kScanUnroll + 1) * 64 fits them: K <= 960 with the defaults 20 and 4, every config of the reference).
// select_kth walks the LDS list once per bit -- 18 passes x 24 dependent reads for a 200 000-point cloud, ~50 000 cycles of a wavefront's
// life per selection -- and every saturated ball needs at least one (config 5: search 198 of the kernel's 248 us).  Here each lane
// reads its <= kSelRegs entries once (the reads in flight together), the K-th smallest index is found by bisection on the VALUE with
// one compare + ballot per entry and step (t = the largest value with fewer than K entries below it), and the survivors are written
// back from the registers.  Same threshold, same kept set; their ORDER in the list is the one compact_le gives (ascending position).
#ifndef UMEREG_SEL_REGS
#define UMEREG_SEL_REGS 20
#endif
constexpr int kSelRegs = UMEREG_SEL_REGS;
__device__ __forceinline__ int select_compact_regs(int* lst, int cnt, int K, int nbits, int lane, int& thr_out)
{
    int v[kSelRegs];
#pragma unroll
    for (int i = 0; i < kSelRegs; ++i) {
        const int e = i * kWave + lane;
        v[i] = e < cnt ? lst[e] : 0x7fffffff;
    }
    const int n_i = (cnt + kWave - 1) / kWave;                   // (wave-uniform)
    int t = 0;
    for (int bit = nbits - 1; bit >= 0; --bit) {
        const int trial = t | (1 << bit);
        int below = 0;
#pragma unroll
        for (int i = 0; i < kSelRegs; ++i)
            if (i < n_i) below += (int)__popcll(__ballot(v[i] < trial));
        if (below < K) t = trial;                                // fewer than K entries below `trial`: the K-th smallest is >= trial
    }
    thr_out = t;
    __builtin_amdgcn_wave_barrier();
    int out = 0;
#pragma unroll
    for (int i = 0; i < kSelRegs; ++i) {
        if (i < n_i) {
            const bool keep = v[i] <= t;                         // (the padding, INT_MAX, never is)
            const unsigned long long m = __ballot(keep);
            if (keep) lst[out + mbcnt(m)] = v[i];
            out += (int)__popcll(m);
        }
    }
    __builtin_amdgcn_wave_barrier();
    return out;
}

// keep the K smallest entries of lst[0..cnt) (cnt > K), -> the new count (= K: the entries are distinct) and the threshold
__device__ __forceinline__ int keep_k_smallest(int* lst, int cnt, int K, int nbits, int cap, int lane, int& thr)
{
    if (cap <= kSelRegs * kWave) return select_compact_regs(lst, cnt, K, nbits, lane, thr);
    thr = select_kth(lst, cnt, K, nbits, lane);
    return compact_le(lst, cnt, thr, lane);
}

// Grid search for one query.  Returns min(#hits, K); the kept ORIGINAL indices are in
// lst[0..count) in unspecified (deterministic) order.  lst has capacity cap >= K + (kScanUnroll + 1) * 64 (lds_plan).
// kFma (opt-in, UMEREG_BALL_FMA / UMEREG_MOMENTS_FMA_DIST): the squared distance as nvcc contracts pytorch3d's CUDA kernel
// (`dist2 += diff * diff` under -fmad=true): d2 = fma(dz, dz, fma(dy, dy, dx * dx)).  The reference's published numbers come from
// that build; the default (kFma = false) is the uncontracted CPU form `north_star` names.  The two differ in one neighbour of one
// ball in ~1e5 on off-lattice clouds (tools/soak_fma_boundary.py); the cell ranges' 1e-4 inflation covers either rounding.
template <bool kFma>
__device__ __forceinline__ float dist2_as_the_reference(float dx, float dy, float dz)
{
    if (kFma) return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    float d2 = dx * dx;
    d2 = d2 + dy * dy;
    d2 = d2 + dz * dz;
    return d2;
}

template <bool kFma = false>
__device__ __forceinline__ int ball_search_grid(const float4* __restrict__ P4s, const int* __restrict__ start,
                                                const Grid& g, float qx, float qy, float qz, float r2, int K,
                                                int n_eff, int nbits, int* lst, int cap, int lane)
{
    // the rows (y, z) of cells that intersect the ball, each clipped to the ball's chord in that row.  A point with d2 < r2
    // always lies in a visited cell: cell_axis is monotone, the ranges come from a radius inflated by 1e-4 (>> the rounding of
    // the coordinates involved), and a row's chord is computed from the row's distance to the query -- a lower bound of the
    // distance of every point in it (shrunk by 1e-4 for the same reason).
    const float rq = sqrtf(r2) * 1.0001f + 1e-20f;
    const int y0 = cell_axis(qy - rq, g.miny, g.invy, g.ny), y1 = cell_axis(qy + rq, g.miny, g.invy, g.ny);
    const int z0 = cell_axis(qz - rq, g.minz, g.invz, g.nz), z1 = cell_axis(qz + rq, g.minz, g.invz, g.nz);
    const float csy = 1.0f / g.invy, csz = 1.0f / g.invz;
    const float rq2 = rq * rq;
    int cnt = 0;
    int thr = n_eff - 1;   // accept original indices <= thr (lengths2: only the first n_eff points exist)
    // every row's run [beg, end) of the sorted table is looked up by ONE LANE, all rows at once (two dependent table reads per
    // row, one memory latency for all of them instead of one per row), then the rows are walked in order
    const int ny_r = y1 - y0 + 1, n_rows = ny_r * (z1 - z0 + 1);
    for (int r0 = 0; r0 < n_rows; r0 += kWave) {
        int my_beg = 0, my_end = 0;
        {
            const int r = r0 + lane;
            const int z = z0 + r / ny_r, y = y0 + r % ny_r;
            const float z_a = g.minz + (float)z * csz, z_b = z_a + csz;
            // (edge layers hold everything beyond them too: cell_axis clamps)
            const float dzc = fmaxf(fmaxf(z > 0 ? z_a - qz : 0.f, z < g.nz - 1 ? qz - z_b : 0.f), 0.f) * 0.9999f;
            const float y_a = g.miny + (float)y * csy, y_b = y_a + csy;
            const float dyc = fmaxf(fmaxf(y > 0 ? y_a - qy : 0.f, y < g.ny - 1 ? qy - y_b : 0.f), 0.f) * 0.9999f;
            const float rem = rq2 - dyc * dyc - dzc * dzc;
            if (r < n_rows && rem > 0.f) {
                const float sx = sqrtf(rem) * 1.0001f + 1e-20f;
                const int cbase = (z * g.ny + y) * g.nx;
                my_beg = start[cbase + cell_axis(qx - sx, g.minx, g.invx, g.nx)];
                my_end = start[cbase + cell_axis(qx + sx, g.minx, g.invx, g.nx) + 1];
            }
        }
        const int n_here = min(kWave, n_rows - r0);
        for (int rr = 0; rr < n_here; ++rr) {
            const int beg = __builtin_amdgcn_readlane(my_beg, rr);
            const int end = __builtin_amdgcn_readlane(my_end, rr);
            if (beg >= end) continue;                                     // (wave-uniform)
            // up to kScanUnroll chunks per trip, loads issued together: a serial load -> test -> load chain left the wave
            // waiting on L2 latency for half of its lifetime (SQ_WAIT_ANY 49 %); a row's tail of <= 2 chunks takes the 2-chunk
            // form (rows are ~100-250 points with the half-radius cells)
            auto scan = [&](int base, auto U_) __attribute__((always_inline)) {
                constexpr int U = decltype(U_)::value;
                float4 pv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int pos = base + u * kWave + lane;
                    pv[u] = P4s[pos < end ? pos : end - 1];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int pos = base + u * kWave + lane;
                    const float4 p = pv[u];
                    const int oi = __float_as_int(p.w);
                    const float dx = qx - p.x;
                    const float dy = qy - p.y;
                    const float dz = qz - p.z;
                    const float d2 = dist2_as_the_reference<kFma>(dx, dy, dz);
                    const bool hit = (pos < end) && (d2 < r2) && (oi <= thr);
                    const unsigned long long m = __ballot(hit);
                    if (m != 0ull) {   // wave-uniform
                        if (hit) lst[cnt + mbcnt(m)] = oi;
                        cnt += __popcll(m);
                    }
                }
            };
            // room for a whole trip is made BEFORE its loads are issued (keep the K smallest; cap >= K + kScanUnroll chunks): the
            // selection then runs with none of the trip's points in registers
            auto make_room = [&](int chunks) __attribute__((always_inline)) {
                if (cnt > cap - chunks * kWave) {
                    __builtin_amdgcn_wave_barrier();
                    cnt = keep_k_smallest(lst, cnt, K, nbits, cap, lane, thr);
                }
            };
            int base = beg;
            for (; end - base > 2 * kWave; base += kWave * kScanUnroll) { make_room(kScanUnroll); scan(base, std::integral_constant<int, kScanUnroll>{}); }
            if (base < end) { make_room(2); scan(base, std::integral_constant<int, 2>{}); }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (cnt > K) cnt = keep_k_smallest(lst, cnt, K, nbits, cap, lane, thr);
    return cnt;
}

// ascending bitonic sort of lst[0..n_pow2) (entries beyond the live count must hold INT_MAX)
__device__ __forceinline__ void bitonic_sort(int* lst, int n_pow2, int lane)
{
    for (int k = 2; k <= n_pow2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __builtin_amdgcn_wave_barrier();
            for (int t = lane; t < (n_pow2 >> 1); t += kWave) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // index with bit j clear
                const int hi = lo | j;
                const bool up = (lo & k) == 0;
                const int a = lst[lo], b = lst[hi];
                if ((a > b) == up) { lst[lo] = b; lst[hi] = a; }
            }
        }
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void sort_kept(int* lst, int count, int lane)
{
    int n_pow2 = 64;
    while (n_pow2 < count) n_pow2 <<= 1;
    for (int e = count + lane; e < n_pow2; e += kWave) lst[e] = 0x7fffffff;
    bitonic_sort(lst, n_pow2, lane);
}

// ---- host side ---------------------------------------------------------------------------------
// per-wave LDS list capacity and waves per workgroup for a given K
constexpr void lds_plan(int K, int* cap, int* waves)
{
    const int Kpad = (K + 63) / 64 * 64;
    // the list: >= K + a trip of kScanUnroll chunks + one (room is made before a trip's loads are issued); twice K + a chunk where that is
    // more (fewer selections).  A list that can fit the in-register selection (kSelRegs entries per lane: cap_min <= reg_cap, which is
    // K <= 960 with the defaults kSelRegs = 20, kScanUnroll = 4 -- the reference's 750 is inside) is capped at what fits; K = 961 is the first
    // plan whose selection walks the LDS list.  Measured (tools/exp_mom_time.py, us per pair SY / KT / NS; selection in LDS: 242 / 103 /
    // 47): 25 registers (list 1 600) 149 / 108 / 50, 20 (1 280) 158 / 103 / 48 -- five registers more cost KT its eighth wavefront.
    const int reg_cap = kSelRegs * kWave, cap_min = Kpad + (kScanUnroll + 1) * kWave;
    const int cap_big = std::max(2 * Kpad + 64, cap_min);
    *cap = cap_min <= reg_cap ? std::min(reg_cap, cap_big) : cap_big;
    *waves = (*cap) * 4 * 4 <= 48 * 1024 ? 4 : ((*cap) * 4 * 2 <= 64 * 1024 ? 2 : 1);
}

// The largest K the entries accept (their messages print it as 7680).  It is tied to the plan above: at this K a wavefront's list is
// 2 * Kpad + 64 ints, one wavefront per workgroup, and the workgroup's lists must fit the 64 KiB of LDS a launch may ask for.
constexpr int kMaxBallK = 7680;
static_assert([] { int cap = 0, waves = 0; lds_plan(kMaxBallK, &cap, &waves); return (size_t)waves * cap * sizeof(int) <= 64 * 1024; }(),
              "the LDS lists that lds_plan sizes for kMaxBallK exceed 64 KiB");

// Are the keypoints processed in cell order (launch_query_order, UMEREG_MOMENTS_ORDERED)?  Only if the order fits its buffer (Npad
// entries), and not for a handful of keypoints, where the extra launch costs more than the locality gains.
inline bool keypoint_order_pays(int N, int n_kp) { return n_kp <= grid_ws(N).Npad && n_kp >= 64; }

// the fused search + gather + moment kernel over a structure built by launch_prep (arguments as umereg_ume_moments_packed_f32);
// ume_moments.hip
int launch_moments(const void* packed, const float* kpts, const int64_t* kp_index, const float* feat, int B, int N, int n_kp, int K,
                   float radius, int flags, float* F, int32_t* nn_count, int64_t* nn_idx, hipStream_t st, const PairDesc* desc = nullptr);

}  // namespace umereg
