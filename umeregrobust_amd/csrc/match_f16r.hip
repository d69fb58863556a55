// match_f16r.hip -- a4 as the product runs it, the filter + refine matcher (precision "f16r"): a coarse pass on the f16
// MFMA pipe keeps, per source row, the few targets that can win (two kernels for the same job: the Q-form, default, and
// the projector form with its packer), and a refine pass re-evaluates those in fp64 and takes the row arg-min.
// Both passes are one translation unit on purpose: pform_pack_kernel and match_refine_kernel share the offset helpers of
// qlayout.h, and the compiler propagates the value ranges of ALL call sites in a unit into such a helper before it
// inlines it.  Compiled without the packer beside it, match_refine_kernel knows its target index to be below 2^27 and
// comes out as other code (<16,512>: 1054 instructions / 104 VGPRs against 1005 / 124).  Nobody has timed that variant;
// until somebody does, the kernels stay together and the code stays what was measured (profiles/split_match/isa_identity.txt).
#include <type_traits>

#include "common.h"
#include "match_dev.h"
#include "qlayout.h"

namespace umereg {

// ---- filter + refine matching (precision "f16r") ---------------------------------------------------
// The arg-min only needs the exact distance of the few targets that can win.  A COARSE pass runs the
// contraction with the hi planes alone (one f16 MFMA product instead of three) and appends, per source
// row, every target whose coarse score s~ = |Qi^T Qj|_F^2 comes within a margin of the best coarse score
// seen so far; a REFINE pass re-evaluates just those candidates in fp64 from hi+lo and takes the arg-min
// (lowest index on ties).  The result is the arg-min of the fp64 distance over ALL targets because:
//   * |lo| <= 2^-11 |q| and the basis columns have unit norm, so each of the 16 entries of Qi^T Qj
//     changes by at most 2 * 2^-11 when the lo planes are dropped; with sum|c| <= 4 |C|_F <= 8 this
//     moves s by at most delta = 2 * 2^-10 * 8 = 2^-6 (+ fp32 accumulation noise ~1e-5);
//   * every per-lane / per-row / global limit is (some coarse score of that row) - margin, hence
//     <= (coarse row maximum) - margin, and the exact winner's coarse score is >= coarse row maximum -
//     2 delta; margin >= 2 delta therefore keeps the exact winner (and everything tied with it) in the list.
// Limits are shared between lanes, waves and workgroups only to keep the lists short (~20 entries per
// row): sharing is timing dependent, the RESULT is not.  Every (wave of the coarse kernel, target split)
// owns a private region of the candidate buffer, so candidates are appended with plain stores -- no
// atomics, nothing the tile loop has to wait for.  A region that overflows (hundreds of exact duplicates
// among the targets) makes the refine kernel re-scan that block of rows exhaustively.
constexpr float kCoarseMargin = 0.03125f + 0.0009765625f;   // 2 delta + slack
// EARLY EXIT.  s~ = sum_b |Qi~^T q~jb|^2 is accumulated column by column of the target basis, and each term is bounded by
// |Qi~|_2^2 |q~jb|^2 with Qi~, q~jb the hi planes: |hi - q| <= 2^-11 |q| entry by entry, so a unit column keeps a norm <= 1 + 2^-11 and
// |Qi~|_2 <= |Qi|_2 + |Qi~ - Qi|_F <= 1 + 2 * 2^-11.  A term is therefore <= (1 + 2^-10)^2 (1 + 2^-11)^2 < 1.00294, and the fp32
// accumulation of its 32 + 4 terms adds < 1e-5: after m columns  s~ <= s~_partial(m) + (4 - m) c  with any c >= 1.00295.  c is that
// rounded up to 1 + 2^-8; the 9.5e-4 to spare per column also cover the rounding of the test itself, which is evaluated as
// (s~_partial - lim) >= -(4 - m) c in fp32.  A tile whose every (row, target) fails that test can append nothing (s~ >= lim fails) and
// can raise no limit (s~ - margin < lim): it is dropped, filter() included, and everything the proof above rests on still holds.
// The test only bites when rows that sit together share their good targets and meet one early -- the slot order of qlayout.h.
constexpr float kCoarseTermMax = 1.00390625f;
#ifndef UMEREG_COARSE_EXIT
#define UMEREG_COARSE_EXIT 3   // bit 0: test after column 0, bit 1: after columns 0-1, bit 2: column 1's MFMAs are issued before the first test
#endif

// all-reduce (max) over aligned groups of 32 lanes: DPP inside rows of 16, one swizzle across the two rows
__device__ __forceinline__ float group32_max(float v)
{
    int x = __float_as_int(v);
    x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_mov_dpp(x, 0xB1, 0xf, 0xf, true))));    // quad_perm [1,0,3,2]
    x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x4E, 0xf, 0xf, true))));    // quad_perm [2,3,0,1]
    x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x141, 0xf, 0xf, true))));   // row_half_mirror
    x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x140, 0xf, 0xf, true))));   // row_mirror
    x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_ds_swizzle(x, 0x401F))));             // lane ^ 16
    return __int_as_float(x);
}

// Workgroup = 4 waves x 32 source keypoints (four stationary A tiles per wave, hi planes only); every
// 32-target tile (8 KiB of hi fragments) is staged once per workgroup through a double-buffered LDS
// stage.  The tile body is software-pipelined by hand in units of "groups" (one basis column b x two A
// tiles = 4 MFMAs): the squares of group k run in the shadow of the MFMAs of group k+1.
#ifndef UMEREG_COARSE_ABLATE
#define UMEREG_COARSE_ABLATE 0   // timing experiments only (tools/exp_coarse_ablate.sh; results are wrong by construction): 1 no squares, 2 no filter, 4 no MFMAs, 8 no LDS reads, 16 every tile stops at the first test (the floor of the early exit)
#endif
#ifndef UMEREG_COARSE_TPS
#define UMEREG_COARSE_TPS 2   // round 7, with the early exit: 2 against 1 -- the same kernel time, fewer candidates (profiles/r07/coarse_skip.txt); before: (2: 140-146 us against 138-147, 4: 162 -- round-3 measurement: the barrier is not the bound either)
#endif
constexpr int kCoarseTPS = UMEREG_COARSE_TPS;        // target tiles staged (and consumed) per workgroup barrier

// Workgroup = 4 waves x kCoarseRows source keypoints (stationary A tiles, hi planes only); every 32-target
// tile (8 KiB of hi fragments) is staged once per workgroup through a double-buffered LDS stage, two
// further tiles are in flight in registers.  A wave leaves a tile after one or two of its four column groups when the partial
// scores prove that nothing in it can reach a limit (kCoarseTermMax); the workgroup's barrier then waits for the waves that stay.
__global__ __launch_bounds__(kWave* kDistWaves, 2) void ume_coarse_h_kernel(
    const half8* __restrict__ Afrag, const half8* __restrict__ Bfrag, int n1, int n2, int n_ablk, int tile_lo, int tile_mid, int tile_hi,
    int lead_tps, int lead_splits, int tiles_per_split, int sp0, MatchScratch ms)
{
    // this launch: the target tiles [tile_lo, tile_mid) in lead_splits runs of lead_tps, then [tile_mid, tile_hi) in runs of
    // tiles_per_split; the candidate regions of the splits sp0, sp0 + 1, ... (CoarsePlan, match_dev.h)
    __shared__ half8 ldsB[2][kCoarseTPS * 512];             // 2 x (kCoarseTPS x 8 KiB): hi planes of kCoarseTPS 32-target tiles per barrier
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int ablk = blockIdx.x % n_ablk;
    const int spl = blockIdx.x / n_ablk;
    const int sp = sp0 + spl;
    const bool lead = spl < lead_splits;
    const int jt0 = lead ? tile_lo + spl * lead_tps : tile_mid + (spl - lead_splits) * tiles_per_split;
    const int jt1 = lead ? min(jt0 + lead_tps, tile_mid) : min(jt0 + tiles_per_split, tile_hi);
    const int h = lane >> 5;
    const int i_base = ablk * kCoarseWG + wave * kCoarseRows;

    half8 a[kCoarseTA][2];   // [A tile][k step], hi plane
#pragma unroll
    for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s)
            a[t][s] = Afrag[((((size_t)(ablk * (kCoarseWG / 8) + wave * kCoarseTA + t)) * 2 + s) * 2 + 0) * 64 + lane];

    // Limits, kept as the bit patterns of non-negative floats (integer max == float max, one instruction).
    // `seen` holds what other workgroups have published for this lane's rows; it is re-read
    // asynchronously (issued at one sharing point, consumed at the next) so that the tile loop never
    // waits for a global round trip.  Rows beyond n1 (zero bases, score 0) never reach 3e38.
    int lim[kCoarseTA][4];
    unsigned int seen[kCoarseTA][4];
#pragma unroll
    for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = i_base + t * 8 + 2 * g + h;
            seen[t][g] = __hip_atomic_load(ms.rowlim + min(i, n1 - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // what the splits before this one have published (the subsample's, in slot order) holds from the first tile on
            lim[t][g] = i < n1 ? max(__float_as_int(1.0e-30f), (int)seen[t][g]) : __float_as_int(3.0e38f);
        }
#pragma unroll
    for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) asm volatile("" ::"v"(a[t][s]));

    // this wave's private candidate region
    const int blk = ablk * kDistWaves + wave;
    unsigned int* const region = ms.cand + ((size_t)blk * ms.splits + sp) * kRegionCap;
    int qn = 0;   // wave-uniform number of candidates appended so far
    auto share = [&](bool reload) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float v = group32_max(__int_as_float(lim[t][g]));
                const int i = i_base + t * 8 + 2 * g + h;
                if ((lane & 31) == 0 && i < n1 && __float_as_uint(v) > seen[t][g]) atomicMax(ms.rowlim + i, __float_as_uint(v));
                lim[t][g] = max(__float_as_int(v), (int)seen[t][g]);
            }
        if (reload) {
#pragma unroll
            for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int i = min(i_base + t * 8 + 2 * g + h, n1 - 1);
                    seen[t][g] = __hip_atomic_load(ms.rowlim + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
    };

    // Staging: chunk c = r*256 + tid of the tile's 512 hi chunks; hi chunk (q = c>>6, l = c&63) sits at
    // fragment index (q*2 + 0)*64 + l.  A tile's loads are issued two tile-times before its LDS store.
    // A GROUP of kCoarseTPS tiles is staged and consumed per barrier.  (Round 3 asked whether one barrier per tile is what
    // the kernel waits for -- tools/exp_coarse_ablate.sh: 150 us as it is, 155 without its squares, 123 without its filter,
    // 100 without both, 105 without its MFMAs -- and the answer is no: two tiles per barrier measure the same, four are slower.)
    half8 st[kCoarseTPS][2];
    const int c0 = threadIdx.x, c1 = 256 + threadIdx.x;
    const int src0 = ((c0 >> 6) * 2) * 64 + (c0 & 63), src1 = ((c1 >> 6) * 2) * 64 + (c1 & 63);
    auto gload = [&](int jg) __attribute__((always_inline)) {          // the tiles jg .. jg + kCoarseTPS - 1 -> registers
#pragma unroll
        for (int q = 0; q < kCoarseTPS; ++q) {
            const int jt = min(jg + q, jt1 - 1);
            st[q][0] = Bfrag[(size_t)jt * 1024 + src0];
            st[q][1] = Bfrag[(size_t)jt * 1024 + src1];
        }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < kCoarseTPS; ++q) {
            ldsB[buf][q * 512 + c0] = st[q][0];
            ldsB[buf][q * 512 + c1] = st[q][1];
        }
    };
    if (jt0 < jt1) {
        gload(jt0);
        lstore(0);
    }
    if (jt0 + kCoarseTPS < jt1) gload(jt0 + kCoarseTPS);
    __syncthreads();
    int cur = 0;
    // The filter of a tile -- limit updates, hit tests, candidate appends: a dependent chain of compares, ballots and scalar
    // branches.  The ablations of tools/exp_coarse_ablate.sh say the squares overlap with the MFMAs completely and the filter
    // not at all, so round 3 tried to run it ONE TILE LATE, right after the first MFMAs of the next tile have been issued
    // (a limit that is one tile staler is still "some coarse score of that row - margin", the proof obligation is untouched):
    // 168 us against 143 -- the scheduling fences and the eight score registers carried across the tile cost more than the
    // shadow returns.  The variant is gone from the source (round 4); the measurement stays in DESIGN 3.3.
    // the sharing points are a property of the tile count, whether a tile ran to its end or not
    auto share_point = [&](const int jt) __attribute__((always_inline)) {
        const int kt = jt - jt0;
        if ((ms.share_mask >> (kt < 31 ? kt : 31)) & 1u) {
            if (kt < 31 || (kt & 31) == 31) share(true);
        }
    };
#if UMEREG_COARSE_STATS
    unsigned int n_stop1 = 0, n_stop2 = 0;
#endif
    // true: after `cols` columns no (row, target) of this wave's tile can still reach its limit (see kCoarseTermMax)
    auto hopeless = [&](const float (&sc)[kCoarseTA][4], const int cols) __attribute__((always_inline)) {
        float d = sc[0][0] - __int_as_float(lim[0][0]);
#pragma unroll
        for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) d = fmaxf(d, sc[t][g] - __int_as_float(lim[t][g]));
        const bool stop = __builtin_amdgcn_ballot_w64(!(d < -(float)(4 - cols) * kCoarseTermMax)) == 0ull;
        return (UMEREG_COARSE_ABLATE & 16) ? true : stop;
    };
    auto filter = [&](const int jt, const float (&sc)[kCoarseTA][4]) __attribute__((always_inline)) {
        if (UMEREG_COARSE_ABLATE & 2) {
            // no limits, no ballots, no candidates: the scores are folded into one register that is stored once at the end
#pragma unroll
            for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) lim[t][g] = max(lim[t][g], __float_as_int(sc[t][g]));
            return;
        }
#pragma unroll
        for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) lim[t][g] = max(lim[t][g], __float_as_int(sc[t][g] - kCoarseMargin));
        share_point(jt);
        unsigned long long hit[kCoarseTA][4], any = 0;
#pragma unroll
        for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                hit[t][g] = __builtin_amdgcn_ballot_w64(sc[t][g] >= __int_as_float(lim[t][g]));
                any |= hit[t][g];
            }
        if (__builtin_popcountll(any) > 8) {
            // a crowd of lanes hits at once: neighbouring targets are similar (the pair chain hands the targets over in cell
            // order, qlayout.h; a caller of the layered entries may have sorted them too) and
            // each lane only knows its own column's history.  Pool the limits of the 32 columns first, so that
            // only scores within the margin of this tile's row maximum remain.
#pragma unroll
            for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) lim[t][g] = __float_as_int(group32_max(__int_as_float(lim[t][g])));
            any = 0;
#pragma unroll
            for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    hit[t][g] = __builtin_amdgcn_ballot_w64(sc[t][g] >= __int_as_float(lim[t][g]));
                    any |= hit[t][g];
                }
        }
        if (any) {
            const unsigned int j = (unsigned int)(jt * 32 + (lane & 31));
#pragma unroll
            for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned long long mask = hit[t][g];
                    if (mask) {
                        const int pos = qn + mbcnt(mask);
                        if (((mask >> lane) & 1ull) && pos < kRegionCap)
                            region[pos] = ((unsigned int)(t * 8 + 2 * g + h) << 27) | j;
                        qn += __builtin_popcountll(mask);
                    }
                }
        }
    };
    auto tile = [&](const int jt, const int q) __attribute__((always_inline)) {
        const half8* const lB = &ldsB[cur][q * 512];
        float sc[kCoarseTA][4];    // coarse scores of this lane's 4*TA (source, target) pairs
        // one group: the 2 * kCoarseTA MFMAs of basis column b ...
        auto products = [&](const int b, f32x16 (&cc)[kCoarseTA]) __attribute__((always_inline)) {
            const half8 b0 = (UMEREG_COARSE_ABLATE & 8) ? a[0][0] : lB[(b * 2 + 0) * 64 + lane];
            const half8 b1 = (UMEREG_COARSE_ABLATE & 8) ? a[0][1] : lB[(b * 2 + 1) * 64 + lane];
            if (UMEREG_COARSE_ABLATE & 4) {
#pragma unroll
                for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
                    for (int e = 0; e < 16; ++e) cc[t][e] = (float)b0[e & 7] + (float)b1[(e + t) & 7];
            } else {
#pragma unroll
                for (int t = 0; t < kCoarseTA; ++t) cc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t][0], b0, f32x16{0}, 0, 0, 0);
#pragma unroll
                for (int t = 0; t < kCoarseTA; ++t) cc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t][1], b1, cc[t], 0, 0, 0);
            }
        };
        // ... and its squares
        auto squares = [&](const int b, const f32x16 (&cc)[kCoarseTA]) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < kCoarseTA; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (UMEREG_COARSE_ABLATE & 1) {
                        sc[t][g] = b == 0 ? cc[t][4 * g] : sc[t][g] + cc[t][4 * g + 1];
                        continue;
                    }
                    // scalar FMAs on purpose: packed f32 VALU beside MFMAs is slower on gfx950
                    float acc = b == 0 ? cc[t][4 * g] * cc[t][4 * g] : fmaf(cc[t][4 * g], cc[t][4 * g], sc[t][g]);
                    acc = fmaf(cc[t][4 * g + 1], cc[t][4 * g + 1], acc);
                    acc = fmaf(cc[t][4 * g + 2], cc[t][4 * g + 2], acc);
                    sc[t][g] = fmaf(cc[t][4 * g + 3], cc[t][4 * g + 3], acc);
                }
        };
        constexpr bool kTest1 = (UMEREG_COARSE_EXIT & 1) && !(UMEREG_COARSE_ABLATE & 15), kTest2 = (UMEREG_COARSE_EXIT & 2) && !(UMEREG_COARSE_ABLATE & 15);
        constexpr bool kAhead = (UMEREG_COARSE_EXIT & 4) != 0;   // column 1's MFMAs in flight while column 0 is squared and tested
        f32x16 c0[kCoarseTA], c1[kCoarseTA];
        products(0, c0);
        if (kAhead || !kTest1) products(1, c1);
        squares(0, c0);
        if (kTest1 && hopeless(sc, 1)) {
#if UMEREG_COARSE_STATS
            ++n_stop1;
#endif
            share_point(jt);
            return;
        }
        if (!kAhead && kTest1) products(1, c1);
        squares(1, c1);
        if (kTest2 && hopeless(sc, 2)) {
#if UMEREG_COARSE_STATS
            ++n_stop2;
#endif
            share_point(jt);
            return;
        }
#pragma unroll
        for (int b = 2; b < 4; ++b) {
            f32x16 cc[kCoarseTA];
            products(b, cc);
            squares(b, cc);
        }
        filter(jt, sc);
    };
    for (int jg = jt0; jg < jt1; jg += kCoarseTPS) {
#pragma unroll
        for (int q = 0; q < kCoarseTPS; ++q)
            if (jg + q < jt1) tile(jg + q, q);
        // the next group (loaded one group ago) into the other buffer, the one after it into the registers
        if (jg + kCoarseTPS < jt1) lstore(cur ^ 1);
        if (jg + 2 * kCoarseTPS < jt1) gload(jg + 2 * kCoarseTPS);
        __syncthreads();
        cur ^= 1;
    }
    // publish what this split learned for the workgroups that start later
    share(false);
    if (lane == 0) ms.cnt[(size_t)blk * ms.splits + sp] = (unsigned int)qn;
#if UMEREG_COARSE_STATS
    if (lane == 0) {
        atomicAdd(ms.stats + 0, (unsigned long long)max(jt1 - jt0, 0));
        atomicAdd(ms.stats + 1, (unsigned long long)n_stop1);
        atomicAdd(ms.stats + 2, (unsigned long long)n_stop2);
        atomicAdd(ms.stats + 3, (unsigned long long)qn);
    }
#endif
}

// ---- P-form coarse filter ---------------------------------------------------------------------------------------------
// The Q-form kernel above is bound by its VALU epilogue (16 squares per (source, target) pair: ~13 VALU instructions
// per MFMA, MFMA pipe 1/3 busy).  The same score as ONE inner product per pair needs no squares at all:
//     s = |Qi^T Qj|_F^2 = <Pi, Pj>_F,   P = Q Q^T (32 x 32, symmetric)
// packed as the 528 entries of the upper triangle, off-diagonals scaled by sqrt(2) -> K = 528 (33 k-steps of 16):
// 1.03x the MFMA work of the Q-form, one accumulator per pair, and the epilogue is the three
// limit instructions per pair.  Packing order: k = 32 d + u holds P[u][(u + d) & 31] for the wrapped diagonals
// d = 0..15 (every unordered pair once), k = 512 + u (u < 16) holds P[u][u + 16].
// Error of the coarse score: the packed entries are f16-rounded from fp32 (|dP|_F <= 2^-11 |P|_F + 1e-5, |P|_F = 2), so
// |s~ - s| <= 2 |dP|_F |P|_F = 2^-8 (+ fp32 accumulation of 544 terms <= 2.6e-4): delta = 4.3e-3 against the Q-form's 2^-6.
constexpr float kCoarseMarginP = 0.009765625f;   // 2 delta + slack
constexpr int kPDepth = 5;                   // B fragments in flight LDS -> registers per wave
constexpr int kQsStride = 33;                // float4 per keypoint in the packer's LDS (32 rows + 1)

// Q (split-f16 fragment order, hi + lo) -> packed projector fragments.  One workgroup per tile of 32 keypoints;
// fragment (tile, ks) = 64 lanes x 8 halfs: lane l = keypoint (l & 31), k = 16 ks + 8 (l >> 5) + e -- the A and the B
// operand order of v_mfma_f32_32x32x16_f16 alike, so both sets use the same layout.
__global__ __launch_bounds__(256) void pform_pack_kernel(const _Float16* __restrict__ Ah, const _Float16* __restrict__ Bh, int n1,
                                                         int n2, int tiles1, int tiles2, half8* __restrict__ PA,
                                                         half8* __restrict__ PB)
{
    __shared__ float4 qs[32 * kQsStride];
    const int side = blockIdx.y, tile = blockIdx.x;
    if (tile >= (side ? tiles2 : tiles1)) return;
    const int n = side ? n2 : n1;
    const _Float16* const Q = side ? Bh : Ah;
    half8* const P = (side ? PB : PA) + (size_t)tile * kPK * 64;
    const int tid = threadIdx.x;
    if (tile * 32 >= n) {   // padding tiles: zero fragments, nothing read
        for (int o = tid; o < kPK * 64; o += 256) P[o] = half8{0};
        return;
    }
    float* const qf = reinterpret_cast<float*>(qs);
    for (int c = tid; c < 512; c += 256) {   // chunk = (keypoint, basis column, 8 channels)
        const int kp = c & 31, a = (c >> 5) & 3, k8 = c >> 7;
        const int i = tile * 32 + kp;
        half8 vh = half8{0}, vl = half8{0};
        if (i < n) {
            const size_t off0 = side ? hoff_cols(i, a, k8 * 8, 0) : hoff_rows(i, a, k8 * 8, 0);
            const size_t off1 = side ? hoff_cols(i, a, k8 * 8, 1) : hoff_rows(i, a, k8 * 8, 1);
            vh = *reinterpret_cast<const half8*>(Q + off0);
            vl = *reinterpret_cast<const half8*>(Q + off1);
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) qf[(kp * kQsStride + k8 * 8 + x) * 4 + a] = (float)vh[x] + (float)vl[x];   // as the refine pass reads it
    }
    __syncthreads();
    for (int o = tid; o < kPK * 64; o += 256) {
        const int ks = o >> 6, l = o & 63, kp = l & 31, c = ks * 2 + (l >> 5);
        half8 out = half8{0};
        if (c < 66) {
            const int d = c < 64 ? c >> 2 : 16, u0 = c < 64 ? (c & 3) * 8 : (c - 64) * 8;
            const float w = d == 0 ? 1.0f : 1.41421356237f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float4 qu = qs[kp * kQsStride + u0 + e], qv = qs[kp * kQsStride + ((u0 + e + d) & 31)];
                out[e] = (_Float16)(w * fmaf(qu.x, qv.x, fmaf(qu.y, qv.y, fmaf(qu.z, qv.z, qu.w * qv.w))));
            }
        }
        P[o] = out;
    }
}

// Workgroup = 8 waves (two per SIMD) x 32 source keypoints: one stationary A tile of 33 fragments per wave, held in
// AGPRs (the MFMA reads either register file) next to the accumulators; limits and the B ring live in VGPRs.  A panel =
// 32 targets x 33 fragments (33 KiB) goes global -> LDS directly, once per workgroup, double-buffered, and is read by
// all 8 waves.  A wave's MFMAs form ONE dependent accumulator chain (measured: ~47 cycles per dependent
// v_mfma_f32_32x32x16_f16 against 32 of issue), so the SIMD's second wave is what fills the matrix pipe, and its MFMAs
// are also what covers this wave's candidate bookkeeping after each panel.
__global__ __launch_bounds__(kWave* kPWaves, 2) void ume_coarse_p_kernel(const half8* __restrict__ PA, const half8* __restrict__ PB,
                                                                        int n1, int n2, int n_ablk, int n_btiles,
                                                                        int tiles_per_split, MatchScratch ms)
{
    __shared__ half8 ldsB[3][kPK * 64];   // 3 x 33 KiB: the panel in use, the next one, the one being staged
    __shared__ __attribute__((aligned(16))) unsigned int seenL[kPWaves][32];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = lane_id();
    const int ablk = blockIdx.x % n_ablk;
    const int sp = blockIdx.x / n_ablk;
    const int jt0 = sp * tiles_per_split;
    const int jt1 = min(jt0 + tiles_per_split, n_btiles);
    const int h = lane >> 5;
    const int atile = ablk * kPWaves + wave;   // this wave's 32-row tile = its candidate region = its refine workgroup
    const int i_base = atile * 32;

    half8 a[kPK];
#pragma unroll
    for (int ks = 0; ks < kPK; ++ks) a[ks] = PA[((size_t)atile * kPK + ks) * 64 + lane];

    // accumulator register r = source row (r >> 2) * 8 + h * 4 + (r & 3), target column lane & 31
    int lim[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i_base + (r >> 2) * 8 + h * 4 + (r & 3);
        lim[r] = __float_as_int(i < n1 ? 1.0e-30f : 3.0e38f);
    }
    int qn = 0;   // wave-uniform number of candidates appended so far
    // What the other workgroups have published for this wave's 32 rows is fetched global -> LDS asynchronously (issued at
    // one sharing point, consumed at the next; agent-coherent load), so the panel loop never waits for that round trip
    // and the copy costs no registers.
    auto fetch_seen = [&]() __attribute__((always_inline)) {
        if (lane < 32)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ms.rowlim + min(i_base + lane, n1 - 1)),
                                             (__attribute__((address_space(3))) void*)(&seenL[wave][0]), 4, 0, 16 /* sc1 */);
    };
    auto share = [&](bool reload) __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the fetch issued at the previous sharing point (long landed)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint4 sv = *reinterpret_cast<const uint4*>(&seenL[wave][g * 8 + h * 4]);
            const unsigned int seen[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = g * 4 + e;
                const float v = group32_max(__int_as_float(lim[r]));
                const int i = i_base + g * 8 + h * 4 + e;
                if ((lane & 31) == 0 && i < n1 && __float_as_uint(v) > seen[e]) atomicMax(ms.rowlim + i, __float_as_uint(v));
                lim[r] = max(__float_as_int(v), (int)seen[e]);
            }
        }
        if (reload) fetch_seen();
    };
    // candidates of one 32 x 32 tile of scores whose limits are already updated (some lane hit)
    unsigned int* const region = ms.cand + ((size_t)atile * ms.splits + sp) * kPRegionCap;
    auto tile_candidates = [&](const f32x16& cc, const int jt) __attribute__((always_inline)) {
        unsigned long long any = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) any |= __builtin_amdgcn_ballot_w64(cc[r] >= __int_as_float(lim[r]));
        if (__builtin_popcountll(any) > 8) {   // a crowd: pool the limits of the 32 columns first (see the Q-form kernel)
#pragma unroll
            for (int r = 0; r < 16; ++r) lim[r] = __float_as_int(group32_max(__int_as_float(lim[r])));
        }
        const unsigned int j = (unsigned int)(jt * 32 + (lane & 31));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(cc[r] >= __int_as_float(lim[r]));
            if (mask) {
                const int pos = qn + mbcnt(mask);
                if (((mask >> lane) & 1ull) && pos < kPRegionCap)
                    region[pos] = ((unsigned int)((r >> 2) * 8 + h * 4 + (r & 3)) << 27) | j;
                qn += __builtin_popcountll(mask);
            }
        }
    };

    // staging: the panel's 33 fragments of 1 KiB go global -> LDS directly (global_load_lds_dwordx4: 16 B per lane, LDS
    // address = wave-uniform base + 16 * lane) -- no staging registers, no ds_write.  Issued by the four OLDER waves
    // (fragment f by wave f & 3) in the slack they have before each barrier: the matrix pipe serves the older wave of a
    // SIMD first, so it is the younger one that arrives last.
    auto stage = [&](int jt, int buf) __attribute__((always_inline)) {
        const half8* const src = PB + (size_t)jt * kPK * 64 + lane;
#pragma unroll
        for (int q = 0; q < (kPK + kPWaves / 2 - 1) / (kPWaves / 2); ++q) {
            const int f = q * (kPWaves / 2) + wave;
            if (f < kPK)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + f * 64),
                                                 (__attribute__((address_space(3))) void*)(&ldsB[buf][f * 64]), 16, 0, 0);
        }
    };
    // limits and hit tests of one panel's scores, as straight code: the lane's row history in `fl`
    auto limits = [&](const f32x16& cc, unsigned int& fl) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            lim[r] = max(lim[r], __float_as_int(cc[r] - kCoarseMarginP));
            fl = __builtin_amdgcn_alignbit(fl, __float_as_int(cc[r] - __int_as_float(lim[r])), 31);
        }
    };
    // sharing point + candidates of panel jp, whose limits are updated and whose row history is `fl`
    auto bookkeeping = [&](const f32x16& cc, const unsigned int fl, const int jp) __attribute__((always_inline)) {
        const int kt = jp - jt0;
        if ((ms.share_mask >> (kt < 31 ? kt : 31)) & 1u) {
            if (kt < 31 || (kt & 31) == 31) share(true);
        }
        unsigned int hits = ~fl & 0xffffu;   // bit 15 - r set = this lane's row r hit
        unsigned long long mask = __builtin_amdgcn_ballot_w64(hits != 0);
        if (__builtin_popcountll(mask) > 8) {
            tile_candidates(cc, jp);   // a crowd: pool the limits first
        } else {
            // a few lanes, usually one row each: every round appends the highest pending row of each such lane
            const unsigned int j = (unsigned int)(jp * 32 + (lane & 31));
            while (mask) {
                if (hits) {
                    const int k = 31 - __builtin_clz(hits);
                    hits &= ~(1u << k);
                    const int r = 15 - k;
                    const int pos = qn + mbcnt(mask);
                    if (pos < kPRegionCap) region[pos] = ((unsigned int)((r >> 2) * 8 + h * 4 + (r & 3)) << 27) | j;
                }
                qn += __builtin_popcountll(mask);
                mask = __builtin_amdgcn_ballot_w64(hits != 0);
            }
        }
    };
    // The 33 MFMAs of panel jt from LDS buffer `buf` into `acc` (inline asm: the register file of every operand is ours
    // to choose -- A tile and accumulators in AGPRs).  INTERLEAVE: the limit updates and hit tests of panel jt - 1
    // (scores in `prev`) go between the MFMAs, one accumulator register per two k-steps.
    auto mfma_panel = [&](const int buf, f32x16& acc, const f32x16& prev, unsigned int& fl, auto interleave) __attribute__((always_inline)) {
        const half8* const lb = &ldsB[buf][lane];
        half8 b[kPDepth];
#pragma unroll
        for (int q = 0; q < kPDepth; ++q) b[q] = lb[q * 64];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < kPK; ++ks) {
            // refill the ring slot the PREVIOUS MFMA consumed: a whole MFMA lies between an MFMA and the LDS read that
            // overwrites its B operand (the compiler's hazard recogniser does not see inside the asm)
            if (ks >= 1 && ks - 1 + kPDepth < kPK) b[(ks - 1) % kPDepth] = lb[(ks - 1 + kPDepth) * 64];
            __builtin_amdgcn_sched_barrier(0);
            // fragments 0..31 of the A tile fill the 128 AGPRs a wave of this kernel gets; the last one stays in VGPRs
            // (asking for a 33rd AGPR quad makes the compiler copy into it right before the MFMA -- a VALU write ->
            // MFMA read hazard it cannot see through the asm: wrong scores, now and then)
            if (ks == 0) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=v"(acc) : "a"(a[ks]), "v"(b[ks % kPDepth]));
            else if (ks < 32) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(a[ks]), "v"(b[ks % kPDepth]));
            else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a[ks]), "v"(b[ks % kPDepth]));
            if (decltype(interleave)::value && ks < 32 && (ks & 1) == 0) {
                const int r = ks >> 1;
                lim[r] = max(lim[r], __float_as_int(prev[r] - kCoarseMarginP));
                fl = __builtin_amdgcn_alignbit(fl, __float_as_int(prev[r] - __int_as_float(lim[r])), 31);
                asm volatile("" : "+v"(fl), "+v"(lim[r]));   // here, not after the loop
            }
            __builtin_amdgcn_sched_barrier(0);   // keep the reads kPDepth steps ahead and the limit work between the MFMAs
        }
        // the last MFMA's results must not be read for 18 wait states (the compiler does not see inside the asm)
        // (`acc` is an operand so that no compiler-generated read of it can be scheduled between the last MFMA and the nops)
        asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" : "+v"(acc) : : "memory");
    };
    const bool young = wave >= kPWaves / 2;   // wave-uniform
    // One panel.  Older wave of a SIMD: MFMAs with the limit work of the previous panel in between, then that panel's
    // candidates, then -- in the slack before the barrier -- the staging of panel jt + 2.  Younger wave: the previous
    // panel's limits and candidates first (the matrix pipe is busy with the older wave anyway), then a bare MFMA loop.
    auto panel = [&](const int jt, f32x16& acc, f32x16& prev) __attribute__((always_inline)) {
        const int buf = (jt - jt0) % 3;
        unsigned int fl = ~0u;
        if (young) {
            if (jt > jt0) {
                limits(prev, fl);
                bookkeeping(prev, fl, jt - 1);
            }
            mfma_panel(buf, acc, prev, fl, std::false_type{});
        } else {
            mfma_panel(buf, acc, prev, fl, std::true_type{});
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // panel jt + 1 (issued one panel ago) has landed
            if (jt > jt0) bookkeeping(prev, fl, jt - 1);
            if (jt + 2 < jt1) stage(jt + 2, (buf + 2) % 3);    // its buffer was last read in panel jt - 1
        }
        // a bare barrier: __syncthreads() would drain the staging just issued (its fence waits for vmcnt(0)).  LDS reads
        // of this panel are complete (every fragment went through an MFMA), the staged data is covered by the explicit
        // vmcnt(0) above, one barrier before its first read.
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    if (!young) {
        if (jt0 < jt1) stage(jt0, 0);
        if (jt0 + 1 < jt1) stage(jt0 + 1, 1);
    }
    fetch_seen();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x16 accA, accB;
    accA = accB = f32x16{-1.0f};   // below every limit
    int jt = jt0;
    for (; jt + 1 < jt1; jt += 2) {
        panel(jt, accA, accB);
        panel(jt + 1, accB, accA);
    }
    if (jt < jt1) {
        panel(jt, accA, accB);
        accB = accA;
    }
    if (jt0 < jt1) {   // drain: limits and candidates of the last panel (its scores are in accB either way)
        unsigned int fl = ~0u;
        limits(accB, fl);
        bookkeeping(accB, fl, jt1 - 1);
    }
    share(false);   // publish what this split learned
    if (lane == 0) ms.cnt[(size_t)atile * ms.splits + sp] = (unsigned int)qn;
}

// refine: one workgroup per block of kCoarseRows source rows (= one wave of the coarse kernel), one
// thread per candidate.  d2 = 4 - sum_ab (Qi[:,a] . Qj[:,b])^2 in fp64 from hi+lo; per-row arg-min through
// an LDS atomicMin on (bits(float(d2)) << 32 | j): lowest index among candidates whose d2 agree to fp32.
// Rows and candidates are SLOTS of the basis buffers; with a slot order (ms.ord1 / ms.ord2, qlayout.h) j in the key and the row
// that is written are the keypoints behind the slots, so the tie rule and the outputs are those of the identity order.
constexpr int kQiStride = 130;   // doubles per row in LDS: 128 + 2 (rows land on different banks)

template <int kRows, int kCap>   // rows per block = rows per wave of the coarse kernel that filled the regions; region capacity
__global__ __launch_bounds__(256, 4) void match_refine_kernel(const _Float16* __restrict__ Ah,
                                                           const _Float16* __restrict__ Bh, int n1, int n2,
                                                           MatchScratch ms, int64_t* __restrict__ idx,
                                                           float* __restrict__ dist)
{
    constexpr int kCoarseRows = kRows, kRegionCap = kCap;   // shadow the Q-form constants
    __shared__ double qi[kCoarseRows * kQiStride];
    __shared__ unsigned long long best[kCoarseRows];
    __shared__ unsigned int offs[kWave + 1];
    __shared__ int overflow;
    const int blk = blockIdx.x;
    const int i0 = blk * kCoarseRows;
    const int tid = threadIdx.x;
    if (tid < kWave) {   // wave 0: exclusive prefix sum of the region fills (splits <= kMaxSplits = 64)
        const unsigned int c = tid < ms.splits ? ms.cnt[(size_t)blk * ms.splits + tid] : 0u;
        const bool ovf = c > (unsigned int)kRegionCap;
        unsigned int incl = min(c, (unsigned int)kRegionCap);
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned int up = (unsigned int)__shfl_up((int)incl, d, kWave);
            if (tid >= d) incl += up;
        }
        offs[tid + 1] = incl;
        const bool any_ovf = __builtin_amdgcn_ballot_w64(ovf) != 0ull;   // all 64 lanes vote (NOT inside the tid == 0 branch)
        if (tid == 0) {
            offs[0] = 0;
            overflow = any_ovf || ms.force_exhaustive;
        }
    }
    if (tid < kCoarseRows) best[tid] = ~0ull;
    // stationary rows: 16 (a, k8) groups of 8 channels per row
    for (int e = tid; e < kCoarseRows * 16; e += blockDim.x) {
        const int r = e >> 4, a = (e >> 2) & 3, k8 = e & 3;
        const int i = min(i0 + r, n1 - 1);
        const half8 vh = *reinterpret_cast<const half8*>(Ah + hoff_rows(i, a, k8 * 8, 0));
        const half8 vl = *reinterpret_cast<const half8*>(Ah + hoff_rows(i, a, k8 * 8, 1));
#pragma unroll
        for (int x = 0; x < 8; ++x) qi[r * kQiStride + (k8 * 8 + x) * 4 + a] = (double)vh[x] + (double)vl[x];
    }
    __syncthreads();
    const bool exhaustive = overflow != 0;
    const unsigned int total = exhaustive ? (unsigned int)kCoarseRows * (unsigned int)n2 : offs[ms.splits];
    const unsigned int* const regions = ms.cand + (size_t)blk * ms.splits * kRegionCap;
    int sp = 0;
    for (unsigned int e = tid; e < total; e += blockDim.x) {
        unsigned int r, j;
        if (exhaustive) {
            r = e % kCoarseRows;
            j = e / kCoarseRows;
        } else {
            while (e >= offs[sp + 1]) ++sp;   // e grows monotonically per thread
            const unsigned int ent = regions[(size_t)sp * kRegionCap + (e - offs[sp])];
            r = ent >> 27;
            j = ent & 0x07ffffffu;
        }
        const double* const q = qi + r * kQiStride;
        double dot[4][4];   // [a][b]
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) dot[a][b] = 0.0;
#pragma unroll 2
        for (int k8 = 0; k8 < 4; ++k8) {
            half8 vh[4], vl[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                vh[b] = *reinterpret_cast<const half8*>(Bh + hoff_cols((int)j, b, k8 * 8, 0));
                vl[b] = *reinterpret_cast<const half8*>(Bh + hoff_cols((int)j, b, k8 * 8, 1));
            }
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int k = k8 * 8 + x;
                const double q0 = q[k * 4 + 0], q1 = q[k * 4 + 1], q2 = q[k * 4 + 2], q3 = q[k * 4 + 3];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double v = (double)((float)vh[b][x] + (float)vl[b][x]);   // fp32 sum: error <= 2^-24 |q|
                    dot[0][b] = fma(q0, v, dot[0][b]);
                    dot[1][b] = fma(q1, v, dot[1][b]);
                    dot[2][b] = fma(q2, v, dot[2][b]);
                    dot[3][b] = fma(q3, v, dot[3][b]);
                }
            }
        }
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) s = fma(dot[a][b], dot[a][b], s);
        const float d2 = (float)fmax(4.0 - s, 0.0);
        if (d2 == d2 && (int)(i0 + r) < n1) {   // NaN scores never win
            const unsigned int jk = ms.ord2 ? (unsigned int)ms.ord2[target_slot_pos((int)j, n2)] : j;
            atomicMin(&best[r], ((unsigned long long)__float_as_uint(d2) << 32) | jk);
        }
    }
    __syncthreads();
    if (tid < kCoarseRows && i0 + tid < n1) {
        const unsigned long long k = best[tid];
        const bool ok = k != ~0ull;   // all-NaN rows: report target 0 at the maximum distance
        const int ik = ms.ord1 ? ms.ord1[i0 + tid] : i0 + tid;
        idx[ik] = ok ? (int64_t)(unsigned int)(k & 0xffffffffull) : 0;
        if (dist) dist[ik] = ok ? sqrtf(__uint_as_float((unsigned int)(k >> 32))) : 2.0f;
    }
}

}  // namespace umereg

using namespace umereg;

UMEREG_API int umereg_ume_match_coarse_f16_ex(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, void* scratch,
                                              size_t scratch_bytes, const umereg_match_opts* opts, void* stream)
{
    MatchOpts o;
    if (int rc = resolve_opts(opts, o, "ume_match_coarse_f16")) return rc;
    if (int rc = match_args(Q1_rows_h, Q2_cols_h, n1, n2, scratch, scratch_bytes, o, "ume_match_coarse_f16")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const CoarsePlan p = coarse_plan(n1, n2, o);
    const MatchScratch ms = carve_scratch(scratch, n1, p, o);
    if (use_pform(o)) {
        half8* const PA = pfrag_rows(scratch, n1, p, o);
        half8* const PB = pfrag_cols(scratch, n1, p, o);
        const int tiles = p.n_blocks > p.n_btiles ? p.n_blocks : p.n_btiles;
        hipLaunchKernelGGL(pform_pack_kernel, dim3(tiles, 2), dim3(256), 0, st, (const _Float16*)Q1_rows_h, (const _Float16*)Q2_cols_h,
                           n1, n2, p.n_blocks, p.n_btiles, PA, PB);
        UMEREG_CHECK_LAUNCH("pform_pack_kernel");
        hipLaunchKernelGGL(ume_coarse_p_kernel, dim3(p.n_ablk * p.splits), dim3(kWave * kPWaves), 0, st, PA, PB, n1, n2, p.n_ablk,
                           p.n_btiles, p.tiles_per_split, ms);
        UMEREG_CHECK_LAUNCH("ume_coarse_p_kernel");
        return UMEREG_OK;
    }
    const dim3 wg(kWave * kDistWaves);
    if (p.sub_tiles && UMEREG_COARSE_PHASES == 2) {
        hipLaunchKernelGGL(ume_coarse_h_kernel, dim3(p.n_ablk * p.sub_splits), wg, 0, st, (const half8*)Q1_rows_h, (const half8*)Q2_cols_h,
                           n1, n2, p.n_ablk, 0, p.sub_tiles, p.sub_tiles, p.sub_tps, p.sub_splits, 1, 0, ms);
        UMEREG_CHECK_LAUNCH("ume_coarse_h_kernel");
        hipLaunchKernelGGL(ume_coarse_h_kernel, dim3(p.n_ablk * (p.splits - p.sub_splits)), wg, 0, st, (const half8*)Q1_rows_h,
                           (const half8*)Q2_cols_h, n1, n2, p.n_ablk, p.sub_tiles, p.sub_tiles, p.n_btiles, 1, 0, p.tiles_per_split,
                           p.sub_splits, ms);
    } else {
        hipLaunchKernelGGL(ume_coarse_h_kernel, dim3(p.n_ablk * p.splits), wg, 0, st, (const half8*)Q1_rows_h, (const half8*)Q2_cols_h,
                           n1, n2, p.n_ablk, 0, p.sub_tiles, p.n_btiles, p.sub_tiles ? p.sub_tps : 1, p.sub_splits, p.tiles_per_split, 0, ms);
    }
    UMEREG_CHECK_LAUNCH("ume_coarse_h_kernel");
    return UMEREG_OK;
}
UMEREG_API int umereg_ume_match_coarse_f16(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, void* scratch,
                                           size_t scratch_bytes, void* stream)
{
    return umereg_ume_match_coarse_f16_ex(Q1_rows_h, Q2_cols_h, n1, n2, scratch, scratch_bytes, nullptr, stream);
}

int umereg::match_refine_f16(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, const void* scratch, size_t scratch_bytes,
                             int64_t* match_idx, float* match_dist, const umereg_match_opts* opts, const int* order1,
                             const int* order2, void* stream)
{
    UMEREG_REQUIRE(match_idx, "ume_match_refine_f16: null match_idx");
    MatchOpts o;
    if (int rc = resolve_opts(opts, o, "ume_match_refine_f16")) return rc;
    if (int rc = match_args(Q1_rows_h, Q2_cols_h, n1, n2, (void*)scratch, scratch_bytes, o, "ume_match_refine_f16")) return rc;
    const CoarsePlan p = coarse_plan(n1, n2, o);
    const MatchScratch ms = carve_scratch((void*)scratch, n1, p, o, order1, order2);
    if (use_pform(o))
        hipLaunchKernelGGL((match_refine_kernel<kPRows, kPRegionCap>), dim3(p.n_blocks), dim3(256), 0, (hipStream_t)stream,
                           (const _Float16*)Q1_rows_h, (const _Float16*)Q2_cols_h, n1, n2, ms, match_idx, match_dist);
    else
        hipLaunchKernelGGL((match_refine_kernel<kCoarseRows, kRegionCap>), dim3(p.n_blocks), dim3(256), 0, (hipStream_t)stream,
                           (const _Float16*)Q1_rows_h, (const _Float16*)Q2_cols_h, n1, n2, ms, match_idx, match_dist);
    UMEREG_CHECK_LAUNCH("match_refine_kernel");
    return UMEREG_OK;
}
UMEREG_API int umereg_ume_match_refine_f16_ex(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2,
                                              const void* scratch, size_t scratch_bytes, int64_t* match_idx,
                                              float* match_dist, const umereg_match_opts* opts, void* stream)
{
    return match_refine_f16(Q1_rows_h, Q2_cols_h, n1, n2, scratch, scratch_bytes, match_idx, match_dist, opts, nullptr, nullptr, stream);
}
UMEREG_API int umereg_ume_match_refine_f16(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2,
                                           const void* scratch, size_t scratch_bytes, int64_t* match_idx,
                                           float* match_dist, void* stream)
{
    return umereg_ume_match_refine_f16_ex(Q1_rows_h, Q2_cols_h, n1, n2, scratch, scratch_bytes, match_idx, match_dist, nullptr, stream);
}
