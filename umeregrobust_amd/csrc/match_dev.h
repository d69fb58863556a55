// match_dev.h -- what the units of the a3/a4 matcher share (ume_dist.hip, match_f16r.hip, match.hip, pair_match.hip):
// the MFMA vector types, the geometry of the candidate regions, the scratch record the coarse and the
// refine kernels both take, and the host-side plan (options, splits, scratch carve-up).  Kernels are NOT declared here: a
// kernel is launched only from the unit that defines it, and units call each other through the public umereg_* entries --
// or, where a call carries what the C ABI does not (the slot order of the pair chain), through the host functions at the end.
// Not part of the C ABI.
#pragma once
#include "common.h"
#include "qlayout.h"

namespace umereg {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using half8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x2 = __attribute__((ext_vector_type(2))) float;

constexpr int kDistWaves = 4;

// ---- filter + refine matcher (precision "f16r"; the proof that the filter keeps the exact winner: match_f16r.hip) ----
constexpr int kRegionCap = 512;    // candidates per (block of rows, split)
constexpr int kMaxSplits = 64;
constexpr unsigned int kShareMask = 0x8000808bu;   // after tiles 1, 2, 4, 8, 16 of a split, then every 32nd

struct MatchScratch {
    unsigned int* rowlim;   // [n1] bits of the best (coarse score - margin) published so far, >= 0
    unsigned int* cnt;      // [n_blocks][splits] candidates appended to the region (> kRegionCap: overflowed)
    unsigned int* cand;     // [n_blocks][splits][kRegionCap]  (local row << 27) | target
    int splits;
    unsigned int share_mask;   // bit k: share the limits after tile k of a split (k >= 31: every 32nd tile)
    int force_exhaustive;      // testing probe: UMEREG_FORCE_EXHAUSTIVE
    // slot order (qlayout.h; null = identity): the bases were written with source slot s = keypoint ord1[s] and target slot s =
    // keypoint ord2[target_slot_pos(s, n2)].  The coarse kernel works on slots; the refine kernel maps back to keypoints.
    const int* ord1;
    const int* ord2;
    unsigned long long* stats; // UMEREG_COARSE_STATS builds only (else null): tiles, tiles stopped at test 1 / 2, candidates
};

// Q-form coarse kernel (ume_coarse_h_kernel)
constexpr int kCoarseTA = 2;   // A tiles (8 source keypoints each) per wave (4 -- half the LDS reads per MFMA, 238 VGPRs -- measured 174 us against 142)
constexpr int kCoarseRows = kCoarseTA * 8;           // source keypoints per wave
constexpr int kCoarseWG = kCoarseRows * kDistWaves;  // source keypoints per workgroup (<= ROWS_F16X2 padding)

// P-form coarse kernel (ume_coarse_p_kernel)
constexpr int kPK = 33;                      // MFMA k-steps per pair of keypoints (528 / 16)
constexpr int kPWaves = 8;                   // waves per workgroup: two per SIMD
constexpr int kPRows = 32;                   // source keypoints per wave = per A tile = per candidate region = per refine workgroup
constexpr int kPWG = kPRows * kPWaves;       // source keypoints per workgroup
constexpr int kPRegionCap = 1024;            // candidates per (32 rows, split)

// ---- host side: sizes, options, plan, scratch carve-up ----
inline size_t qa_bytes(int n1) { return align_up((size_t)n1, 128) * 128 * sizeof(float); }   // covers ROWS and ROWS_F16X2
inline size_t qb_bytes(int n2) { return align_up((size_t)n2, 32) * 128 * sizeof(float); }
// splits [0, sub_splits) cover the target tiles [0, sub_tiles) in runs of sub_tps (the LEADING splits of the Q-form: the tiles of
// the subsample that leads the slot order, qlayout.h), the other splits cover [sub_tiles, n_btiles) in runs of tiles_per_split.
// sub_tiles = 0: uniform splits over everything.
struct CoarsePlan {
    int n_ablk, n_blocks, n_btiles, splits, tiles_per_split;
    int sub_tiles, sub_tps, sub_splits;
};
// Per-call options of the filter + refine matcher (umereg_match_opts in umereg.h; NULL = the defaults).  There is no
// process-wide matcher state: a call's plan (splits, region capacity, scratch layout) is a function of its arguments only.
struct MatchOpts {
    int variant = 0;            // 0 = Q-form coarse kernel, 1 = P-form (one inner product per pair, no squares; DESIGN.md 3.3:
                                // 11 % faster as a stage on MI355X, 4 % slower in the pipelined path -- kept as a variant)
    int splits = 0;             // target splits of the coarse pass (0 = automatic)
    long long share_mask = -1;  // limit-sharing schedule (< 0 = kShareMask)
    int exhaustive = 0;         // refine every block of rows exhaustively (parity test)
};
inline int resolve_opts(const umereg_match_opts* o, MatchOpts& m, const char* who)
{
    m = MatchOpts();
    if (!o) return UMEREG_OK;
    UMEREG_REQUIRE(o->variant == 0 || o->variant == 1, "%s: unknown matcher variant %d (0 = Q-form, 1 = P-form)", who, (int)o->variant);
    UMEREG_REQUIRE(o->splits >= 0 && o->force_exhaustive >= 0, "%s: negative matcher option", who);
    UMEREG_REQUIRE(o->share_mask <= 0xffffffffll, "%s: share_mask does not fit 32 bits", who);
    UMEREG_REQUIRE(o->reserved == 0, "%s: umereg_match_opts.reserved must be 0 (got %d)", who, (int)o->reserved);
    m.variant = o->variant;
    m.splits = o->splits;
    m.share_mask = o->share_mask;
    m.exhaustive = o->force_exhaustive ? 1 : 0;
    return UMEREG_OK;
}
inline bool use_pform(const MatchOpts& o) { return o.variant == 1; }
constexpr int kNumCU = 256;   // MI355X
#ifndef UMEREG_COARSE_PHASES
#define UMEREG_COARSE_PHASES 3   // A/B (profiles/r07/coarse_skip.txt): 1 = uniform splits, 2 = the leading splits as a launch of their own
#endif
constexpr int kMinSplitTiles = 4;   // a split of fewer tiles is all prologue: rows loaded, limits fetched and published, nothing skipped yet
constexpr int kLeadMinTiles = 64;   // below 2 048 targets the plan stays uniform (few workgroups: nothing to order)

inline CoarsePlan coarse_plan(int n1, int n2, const MatchOpts& o)
{
    CoarsePlan p;
    p.n_btiles = (n2 + 31) / 32;
    int splits;
    if (use_pform(o)) {
        p.n_ablk = (n1 + kPWG - 1) / kPWG;
        p.n_blocks = p.n_ablk * kPWaves;
        splits = kNumCU / p.n_ablk;   // one workgroup per CU, one round
    } else {
        p.n_ablk = (n1 + kCoarseWG - 1) / kCoarseWG;
        p.n_blocks = p.n_ablk * kDistWaves;
        splits = (2560 + p.n_ablk - 1) / p.n_ablk;   // ~10 workgroups per CU
    }
    p.sub_tiles = p.sub_tps = p.sub_splits = 0;
    if (UMEREG_COARSE_PHASES >= 2 && !use_pform(o) && o.splits <= 0 && p.n_btiles >= kLeadMinTiles) {
        // The tiles of the leading subsample go first (block index is split-major), in splits sized so that their workgroups fill
        // ONE round of the chip: they publish every row's limit when they retire, and the bulk's workgroups, which take their
        // places, start from those limits -- the early exit then bites from their first tile on.  With uniform splits the
        // workgroups of the first bulk splits are resident beside the subsample's and run a quarter of the bulk with limits near
        // zero; as a launch of its own the lead costs its drain (measured, all three: profiles/r07/coarse_skip.txt).
        const int n_sub = (n2 + kSubStride - 1) / kSubStride;
        p.sub_tiles = (n_sub + 31) / 32;
        int s1 = 4 * kNumCU / p.n_ablk;   // four workgroups are resident per CU
        s1 = s1 < 1 ? 1 : (s1 > 16 ? 16 : s1);
        s1 = s1 > p.sub_tiles / kMinSplitTiles ? p.sub_tiles / kMinSplitTiles : s1;   // (sub_tiles >= 8 here)
        p.sub_tps = (p.sub_tiles + s1 - 1) / s1;
        p.sub_splits = (p.sub_tiles + p.sub_tps - 1) / p.sub_tps;
        const int bulk = p.n_btiles - p.sub_tiles;
        int s2 = splits > kMaxSplits - 16 ? kMaxSplits - 16 : splits;
        s2 = s2 > bulk / kMinSplitTiles ? bulk / kMinSplitTiles : s2;
        p.tiles_per_split = (bulk + s2 - 1) / s2;
        p.splits = p.sub_splits + (bulk + p.tiles_per_split - 1) / p.tiles_per_split;
        return p;
    }
    if (o.splits > 0) splits = o.splits;   // umereg_match_opts.splits
    if (splits > kMaxSplits) splits = kMaxSplits;
    if (splits > p.n_btiles) splits = p.n_btiles;
    if (splits < 1) splits = 1;
    p.tiles_per_split = (p.n_btiles + splits - 1) / splits;
    p.splits = (p.n_btiles + p.tiles_per_split - 1) / p.tiles_per_split;
    return p;
}
inline size_t region_cap(const MatchOpts& o) { return use_pform(o) ? (size_t)kPRegionCap : (size_t)kRegionCap; }
inline size_t cand_bytes(int n1, const CoarsePlan& p, const MatchOpts& o)
{
    return align_up(((size_t)n1 + (size_t)p.n_blocks * p.splits * (1 + region_cap(o))) * sizeof(unsigned int), 256);
}
// packed projector fragments of both sets (P-form only): [n_blocks][34][64] + [n_btiles][34][64] half8
inline size_t pfrag_bytes(const CoarsePlan& p, const MatchOpts& o)
{
    return use_pform(o) ? ((size_t)p.n_blocks + (size_t)p.n_btiles) * kPK * 64 * sizeof(half8) : 0;
}
#ifndef UMEREG_COARSE_STATS
#define UMEREG_COARSE_STATS 0   // 1: the Q-form coarse kernel counts its tiles and candidates (tools/exp_coarse_skip.py); never in the product
#endif
constexpr size_t kStatsBytes = UMEREG_COARSE_STATS ? 256 : 0;   // four 64-bit counters at the very end of the scratch
inline size_t match_scratch_bytes(int n1, int n2, const MatchOpts& o = MatchOpts())
{
    const CoarsePlan p = coarse_plan(n1, n2, o);
    return cand_bytes(n1, p, o) + pfrag_bytes(p, o) + kStatsBytes;
}

inline int match_args(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, void* scratch, size_t scratch_bytes,
                      const MatchOpts& o, const char* who)
{
    UMEREG_REQUIRE(Q1_rows_h && Q2_cols_h, "%s: null basis pointer", who);
    UMEREG_REQUIRE(n1 > 0 && n2 > 0, "%s: n1, n2 must be positive (got %d, %d)", who, n1, n2);
    UMEREG_REQUIRE(n2 < (1 << 27), "%s: n2 must be below 2^27 (got %d)", who, n2);
    UMEREG_REQUIRE(((uintptr_t)Q1_rows_h & 15) == 0 && ((uintptr_t)Q2_cols_h & 15) == 0, "%s: misaligned basis pointer", who);
    if (int rc = check_device()) return rc;
    if (!scratch || scratch_bytes < match_scratch_bytes(n1, n2, o) || ((uintptr_t)scratch & 15)) {
        set_error("%s: scratch too small or misaligned (%zu < %zu)", who, scratch_bytes, match_scratch_bytes(n1, n2, o));
        return UMEREG_EWORKSPACE;
    }
    return UMEREG_OK;
}

inline MatchScratch carve_scratch(void* scratch, int n1, const CoarsePlan& p, const MatchOpts& o, const int* ord1 = nullptr,
                                  const int* ord2 = nullptr)
{
    MatchScratch ms;
    ms.rowlim = (unsigned int*)scratch;
    ms.cnt = ms.rowlim + n1;
    ms.cand = ms.cnt + (size_t)p.n_blocks * p.splits;
    ms.splits = p.splits;
    ms.share_mask = o.share_mask >= 0 ? (unsigned int)o.share_mask : kShareMask;
    ms.force_exhaustive = o.exhaustive;
    ms.ord1 = ord1;
    ms.ord2 = ord2;
    ms.stats = UMEREG_COARSE_STATS ? (unsigned long long*)((char*)scratch + cand_bytes(n1, p, o) + pfrag_bytes(p, o)) : nullptr;
    return ms;
}
inline half8* pfrag_rows(void* scratch, int n1, const CoarsePlan& p, const MatchOpts& o) { return (half8*)((char*)scratch + cand_bytes(n1, p, o)); }
inline half8* pfrag_cols(void* scratch, int n1, const CoarsePlan& p, const MatchOpts& o) { return pfrag_rows(scratch, n1, p, o) + (size_t)p.n_blocks * kPK * 64; }

// ---- the matcher with a slot order (not exported) ----
// ortho.hip: bases of both sets in one launch; order1 / order2 as in MatchScratch (null = identity)
int launch_orthobasis_pair(const float* ume1, int n1, int layout1, float* Q1, const float* ume2, int n2, int layout2, float* Q2,
                           hipStream_t st, const int* order1 = nullptr, const int* order2 = nullptr);
// match_f16r.hip: umereg_ume_match_refine_f16_ex for bases written in slot order; match_idx / match_dist are keyed on keypoints
int match_refine_f16(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, const void* scratch, size_t scratch_bytes,
                     int64_t* match_idx, float* match_dist, const umereg_match_opts* opts, const int* order1, const int* order2,
                     void* stream);
// match.hip: umereg_ume_match_f16r_ex (B = 1) with both sets matched in the given orders; the results are those of the plain call
int match_f16r_ordered(const float* ume1, const float* ume2, int n1, int n2, const int* order1, const int* order2,
                       int64_t* match_idx, float* match_dist, void* workspace, size_t workspace_bytes,
                       const umereg_match_opts* opts, void* stream);

}  // namespace umereg
