// corr.hip -- SURVEY 8(f1): hypothesis selection by feature correlation, for gfx950.
// Replaces pytorch3d.ops.knn_points as used at reference utils/loc_utils.py:580,623 and
// evaluate.py:272,274, feature_spatial_var (utils/loc_utils.py:579-585) and the per-hypothesis
// score of pc_corr / pc_corr_cost_pytorch3d (utils/loc_utils.py:592-637) that
// FeatureCorrelator.feature_corr_hypothesis_test (utils/loc_utils.py:656-681) maximises.
//
// The reference runs a brute-force kNN (every query against every target point) for each of the
// M = 2 500 hypotheses: 2.5e11 distance tests and a [64,10000,20,32] gathered tensor (1.6 GB) per
// batch of 64 hypotheses.  Here:
//
//   * exact kNN on the uniform grid of grid.h (kNN mode: cell edge from the point density, thin axes
//     collapsed);
//   * one LANE per query, one wavefront per 64 spatially adjacent queries (queries are processed in
//     cell-sorted order, and a rigid transform keeps neighbours adjacent, so adjacent lanes touch the
//     same cache lines); each lane walks only the cell rows that intersect ITS search ball, clipped to
//     the ball's chord (walk_ball).  The first radius comes from the local point density and grows
//     while the lane is starved, until the ball provably holds the K nearest;
//   * "K smallest by (d2, index)" without per-candidate sorted insertion: pass 1 histograms d2 per
//     lane (32 bins, LDS, lane-private counters) to find the bin that holds the K-th neighbour,
//     zooming x32 into that bin when too many candidates share it; pass 2 walks the (smaller) ball of
//     that bin and appends only candidates up to it (K + a few) to a lane-private LDS list, then
//     trims the extras by repeated arg-max.  Overflowing lists are trimmed on the fly and the
//     admission key tightened, so any density is handled exactly;
//   * the score  sum_k cauchy(d_k) <vp_n, vq_jk> / Ns  is accumulated straight from the K kept
//     (d2, index) keys; the gathered [.,.,20,32] tensor never exists.  Per-(hypothesis, 64-query
//     chunk) partial sums are written and reduced in a fixed order => deterministic scores.
// Squared distances use the reference's arithmetic: sum_d (p1-p2)^2 left to right in fp32, no FMA
// contraction (-ffp-contract=off), ties resolved towards the lower index.
//
// Files (one translation unit each; corr_dev.h = shared inline device code, corr_kernels.h = kernel declarations):
//   corr.hip            this file, host only: routing thresholds, the workspace layout (corr_ws: the one place that knows it), the stage functions and
//                       umereg_corr_scores_ex_f32, the ONE call that enqueues them, its stage profile, umereg_corr_select_best_f32
//   corr_knn.hip        knn_points / feature_spatial_var / weighted features + their entry points
//   corr_consensus.hip  orders + the consensus pass
//   corr_lattice.hip    candidate lattice, cell pass, second pass of the arg-max mode
//   corr_leftover.hip   per-lane grid walk, one wavefront per query (queue / flat / records), outside bound, reductions, pick
#include <assert.h>

#include "corr_kernels.h"

namespace umereg {
#ifndef UMEREG_LAT_MAXCELLS
#define UMEREG_LAT_MAXCELLS (1u << 19)   // (2^20 until round 4: see lattice_budget)
#endif
constexpr unsigned int kLatMinCells = 4096, kLatMaxCells = UMEREG_LAT_MAXCELLS;

// cells for a job of M x Ns queries: the build costs ~5 grid walks per cell, a query saves ~2 of them
__host__ inline unsigned int lattice_cells_for(long queries, int Nt, int flags)
{
    if (Nt > 65535 - 64 || (flags & UMEREG_CORR_NO_LATTICE)) return 0;          // 16-bit list entries
    if (queries < (1l << 17) && !(flags & UMEREG_CORR_FORCE_LATTICE)) return 0;   // tiny jobs keep the grid walk
    long c = queries / 16;
    c = c < (long)kLatMinCells ? kLatMinCells : (c > (long)kLatMaxCells ? kLatMaxCells : c);
    return (unsigned int)c;
}

// (consensus pass, second form: corr_consensus.hip; the far-point margin below is the caller's default)
constexpr float kConsFarMarginCells = 2.5f;   // default margin of the far-point stage (see corr_consensus2_kernel), in grid cells
#ifndef UMEREG_LEFT_MAX_BOUND
#define UMEREG_LEFT_MAX_BOUND 1000000u
#endif
constexpr unsigned int kLeftMaxBound = UMEREG_LEFT_MAX_BOUND;      // kLeftMax (corr_dev.h) where the cell pass rides in arg-max mode on a job below 2^25 queries

// ascending list of the marked cells (deterministic order): cids[0 .. header[3])
// (kCompactBlocks workgroups, each with a contiguous range of 16-cell groups; a workgroup counts the marks of the ranges before its own
// itself -- 512 KiB of marks, read from L2 -- instead of waiting for a scan: one launch, 0.15 -> 0.02 ms for 2^19 cells)
constexpr int kCompactBlocks = 64;
constexpr size_t kCellMaxEntries = (size_t)1 << 26; // queries the pass can list (512 MiB of entries)
constexpr long kCellMinQueries = 1l << 25;          // jobs below this enqueue the pass in arg-max mode only, from 2^24 queries on (corr_ws: cell_pass; a KITTI-test pair: 2.5e7 queries)
__host__ __device__ inline size_t cell_cap(long queries) { return (size_t)(queries < (long)kCellMaxEntries ? queries : (long)kCellMaxEntries); }
__host__ __device__ inline size_t cell_items(unsigned int c_max, long queries) { return (size_t)c_max + cell_cap(queries) / (kCellChunk < kCellChunkLong ? kCellChunk : kCellChunkLong) + 64; }
__host__ inline size_t cell_bytes(unsigned int c_max, long queries)
{
    return 2 * align_up(((size_t)c_max + 64) * 4, 256) + 2 * align_up(cell_items(c_max, queries) * 8, 256) + align_up((1024 + 64) * 4, 256) +
           align_up((size_t)c_max * 32, 256) + align_up(cell_cap(queries) * 8, 256);
}
__host__ inline CellWs cell_ws(char* base, unsigned int c_max, long queries)
{
    CellWs w;
    size_t o = 0;
    w.cnt = reinterpret_cast<unsigned int*>(base + o);  o += align_up(((size_t)c_max + 64) * 4, 256);
    w.cur = reinterpret_cast<unsigned int*>(base + o);  o += align_up(((size_t)c_max + 64) * 4, 256);
    w.bsum = reinterpret_cast<unsigned int*>(base + o); o += align_up((1024 + 64) * 4, 256);
    w.rec = reinterpret_cast<uint4*>(base + o);         o += align_up((size_t)c_max * 32, 256);
    w.items_s = reinterpret_cast<uint2*>(base + o);     o += align_up(cell_items(c_max, queries) * 8, 256);
    w.items_l = reinterpret_cast<uint2*>(base + o);     o += align_up(cell_items(c_max, queries) * 8, 256);
    w.ent = reinterpret_cast<uint2*>(base + o);
    w.cap = (unsigned int)cell_cap(queries);
    return w;
}
__host__ __device__ inline size_t cell_lds_per_wave(int K, bool lng)
{
    // tie list (16-bit index plane) | stage (256 or 512 slots x 16 B) | the lane's K keys (d2 plane -- the histogram lives there until
    // the second sweep starts --, 16-bit index plane)
    // (14.5 KiB: eleven wavefronts per CU; 128 bytes more are ten)
    return (size_t)kCons2Tie * kWave * 6 + (size_t)(lng ? 512 : kCellStage) * 16 + cell_d2_plane(K, lng) + ((size_t)K * kWave * 2 + 255) / 256 * 256;
}

// (the flat list of leftover queries: corr_leftover.hip)
constexpr unsigned int kFlatMaxQ = 1u << 21;
constexpr int kFlatBlocks = 6144;   // workgroups of corr_score_flat_kernel (8 wavefronts each, visits of 4 queries dealt round-robin; 768 .. 16 384 measured: 1.17 .. 1.10 ms)
// (capacity: 2^21 queries, or half of the job's if that is more -- a nuScenes-size job of 1.5e8 queries with outlier hypotheses
// leaves tens of millions of far-off queries, and the record kernel costs 2.4x the flat one per query)
__host__ __device__ inline size_t flat_slots(long n_queries)
{
    const long cap = n_queries / 2 > (long)kFlatMaxQ ? n_queries / 2 : (long)kFlatMaxQ;
    return (size_t)(n_queries < cap ? n_queries : cap);
}
__host__ __device__ inline size_t flat_bytes(size_t n_records, long n_queries)
{
    return align_up(n_records * 4, 256) + 3 * align_up(flat_slots(n_queries) * 4, 256) + align_up(flat_slots(n_queries), 256);
}
__host__ __device__ inline FlatWs flat_ws(char* base, size_t n_records, long n_queries)
{
    FlatWs f;
    f.rbase = reinterpret_cast<unsigned int*>(base);
    f.qlist = reinterpret_cast<unsigned int*>(base + align_up(n_records * 4, 256));
    f.qval = reinterpret_cast<float*>(base + align_up(n_records * 4, 256) + align_up(flat_slots(n_queries) * 4, 256));
    f.qsel = reinterpret_cast<unsigned int*>(base + align_up(n_records * 4, 256) + 2 * align_up(flat_slots(n_queries) * 4, 256));
    f.qfar = reinterpret_cast<unsigned char*>(base + align_up(n_records * 4, 256) + 3 * align_up(flat_slots(n_queries) * 4, 256));
    f.slots = (unsigned int)flat_slots(n_queries);
    return f;
}

// ---- the workspace of one corr_scores call: routing and layout, decided in ONE place (corr_ws) -------------------------------
// Byte offsets of the regions in workspace order (sizes: the `take` lines of corr_ws; table: DESIGN 4.11).  A region that is switched off
// has no bytes.  The host takes every pointer from here (CorrCtx).  Three things outside this function rely on an ADJACENCY:
//   1. device code finds the queue records at lat + lat_ws(c_max).total (the lattice block's inside is lat_ws's): `queue` is that offset;
//   2. Python and the tools read the 64 header words at `lat` as umereg_corr_workspace_bytes_ex(Ns, Nt, M, UMEREG_CORR_NO_LATTICE):
//      everything in front of `lat` exists for every flag set, everything behind it needs the lattice;
//   3. the cell block (cell_ws: its counters first) follows the bound block at once: ONE fill clears the block and the counters.
// corr_ws asserts all three.
struct CorrWs {
    unsigned int c_max;                                                         // lattice cells (0: none, the per-lane grid walk does everything)
    bool consensus, cell_pass, bound;                                           // WITHOUT T: a misaligned T skips both passes at launch, their regions stay
    size_t n_chunks, n_records;                                                 // 64-query chunks of the source; records the queue can hold
    size_t src, tgt, tgth, partial, colsum, rotated, rbar;                      // always
    size_t lat, queue;                                                          // c_max != 0
    size_t val, served, tmed, slices, gorder, perm, inv, chunk_of, centroid;    // consensus
    size_t b_slack, b_surv, b_vpn, b_vqmax, b_farq, bound_head, bound_bytes;    // bound (bytes in front of b_farq; of the whole block)
    size_t cell, flat, total;                                                   // cell_pass; c_max != 0
};

__host__ inline CorrWs corr_ws(int Ns, int Nt, int M, int flags)
{
    CorrWs w = {};
    const long queries = (long)M * Ns;
    const size_t n_words = (size_t)((M + 63) / 64), sNs = (size_t)Ns;
    w.n_chunks = (size_t)((Ns + kWave - 1) / kWave);
    // one record per (hypothesis, chunk) + the slots the list kernel's wavefronts reserve 16 at a time and may not use (<= 4 096 workgroups x 4 wavefronts x 15)
    w.n_records = (size_t)M * w.n_chunks + (size_t)16 * 16384;
    w.c_max = lattice_cells_for(queries, Nt, flags);
    // the consensus pass rides on the lattice (it leaves the queries it cannot prove exact to it)
    w.consensus = w.c_max != 0 && !(flags & UMEREG_CORR_NO_CONSENSUS) && (M >= 256 || (flags & UMEREG_CORR_FORCE_CONSENSUS));
    // the cell pass (corr_cell_kernel) rides on the consensus pass's result planes and on the lattice (32-bit entries); big jobs only, unless forced
    // (round 4: in arg-max mode also from 2^24 queries on -- a KITTI-test pair --: with the far cells bounded, what is left of a half-overlapping pair's
    // 2 M leftovers goes through the lattice + cell pass in 1.9 ms against 2.5 through the queue; leftover_decide_kernel routes them there from kLeftMaxBound on)
    w.cell_pass = w.consensus && !(flags & (UMEREG_CORR_NO_CELL_PASS | UMEREG_CORR_CONSENSUS_V1 | UMEREG_CORR_LEFT_COOP)) &&
                  (unsigned long long)Ns * (unsigned long long)M < (1ull << 32) &&
                  (queries >= kCellMinQueries || (flags & UMEREG_CORR_CELL_PASS) || ((flags & UMEREG_CORR_BOUND_OUTSIDE) && queries >= (1l << 24)));
    // bounding of the queries outside the lattice (corr_score_flat_kernel<1>) and in far cells
    w.bound = w.c_max != 0 && (flags & UMEREG_CORR_BOUND_OUTSIDE) && !(flags & UMEREG_CORR_NO_FLAT);
    size_t o = 0;
    auto take = [&o](bool on, size_t bytes) { const size_t at = o; o += on ? bytes : 0; return at; };
    const bool lt = w.c_max != 0, c = w.consensus, b = w.bound;
    w.src = take(true, grid_ws(Ns).total);
    w.tgt = take(true, grid_ws(Nt).total);
    w.tgth = take(true, grid_ws(Nt).total);                                         // the target once more, in Hilbert-curve order (structures_and_orders)
    w.partial = take(true, align_up((size_t)M * w.n_chunks * 4, 256));              // [M x n_chunks] f32 partial sums
    w.colsum = take(true, align_up((size_t)kColsumBlocks * 32 * 8, 256));           // (kept for the layout: nothing of this call touches it)
    w.rotated = take(true, align_up((size_t)(Ns + 2 * (size_t)Nt) * 12, 256));      // the source under the mean rotation, room for two target copies
    w.rbar = take(true, 256);                                                       // the mean rotation
    w.lat = take(lt, lat_ws(w.c_max).total);                                        // its first 256 B: the call's header
    w.queue = take(lt, align_up(w.n_records * 16, 256));
    w.val = take(c, align_up(sNs * M * 4, 256));                                    // [Ns x M] f32, in processing order
    w.served = take(c, align_up(sNs * n_words * 8, 256));                           // one bit per query
    w.tmed = take(c, 256);                                                          // the median hypothesis
    w.slices = take(c, align_up((size_t)((Ns + kValSlice - 1) / kValSlice) * M * 4, 256));
    w.gorder = take(c, align_up((size_t)M * 12, 256));                              // global order: perm [M] | inv [M] | err [M]
    w.perm = take(c, align_up(w.n_chunks * M * 4, 256));                            // per-chunk orders
    w.inv = take(c, align_up(w.n_chunks * M * 4, 256));
    w.chunk_of = take(c, align_up(sNs * 4, 256));
    w.centroid = take(c, align_up(w.n_chunks * 16, 256));
    w.b_slack = take(b, align_up((size_t)M * 8, 256));                              // u64 per hypothesis
    w.b_surv = take(b, align_up((size_t)M * 4, 256));                               // survivor flags
    w.b_vpn = take(b, align_up(sNs * 4, 256));                                      // |vp_n|
    w.b_vqmax = take(b, 256);                                                       // max |vq_j|
    w.b_farq = take(b, align_up(sNs * n_words * 8, 256));                           // the queries bounded for lying in far cells (one bit per query, like `served`)
    w.bound_head = w.b_farq - w.b_slack, w.bound_bytes = o - w.b_slack;
    w.cell = take(w.cell_pass, cell_bytes(w.c_max, queries));
    w.flat = take(lt, flat_bytes(w.n_records, queries));
    w.total = o;
    if (lt) {
        assert(w.queue == w.lat + lat_ws(w.c_max).total);                                       // adjacency 1
        assert(w.lat == corr_ws(Ns, Nt, M, flags | UMEREG_CORR_NO_LATTICE).total);              // adjacency 2
        assert(w.cell == w.b_slack + w.bound_bytes);                                            // adjacency 3
    }
    return w;
}

}  // namespace umereg

using namespace umereg;

// ---- stage timing of one corr_scores call (umereg_corr_scores_profile_f32) --------------------------------------------------
// The stages are enqueued by ONE native call, so a caller cannot bracket them with events of its own.  The profile entry
// point hands this thread a row of HIP events; umereg_corr_scores_ex_f32 records event i when it has enqueued stage i's
// last kernel (on the launch stream), and the profile entry reads the differences after a stream synchronise.
constexpr int kCorrStages = 7;      // start | structures + orders | consensus pass | lattice build | list kernel | rest of the leftovers | reduction
static thread_local hipEvent_t* t_corr_marks = nullptr;
static inline void corr_mark(int i, hipStream_t st)
{
    if (t_corr_marks) (void)hipEventRecord(t_corr_marks[i], st);
}

UMEREG_API int umereg_corr_select_best_f32(const float* scores, const float* T, int M, float* T_best, int64_t* best_index, void* stream)
{
    UMEREG_REQUIRE(scores && T && T_best, "corr_select_best: null pointer");
    UMEREG_REQUIRE(M > 0, "corr_select_best: M must be positive (got %d)", M);
    if (int rc = check_device()) return rc;
    hipLaunchKernelGGL(corr_select_best_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, scores, T, M, T_best, best_index);
    UMEREG_CHECK_LAUNCH("corr_select_best_kernel");
    return UMEREG_OK;
}

UMEREG_API size_t umereg_corr_workspace_bytes(int Ns, int Nt, int M) { return umereg_corr_workspace_bytes_ex(Ns, Nt, M, 0); }
UMEREG_API size_t umereg_corr_workspace_bytes_ex(int Ns, int Nt, int M, int flags) { return Ns <= 0 || Nt <= 0 || M <= 0 ? 0 : corr_ws(Ns, Nt, M, flags).total; }

UMEREG_API int umereg_corr_scores_f32(const float* src_pts, const float* tgt_pts, const float* src_wfeat,
                                      const float* tgt_wfeat, const float* T, int Ns, int Nt, int M, int K, float sigma,
                                      float* scores, void* workspace, size_t workspace_bytes, void* stream)
{
    return umereg_corr_scores_ex_f32(src_pts, tgt_pts, src_wfeat, tgt_wfeat, T, Ns, Nt, M, K, sigma, 0, scores, workspace,
                                     workspace_bytes, stream);
}

// ---- one call: what every stage below works on -------------------------------------------------------------------------------
struct CorrCtx {
    const float *src_pts, *tgt_pts, *T;
    const float4 *vp4, *vq4;             // the weighted features
    int Ns, Nt, M, K, flags;
    float sigma, *scores;
    hipStream_t st; CorrWs ws;
    bool consensus, cell_pass, bound;    // routing at launch: the layout's, minus what a misaligned T switches off
    bool far_cells;                      // arg-max mode with a cell pass: queries in far lattice cells are bounded by the scatter (see cell_scatter_kernel)
    bool coop_copy;                      // the Hilbert-ordered copy of the target exists (structures_and_orders)
    long queries;                        // M x Ns
    int n_chunks, n_words, dbg, cap, waves;      // (cap, waves, lds, idx16: knn_lds_plan)
    size_t lds; bool idx16;
    char *ws_src, *ws_tgt, *ws_tgth, *lat;       // the regions; nullptr / zero where the stage that owns them is off
    const char* ws_coop;                 // what the one-wavefront-per-query searches prune with: ws_tgth, or ws_tgt without the copy
    float *partial, *rotated, *Rbar, *val, *Tmed, *slices, *b_vpn;
    unsigned long long *served, *b_slack, *b_farq;
    int *perm, *inv, *chunk_of;          // the per-chunk orders
    unsigned int *b_surv, *b_vqmax;
    CellWs cw; FlatWs fw;
    template <class P> P* at(bool on, size_t off) const { return on ? reinterpret_cast<P*>(ws_src + off) : nullptr; }
};

// bounding boxes of a target table's 64-point chunks (without the Hilbert-ordered copy, the SRC_ROWS route: ws_tgt's own, again in front of every kernel that prunes with them)
static int chunk_boxes(const CorrCtx& c, char* ws)
{
    hipLaunchKernelGGL(chunk_box_kernel, dim3(((c.Nt + kWave - 1) / kWave + 3) / 4, 1), dim3(256), 0, c.st, ws, (size_t)0, c.Nt);
    UMEREG_CHECK_LAUNCH("chunk_box_kernel");
    return UMEREG_OK;
}

// target: the search structure; source: only a processing order (wavefronts of queries that stay row-aligned with the target grid
// under the consensus rotation); and the hypothesis orders of the consensus pass
static int structures_and_orders(const CorrCtx& c)
{
    // ws_tgth: a second copy of the target table in Hilbert-curve order, with the bounding boxes of ITS 64-point chunks: what the
    // one-wavefront-per-query searches (coop_knn) prune with.  Chunks of the row-major table are strips one cell wide and
    // ~40 m long; a far query's bound lets dozens of them through, compact blobs a handful.
    // (compact 64-point chunks of the source where the consensus pass runs; the per-lane grid walk of small jobs keeps the row-aligned strips)
    const int curve_src = c.consensus && !(c.flags & UMEREG_CORR_SRC_ROWS) ? 1 : 0;
    const int Ns = c.Ns, Nt = c.Nt, M = c.M;
    const float radius = -(float)c.K;
    hipLaunchKernelGGL(mean_rotation_kernel, dim3(1), dim3(256), 0, c.st, c.T, M, c.Rbar);
    UMEREG_CHECK_LAUNCH("mean_rotation_kernel");
    if (c.coop_copy && Ns == Nt) {
        // the three structures as one batch of three (their workspaces are consecutive and, the clouds being equally large, equally
        // long): [rotated source | target | target], Hilbert-curve order for the first (if the consensus pass runs) and the third
        hipLaunchKernelGGL(rotate_points_kernel, dim3((Ns + 255) / 256), dim3(256), 0, c.st, c.src_pts, Ns, c.Rbar, c.rotated, c.tgt_pts, 2);
        UMEREG_CHECK_LAUNCH("rotate_points_kernel");
        if (int rc = launch_prep(c.rotated, c.ws_src, 3, Ns, radius, c.st, curve_src | 4)) return rc;
    } else {
        if (int rc = launch_prep(c.tgt_pts, c.ws_tgt, 1, Nt, radius, c.st)) return rc;
        if (c.coop_copy)
            if (int rc = launch_prep(c.tgt_pts, c.ws_tgth, 1, Nt, radius, c.st, 1)) return rc;
        hipLaunchKernelGGL(rotate_points_kernel, dim3((Ns + 255) / 256), dim3(256), 0, c.st, c.src_pts, Ns, c.Rbar, c.rotated, nullptr, 0);
        UMEREG_CHECK_LAUNCH("rotate_points_kernel");
        if (int rc = launch_prep(c.rotated, c.ws_src, 1, Ns, radius, c.st, curve_src)) return rc;
    }
    if (c.coop_copy && chunk_boxes(c, c.ws_tgth) != UMEREG_OK) return UMEREG_ELAUNCH;
    if (c.ws.c_max && hipMemsetAsync(c.lat, 0, 256, c.st) != hipSuccess) { set_error("hipMemsetAsync(lattice header) failed"); return UMEREG_ELAUNCH; }
    if (!c.consensus) return UMEREG_OK;
    // the orders the consensus pass takes the hypotheses in: the median hypothesis, and per 64-point chunk of the source the order around it
    int* gperm = c.at<int>(true, c.ws.gorder);           // the global order: only the fallback of the chunk orders (M > kChunkOrderMax)
    float* err = (float*)(gperm + 2 * M);
    float4* centroid = c.at<float4>(true, c.ws.centroid);
    hipLaunchKernelGGL(hyp_median_kernel, dim3(12), dim3(1024), 0, c.st, c.T, M, c.Tmed);
    UMEREG_CHECK_LAUNCH("hyp_median_kernel");
    if (M > kChunkOrderMax) {
        hipLaunchKernelGGL(hyp_err_kernel, dim3((M + 255) / 256), dim3(256), 0, c.st, c.T, M, (const unsigned int*)(c.ws_src + grid_ws(c.Ns).off_bbox), c.Tmed, err);
        UMEREG_CHECK_LAUNCH("hyp_err_kernel");
        hipLaunchKernelGGL(hyp_order_kernel, dim3((M + kWave - 1) / kWave), dim3(256), 0, c.st, err, M, gperm, gperm + M);
        UMEREG_CHECK_LAUNCH("hyp_order_kernel");
    }
    hipLaunchKernelGGL(chunk_centroid_kernel, dim3((c.n_chunks + 3) / 4), dim3(256), 0, c.st, c.ws_src, c.src_pts, c.Ns, c.chunk_of, centroid);
    UMEREG_CHECK_LAUNCH("chunk_centroid_kernel");
    hipLaunchKernelGGL(hyp_order_chunk_kernel, dim3(c.n_chunks), dim3(1024), 0, c.st, c.T, M, c.Tmed, centroid, gperm, c.perm, c.inv);
    UMEREG_CHECK_LAUNCH("hyp_order_chunk_kernel");
    corr_mark(1, c.st);
    return UMEREG_OK;
}

// consensus pass: scores every (source point, hypothesis) whose image lies near the consensus image of the point, and queues the rest
static int consensus_pass(const CorrCtx& c)
{
    const int Ns = c.Ns, Nt = c.Nt, M = c.M, K = c.K, flags = c.flags;
    unsigned int* header = (unsigned int*)c.lat;
    if (flags & UMEREG_CORR_CONSENSUS_V1) {
        hipLaunchKernelGGL(corr_consensus_kernel, dim3((Ns + 1) / 2), dim3(2 * kWave), 2 * cons_lds_per_wave(c.cap), c.st, c.ws_tgt, c.ws_src, c.src_pts, c.vp4, c.vq4,
                           c.T, c.Tmed, c.perm, Ns, Nt, M, K, c.cap, c.sigma, c.val, c.served, header + 7);
        UMEREG_CHECK_LAUNCH("corr_consensus_kernel");
    } else {
        // images in empty parts of the target stage the ball of radius d_K + margin (in grid cells; flags bits 8..15 in
        // eighths of a cell, 0 = default, 255 = such points give up as in the first form)
        const int mf = (flags >> UMEREG_CORR_FAR_MARGIN_SHIFT) & 0xff;
        const float far_margin = mf == 0 ? kConsFarMarginCells : (mf == 0xff ? 0.f : (float)mf * 0.125f);
        if (!c.coop_copy && chunk_boxes(c, c.ws_tgt) != UMEREG_OK) return UMEREG_ELAUNCH;
        const float act_frac = (c.cell_pass && c.queries >= kCellMinQueries) ? 0.8f : 1.0f;
        const Cons2Args ca = {c.ws_tgt, c.ws_coop, c.ws_src, c.src_pts, c.vp4, c.vq4, c.T, c.Tmed, c.perm, c.val, c.served, header + 7, nullptr,
                              Ns, Nt, M, K, c.sigma, far_margin, c.dbg, act_frac};
        // one wavefront per source point, kC2BlockWaves per workgroup
        hipLaunchKernelGGL(corr_consensus2_kernel, dim3((Ns + kC2BlockWaves - 1) / kC2BlockWaves), dim3(kC2BlockWaves * kWave), kC2BlockWaves * cons2_lds_per_wave(), c.st, ca);
        UMEREG_CHECK_LAUNCH("corr_consensus2_kernel");
    }
    // who takes its leftovers: the grid kernel (few) or the lattice (many); decided on the device, both enqueued
    hipLaunchKernelGGL(leftover_decide_kernel, dim3(1), dim3(1), 0, c.st, header, c.queries,
                       (flags & UMEREG_CORR_LEFT_COOP) ? 1 : ((flags & UMEREG_CORR_LEFT_LATTICE) ? 2 : 0), c.ws.c_max,
                       (c.cell_pass && c.queries < kCellMinQueries && !(flags & UMEREG_CORR_CELL_PASS)) ? kLeftMaxBound : kLeftMax);
    UMEREG_CHECK_LAUNCH("leftover_decide_kernel");
    if (hipMemsetAsync(c.partial, 0, (size_t)M * c.ws.n_chunks * 4, c.st) != hipSuccess) { set_error("hipMemsetAsync(partial) failed"); return UMEREG_ELAUNCH; }
    hipLaunchKernelGGL(leftover_queue_kernel, dim3((unsigned)(((long)c.n_chunks * c.n_words + 3) / 4)), dim3(256), 0, c.st, c.ws_src, Ns, M, c.n_chunks, c.served,
                       c.n_words, c.perm, c.lat, c.ws.c_max);
    UMEREG_CHECK_LAUNCH("leftover_queue_kernel");
    corr_mark(2, c.st);
    return UMEREG_OK;
}

// candidate lattice on the target (built once per pass, used by all M hypotheses): mark -> compact -> list; then the cell pass on it: the
// unserved queries of cells with a list, sorted by cell (counted by the mark kernel), one wavefront per cell (see corr_cell_kernel).
// (with a consensus pass in front, every one of these kernels returns at once unless header word 8 says "lattice")
//   second = false: the call's pass, over the queries the consensus pass left (`served`), or over all of them without one;
//   second = true:  arg-max mode, once the survivors are known: once more on the far-query plane and the surviving hypotheses only
//                   (see bound_pass2_gate_kernel); the values go to the consensus pass's plane.
static int lattice_build_and_cell_pass(const CorrCtx& c, bool second)
{
    const int Ns = c.Ns, Nt = c.Nt, M = c.M, K = c.K;
    const unsigned int c_max = c.ws.c_max;
    const bool far = c.far_cells && !second;                          // this pass bounds the queries of far cells
    unsigned long long* plane = second ? c.b_farq : c.served;         // the pass's queries (a clear bit in `served`, a set one in the far-query plane) ...
    const unsigned int* only = second ? c.b_surv : nullptr;           // ... of these hypotheses
    if (second) hipLaunchKernelGGL(bound_pass2_gate_kernel, dim3(1), dim3(1), 0, c.st, (unsigned int*)c.lat);
    if (hipMemsetAsync(c.lat + 256, 0, lat_ws(c_max).off_wave_tot - 256, c.st) != hipSuccess) { set_error("hipMemsetAsync(lattice marks) failed"); return UMEREG_ELAUNCH; }
    if (c.bound && !second) {
        // the bound's slack / survivor flags / norms / far-query plane, and what every bounding kernel needs before it runs
        // (one fill for the block -- slack, flags, norms, maximum, plane: the norms are written after it --, one launch for both sets of rows:
        // every launch of this chain is 4-5 us of a KITTI-test call whether it finds work or not; and the cell pass's counters right behind it: CorrWs, adjacency 3)
        if (hipMemsetAsync(c.b_slack, 0, far ? c.ws.bound_bytes + (size_t)c_max * 4 : c.ws.bound_head, c.st) != hipSuccess) { set_error("hipMemsetAsync(slack) failed"); return UMEREG_ELAUNCH; }
        hipLaunchKernelGGL(row_norm_kernel, dim3((Ns + 255) / 256 + (Nt + 255) / 256), dim3(256), 0, c.st, c.vp4, Ns, c.b_vpn, c.vq4, Nt, c.b_vqmax);
        UMEREG_CHECK_LAUNCH("row_norm_kernel");
    }
    if (c.cell_pass && !far && hipMemsetAsync(c.cw.cnt, 0, (size_t)c_max * 4, c.st) != hipSuccess) { set_error("hipMemsetAsync(cell counters) failed"); return UMEREG_ELAUNCH; }
    const long order_items = (long)((Ns + 255) / 256) * c.n_words;
    const dim3 order_grid((unsigned)(order_items < 16384 ? order_items : 16384));
    if (far) {
        if (!c.coop_copy && chunk_boxes(c, c.ws_tgt) != UMEREG_OK) return UMEREG_ELAUNCH;
        hipLaunchKernelGGL(lattice_far_table_kernel, dim3((c_max + 255) / 256), dim3(256), 0, c.st, c.ws_coop, c.ws_tgt, c.lat, c_max, Nt, c.sigma);
        hipLaunchKernelGGL(lattice_mark_order_kernel, order_grid, dim3(256), 0, c.st, c.ws_tgt, c.ws_src, c.src_pts, c.T, Ns, Nt, M, c.lat, c_max, plane, c.n_words, c.perm,
                           c.cw.cnt, false, nullptr, K, c.sigma, c.b_vpn, c.b_vqmax, c.b_slack, c.b_farq, c.served);
    } else if (plane)
        hipLaunchKernelGGL(lattice_mark_order_kernel, order_grid, dim3(256), 0, c.st, c.ws_tgt, c.ws_src, c.src_pts, c.T, Ns, Nt, M, c.lat, c_max, plane, c.n_words, c.perm,
                           c.cw.cnt, second, only);
    else
        hipLaunchKernelGGL(lattice_mark_kernel, dim3((Ns + 255) / 256, (M + 15) / 16), dim3(256), 0, c.st, c.ws_tgt, c.src_pts, c.T, Ns, Nt, M, 16 /* hypotheses per thread */,
                           c.lat, c_max, c.served, c.n_words, c.inv, c.chunk_of, c.cw.cnt);
    UMEREG_CHECK_LAUNCH("lattice_mark_kernel");
    hipLaunchKernelGGL(lattice_compact_kernel, dim3(kCompactBlocks), dim3(1024), 0, c.st, c.ws_tgt, c.lat, c_max, Nt);
    UMEREG_CHECK_LAUNCH("lattice_compact_kernel");
    if (!second) {
        if (!c.coop_copy && chunk_boxes(c, c.ws_tgt) != UMEREG_OK) return UMEREG_ELAUNCH;
        hipLaunchKernelGGL(lattice_posof_kernel, dim3((Nt + 255) / 256), dim3(256), 0, c.st, c.ws_tgt, c.lat, c_max, Nt);
    }
    // (grids of the kernels that usually find nothing to do -- the leftovers go to the queue up to 2 M -- are kept small: a
    // workgroup that returns at once still costs its launch, 50 us for 1 024 x 512 threads with 33 KiB of LDS each)
    // (idle on jobs whose leftovers go to the queue -- every KITTI-test pair --, where its launch alone was 60 us of a pair's 3.7 ms
    // beside other streams' kernels: the full grid only where the lattice is the likely path)
    hipLaunchKernelGGL(lattice_list_kernel, dim3(second || c.queries >= kCellMinQueries ? 512 : 256), dim3(8 * kWave), 0, c.st, c.ws_coop, c.ws_tgt, c.lat, c_max, Nt, K,
                       c.sigma, far ? 1 : 0);
    UMEREG_CHECK_LAUNCH("lattice_list_kernel");
    if (!c.cell_pass) return UMEREG_OK;
    const unsigned int nb = (c_max + 1023u) / 1024u;
    hipLaunchKernelGGL(cell_apply_kernel<0>, dim3(nb), dim3(1024), 0, c.st, c.lat, c_max, c.cw);
    hipLaunchKernelGGL(cell_blockscan_kernel, dim3(1), dim3(1024), 0, c.st, c.lat, c_max, c.cw);
    hipLaunchKernelGGL(cell_apply_kernel<1>, dim3(nb), dim3(1024), 0, c.st, c.lat, c_max, c.cw);
    UMEREG_CHECK_LAUNCH("cell_apply_kernel");
    // (the second pass bounds nothing: no norms, no slack, no plane to write)
    hipLaunchKernelGGL(cell_scatter_kernel, order_grid, dim3(256), 0, c.st, c.ws_tgt, c.ws_src, c.src_pts, c.T, Ns, Nt, M, c.lat, c_max, plane, c.n_words, c.perm, c.cw, K,
                       c.sigma, second ? nullptr : c.b_vpn, second ? nullptr : c.b_vqmax, far ? c.b_slack : nullptr, second ? nullptr : c.b_farq, second, only);
    UMEREG_CHECK_LAUNCH("cell_scatter_kernel");
    const int dbg = second ? 0 : c.dbg;
    unsigned long long* farq_clear = second ? c.b_farq : nullptr;
    hipLaunchKernelGGL(corr_cell_kernel<false>, dim3(2816), dim3(kWave), cell_lds_per_wave(K, false), c.st, c.ws_tgt, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, M, K, c.sigma,
                       c.lat, c_max, c.cw, c.val, c.served, dbg, farq_clear);
    hipLaunchKernelGGL(corr_cell_kernel<true>, dim3(2048), dim3(kWave), cell_lds_per_wave(K, true), c.st, c.ws_tgt, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, M, K, c.sigma,
                       c.lat, c_max, c.cw, c.val, c.served, dbg, farq_clear);
    UMEREG_CHECK_LAUNCH("corr_cell_kernel");
    return UMEREG_OK;
}

// the queries the passes above left.  One lane per query: through the lattice's lists where there is a lattice (queueing what it cannot serve), the
// per-lane grid walk otherwise.  Then the records the score kernels queued: queries outside the lattice / in cells without a list, far-off chunks
// ... as a flat list of queries when they fit (header word 12 marks that the flat path ran), record by record otherwise
static int score_queries(const CorrCtx& c)
{
    const int Ns = c.Ns, Nt = c.Nt, M = c.M, K = c.K, flags = c.flags;
    const unsigned int c_max = c.ws.c_max;
    if (c_max) corr_mark(3, c.st);                                  // (the lattice build and cell pass end where this stage begins)
    const int hyp_per_wave = 2;   // 1..4 measured equal (6.4 us per hypothesis), 8: 6.7, 16: 7.3 (balance at the tail, parallelism)
    const long n_waves = (long)c.n_chunks * ((M + hyp_per_wave - 1) / hyp_per_wave);
    const dim3 score_grid((unsigned)((n_waves + c.waves - 1) / c.waves)), score_block(c.waves * kWave);
    if (c_max) {
        const dim3 lat_grid(score_grid.x < 4096u ? score_grid.x : 4096u);
        hipLaunchKernelGGL((corr_score_kernel<unsigned short, true>), lat_grid, score_block, c.lds, c.st, c.ws_tgt, c.ws_src, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, M, K, c.cap,
                           c.sigma, hyp_per_wave, c.n_chunks, c.partial, c.lat, c_max, c.served, c.n_words, c.inv, c.cell_pass ? 1 : 0, c.perm);
    } else if (c.idx16)
        hipLaunchKernelGGL((corr_score_kernel<unsigned short, false>), score_grid, score_block, c.lds, c.st, c.ws_tgt, c.ws_src, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, M, K, c.cap,
                           c.sigma, hyp_per_wave, c.n_chunks, c.partial, nullptr, 0u, nullptr, 0, nullptr);
    else
        hipLaunchKernelGGL((corr_score_kernel<unsigned int, false>), score_grid, score_block, c.lds, c.st, c.ws_tgt, c.ws_src, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, M, K, c.cap,
                           c.sigma, hyp_per_wave, c.n_chunks, c.partial, nullptr, 0u, nullptr, 0, nullptr);
    UMEREG_CHECK_LAUNCH("corr_score_kernel");
    if (!c_max) return UMEREG_OK;
    corr_mark(4, c.st);
    if ((flags & UMEREG_CORR_RECORD_STAGE) && !(flags & UMEREG_CORR_NO_FLAT)) {
        // first one wavefront per record (a staged set of the record's neighbours, one lane per query); the records keep the lanes it could not serve
        if (c.idx16)
            hipLaunchKernelGGL(corr_score_record2_kernel<unsigned short>, dim3(4096), dim3(2 * kWave), 2 * rec_lds_per_wave<unsigned short>(c.cap), c.st, c.ws_coop, c.ws_src,
                               c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, K, c.cap, c.sigma, c.n_chunks, c.partial, c.lat, c_max, c.dbg);
        else
            hipLaunchKernelGGL(corr_score_record2_kernel<unsigned int>, dim3(4096), dim3(2 * kWave), 2 * rec_lds_per_wave<unsigned int>(c.cap), c.st, c.ws_coop, c.ws_src,
                               c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, K, c.cap, c.sigma, c.n_chunks, c.partial, c.lat, c_max, c.dbg);
        UMEREG_CHECK_LAUNCH("corr_score_record2_kernel");
    }
    if (!(flags & UMEREG_CORR_NO_FLAT)) {
        hipLaunchKernelGGL(leftover_flatten_kernel, dim3(256), dim3(256), 0, c.st, c.lat, c_max, c.fw);
        UMEREG_CHECK_LAUNCH("leftover_flatten_kernel");
        if (c.bound) {
            hipLaunchKernelGGL(flat_bound_kernel<1>, dim3(2048), dim3(256), 0, c.st, c.ws_tgt, c.ws_src, c.src_pts, c.T, Ns, Nt, K, c.sigma, c.lat, c_max, c.fw, c.b_vpn,
                               c.b_vqmax, c.b_slack, c.b_surv);
            UMEREG_CHECK_LAUNCH("flat_bound_kernel");
            hipLaunchKernelGGL(corr_score_flat_kernel<3>, dim3(kFlatBlocks), dim3(kCoopWaves * kWave), 0, c.st, c.ws_coop, c.ws_src, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, K,
                               c.sigma, c.lat, c_max, c.fw, c.b_vpn, c.b_vqmax, c.b_slack);
        } else
            hipLaunchKernelGGL(corr_score_flat_kernel<0>, dim3(kFlatBlocks), dim3(kCoopWaves * kWave), 0, c.st, c.ws_coop, c.ws_src, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, K,
                               c.sigma, c.lat, c_max, c.fw);
        UMEREG_CHECK_LAUNCH("corr_score_flat_kernel");
        hipLaunchKernelGGL(leftover_sum_kernel, dim3(256), dim3(256), 0, c.st, c.lat, c_max, c.fw, c.n_chunks, c.partial, 0);
        UMEREG_CHECK_LAUNCH("leftover_sum_kernel");
    }
    // (with the flat list in front this kernel only has work when that list overflowed -- more leftovers than half the job's queries --:
    // 128 workgroups, its idle launch was 70 us per end-to-end pair at 512)
    hipLaunchKernelGGL(corr_score_fallback_kernel, dim3((flags & UMEREG_CORR_NO_FLAT) ? 4096 : 128), dim3(kCoopWaves * kWave), 0, c.st, c.ws_coop, c.ws_src, c.src_pts,
                       c.vp4, c.vq4, c.T, Ns, Nt, K, c.sigma, c.n_chunks, c.partial, c.lat, c_max);
    UMEREG_CHECK_LAUNCH("corr_score_fallback_kernel");
    corr_mark(5, c.st);
    return UMEREG_OK;
}

// scores = the chunks' partial sums + the consensus pass's plane, in a fixed order.  last: the call's final reduction (the plane summed
// in processing order and, in arg-max mode, for the surviving hypotheses only)
static int reduce_scores(const CorrCtx& c, bool last)
{
    const int n_slices = c.val ? (c.Ns + kValSlice - 1) / kValSlice : 0;
    if (c.val) {
        hipLaunchKernelGGL(corr_val_slices_kernel, dim3((c.M + 255) / 256, n_slices), dim3(256), 0, c.st, c.val, c.M, c.Ns, c.ws_src, c.slices, last ? c.perm : nullptr,
                           last ? c.b_surv : nullptr);
        UMEREG_CHECK_LAUNCH("corr_val_slices_kernel");
    }
    hipLaunchKernelGGL(corr_reduce_kernel, dim3((c.M + 3) / 4), dim3(256), 0, c.st, c.partial, c.M, c.n_chunks, c.Ns, c.slices, n_slices, c.inv, c.scores);
    UMEREG_CHECK_LAUNCH("corr_reduce_kernel");
    if (last) corr_mark(6, c.st);
    return UMEREG_OK;
}

// arg-max mode: the scores so far decide which hypotheses need their bounded queries; those queries, exactly; then (the caller) the sums once more
static int bounded_recompute(const CorrCtx& c)
{
    const int Ns = c.Ns, Nt = c.Nt, M = c.M, K = c.K;
    const unsigned int c_max = c.ws.c_max;
    if (int rc = reduce_scores(c, false)) return rc;
    hipLaunchKernelGGL(bound_survivors_kernel, dim3(1), dim3(1024), 0, c.st, c.scores, c.b_slack, M, Ns, c.b_surv, (unsigned int*)c.lat);
    UMEREG_CHECK_LAUNCH("bound_survivors_kernel");
    hipLaunchKernelGGL(flat_bound_kernel<2>, dim3(2048), dim3(256), 0, c.st, c.ws_tgt, c.ws_src, c.src_pts, c.T, Ns, Nt, K, c.sigma, c.lat, c_max, c.fw, c.b_vpn, c.b_vqmax,
                       c.b_slack, c.b_surv);
    UMEREG_CHECK_LAUNCH("flat_bound_kernel");
    hipLaunchKernelGGL(corr_score_flat_kernel<3>, dim3(kFlatBlocks), dim3(kCoopWaves * kWave), 0, c.st, c.ws_coop, c.ws_src, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, K, c.sigma,
                       c.lat, c_max, c.fw);
    UMEREG_CHECK_LAUNCH("corr_score_flat_kernel");
    hipLaunchKernelGGL(leftover_sum_kernel, dim3(256), dim3(256), 0, c.st, c.lat, c_max, c.fw, c.n_chunks, c.partial, 1);
    UMEREG_CHECK_LAUNCH("leftover_sum_kernel");
    if (c.far_cells) {
        // ... and the queries bounded for lying in far lattice cells: through the lattice + cell pass once more, then one by one what that left
        if (int rc = lattice_build_and_cell_pass(c, true)) return rc;
        hipLaunchKernelGGL(far_recompute_kernel, dim3(1024), dim3(kCoopWaves * kWave), 0, c.st, c.ws_coop, c.ws_src, c.src_pts, c.vp4, c.vq4, c.T, Ns, Nt, M, K, c.sigma,
                           c.lat, c_max, c.b_farq, c.n_words, c.perm, c.b_surv, c.val);
        UMEREG_CHECK_LAUNCH("far_recompute_kernel");
    }
    return UMEREG_OK;
}

UMEREG_API int umereg_corr_scores_ex_f32(const float* src_pts, const float* tgt_pts, const float* src_wfeat,
                                         const float* tgt_wfeat, const float* T, int Ns, int Nt, int M, int K, float sigma,
                                         int flags, float* scores, void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(src_pts && tgt_pts && src_wfeat && tgt_wfeat && T && scores, "corr_scores: null pointer");
    UMEREG_REQUIRE(Ns > 0 && Nt > 0 && M > 0, "corr_scores: Ns, Nt, M must be positive");
    UMEREG_REQUIRE(K > 0 && K <= 64 && K <= Nt, "corr_scores: K must be in [1, min(64, Nt)] (got %d)", K);
    UMEREG_REQUIRE(sigma > 0.f, "corr_scores: sigma must be positive");
    UMEREG_REQUIRE(((uintptr_t)src_wfeat & 15) == 0 && ((uintptr_t)tgt_wfeat & 15) == 0, "corr_scores: features must be 16-byte aligned");
    if (int rc = check_device()) return rc;
    const CorrWs ws = corr_ws(Ns, Nt, M, flags);
    if (!workspace || workspace_bytes < ws.total || ((uintptr_t)workspace & 15)) {
        set_error("corr_scores: workspace too small or misaligned (%zu < %zu)", workspace_bytes, ws.total);
        return UMEREG_EWORKSPACE;
    }
    CorrCtx c = {};
    c.src_pts = src_pts; c.tgt_pts = tgt_pts; c.vp4 = (const float4*)src_wfeat; c.vq4 = (const float4*)tgt_wfeat; c.T = T;
    c.Ns = Ns; c.Nt = Nt; c.M = M; c.K = K; c.flags = flags; c.sigma = sigma; c.scores = scores; c.st = (hipStream_t)stream; c.ws = ws;
    const bool t_rows16 = ((uintptr_t)T & 15) == 0;            // the consensus pass reads hypothesis rows as 16-byte vectors
    c.consensus = ws.consensus && t_rows16; c.cell_pass = ws.cell_pass && t_rows16; c.bound = ws.bound;
    c.far_cells = c.bound && c.cell_pass; c.coop_copy = ws.c_max != 0 && !(flags & UMEREG_CORR_SRC_ROWS);
    c.queries = (long)M * Ns; c.n_chunks = (int)ws.n_chunks; c.n_words = (M + 63) / 64; c.dbg = (flags & UMEREG_CORR_DEBUG_STATS) ? 1 : 0;
    knn_lds_plan(K, Nt, &c.cap, &c.waves, &c.lds, 2, &c.idx16);
    c.ws_src = (char*)workspace; c.ws_tgt = c.at<char>(true, ws.tgt); c.ws_tgth = c.at<char>(true, ws.tgth); c.ws_coop = c.coop_copy ? c.ws_tgth : c.ws_tgt;
    c.partial = c.at<float>(true, ws.partial); c.rotated = c.at<float>(true, ws.rotated); c.Rbar = c.at<float>(true, ws.rbar); c.lat = c.at<char>(true, ws.lat);
    c.val = c.at<float>(c.consensus, ws.val); c.served = c.at<unsigned long long>(c.consensus, ws.served); c.Tmed = c.at<float>(c.consensus, ws.tmed);
    c.slices = c.at<float>(c.consensus, ws.slices); c.perm = c.at<int>(c.consensus, ws.perm); c.inv = c.at<int>(c.consensus, ws.inv); c.chunk_of = c.at<int>(c.consensus, ws.chunk_of);
    c.b_slack = c.at<unsigned long long>(c.bound, ws.b_slack); c.b_surv = c.at<unsigned int>(c.bound, ws.b_surv); c.b_vpn = c.at<float>(c.bound, ws.b_vpn);
    c.b_vqmax = c.at<unsigned int>(c.bound, ws.b_vqmax); c.b_farq = c.at<unsigned long long>(c.bound, ws.b_farq);
    if (c.cell_pass) c.cw = cell_ws(c.at<char>(true, ws.cell), ws.c_max, c.queries);
    if (ws.c_max) c.fw = flat_ws(c.at<char>(true, ws.flat), ws.n_records, c.queries);

    corr_mark(0, c.st);                                     // (marks 1 .. 6: inside the stages, where each ends)
    if (int rc = structures_and_orders(c)) return rc;
    if (c.consensus)
        if (int rc = consensus_pass(c)) return rc;
    if (ws.c_max)
        if (int rc = lattice_build_and_cell_pass(c, false)) return rc;
    if (int rc = score_queries(c)) return rc;
    if (c.bound)
        if (int rc = bounded_recompute(c)) return rc;
    return reduce_scores(c, true);
}

UMEREG_API int umereg_corr_scores_profile_f32(const float* src_pts, const float* tgt_pts, const float* src_wfeat,
                                              const float* tgt_wfeat, const float* T, int Ns, int Nt, int M, int K, float sigma,
                                              int flags, float* scores, void* workspace, size_t workspace_bytes, void* stream,
                                              float* stage_ms_host)
{
    UMEREG_REQUIRE(stage_ms_host, "corr_scores_profile: null pointer");
    if (int rc = check_device()) return rc;
    hipEvent_t ev[kCorrStages + 1];                 // [kCorrStages] = the base, recorded before everything
    for (int i = 0; i <= kCorrStages; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) { set_error("corr_scores_profile: hipEventCreate failed"); return UMEREG_ELAUNCH; }
    hipStream_t st = (hipStream_t)stream;
    // a stage that a configuration skips (no consensus pass, no lattice) never records its mark: every mark is recorded once
    // up front, right after the base, so that a skipped stage reads as "no later than the stage before it"
    (void)hipEventRecord(ev[kCorrStages], st);
    for (int i = 0; i < kCorrStages; ++i) (void)hipEventRecord(ev[i], st);
    t_corr_marks = ev;
    const int rc = umereg_corr_scores_ex_f32(src_pts, tgt_pts, src_wfeat, tgt_wfeat, T, Ns, Nt, M, K, sigma, flags, scores, workspace,
                                             workspace_bytes, stream);
    t_corr_marks = nullptr;
    int out = rc;
    if (rc == UMEREG_OK) {
        if (hipStreamSynchronize(st) != hipSuccess) { set_error("corr_scores_profile: hipStreamSynchronize failed"); out = UMEREG_ELAUNCH; }
        float at[kCorrStages];                      // time of mark i since the base, made monotone
        for (int i = 0; i < kCorrStages && out == UMEREG_OK; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[kCorrStages], ev[i]) != hipSuccess) ms = 0.f;
            at[i] = i > 0 && ms < at[i - 1] ? at[i - 1] : ms;
        }
        if (out == UMEREG_OK) {
            for (int i = 0; i + 1 < kCorrStages; ++i) stage_ms_host[i] = at[i + 1] - at[i];
            stage_ms_host[kCorrStages - 1] = at[kCorrStages - 1] - at[0];
        }
    }
    for (int i = 0; i <= kCorrStages; ++i) (void)hipEventDestroy(ev[i]);
    return out;
}
