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
// Files (one translation unit each; corr_dev.h = shared inline device code, corr_host.h = CorrWs, CorrCtx and the launcher declarations).
// A kernel is defined in exactly one unit and launched only there, by the host launcher that follows it (grid, block and LDS arithmetic
// live with the kernel they describe); this file defines and launches none:
//   corr.hip            this file, host only: routing thresholds, the workspace layout (corr_ws: the one place that knows it), the stage functions --
//                       sequences of launcher calls and fills -- and umereg_corr_scores_ex_f32, the ONE call that enqueues them, its stage profile
//   corr_knn.hip        knn_points / feature_spatial_var / weighted features + their entry points, chunk boxes
//   corr_consensus.hip  orders + the consensus pass
//   corr_lattice.hip    candidate lattice, cell pass, second pass of the arg-max mode
//   corr_leftover.hip   per-lane grid walk, one wavefront per query (queue / flat / records), outside bound, reductions, pick + its entry point
#include <assert.h>

#include "corr_host.h"

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
// who takes what the consensus pass left (header word 8): 1 = the grid kernel (few leftovers: they sit in a few
// thousand (hypothesis, chunk) wavefronts), 0 = the candidate lattice (many: hypotheses that do not agree, clouds that
// barely overlap -- queries in empty parts of the target, where lists pay off).  Both sets of kernels are enqueued;
// the ones not chosen return at once.
#ifndef UMEREG_LEFT_MAX
#define UMEREG_LEFT_MAX 3000000u
#endif
constexpr unsigned int kLeftMax = UMEREG_LEFT_MAX;      // (2^21 until the end of round 3: over 32 half-overlapping KITTI-test pairs, whose leftovers straddle
                                                        // 2 M, f1 averages 7.5 ms with 2^21 and 6.4 with 3 M or 4.5 M -- the flat list holds half the job's queries now)   // (measured round 3, with the Hilbert-ordered copy: 0.26 M leftovers 2.2 ms through the queue against 3.2 through the lattice, 1.6 M 7.8 against 8.1)
#ifndef UMEREG_LEFT_MAX_BOUND
#define UMEREG_LEFT_MAX_BOUND 1000000u
#endif
constexpr unsigned int kLeftMaxBound = UMEREG_LEFT_MAX_BOUND;      // kLeftMax where the cell pass rides in arg-max mode on a job below 2^25 queries

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

// (the flat list of leftover queries: corr_leftover.hip)
constexpr unsigned int kFlatMaxQ = 1u << 21;
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

// ---- the workspace of one corr_scores call: routing and layout (CorrWs, corr_host.h: the regions and the three adjacencies asserted below) ----
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

UMEREG_API size_t umereg_corr_workspace_bytes(int Ns, int Nt, int M) { return umereg_corr_workspace_bytes_ex(Ns, Nt, M, 0); }
UMEREG_API size_t umereg_corr_workspace_bytes_ex(int Ns, int Nt, int M, int flags) { return Ns <= 0 || Nt <= 0 || M <= 0 ? 0 : corr_ws(Ns, Nt, M, flags).total; }

UMEREG_API int umereg_corr_scores_f32(const float* src_pts, const float* tgt_pts, const float* src_wfeat,
                                      const float* tgt_wfeat, const float* T, int Ns, int Nt, int M, int K, float sigma,
                                      float* scores, void* workspace, size_t workspace_bytes, void* stream)
{
    return umereg_corr_scores_ex_f32(src_pts, tgt_pts, src_wfeat, tgt_wfeat, T, Ns, Nt, M, K, sigma, 0, scores, workspace,
                                     workspace_bytes, stream);
}

// bounding boxes of a target table's 64-point chunks (without the Hilbert-ordered copy, the SRC_ROWS route: ws_tgt's own, again in front of every kernel that prunes with them)
static int chunk_boxes(const CorrCtx& c, char* ws) { return launch_chunk_box(ws, 0, c.Nt, 1, c.st); }

// target: the search structure; source: only a processing order (wavefronts of queries that stay row-aligned with the target grid
// under the consensus rotation); and the hypothesis orders of the consensus pass
static int structures_and_orders(const CorrCtx& c)
{
    // ws_tgth: a second copy of the target table in Hilbert-curve order, with the bounding boxes of ITS 64-point chunks: what the
    // one-wavefront-per-query searches (coop_knn) prune with.  Chunks of the row-major table are strips one cell wide and
    // ~40 m long; a far query's bound lets dozens of them through, compact blobs a handful.
    // (compact 64-point chunks of the source where the consensus pass runs; the per-lane grid walk of small jobs keeps the row-aligned strips)
    const int curve_src = c.consensus && !(c.flags & UMEREG_CORR_SRC_ROWS) ? 1 : 0;
    const int Ns = c.Ns, Nt = c.Nt;
    const float radius = -(float)c.K;
    if (int rc = launch_mean_rotation(c)) return rc;
    if (c.coop_copy && Ns == Nt) {
        // the three structures as one batch of three (their workspaces are consecutive and, the clouds being equally large, equally
        // long): [rotated source | target | target], Hilbert-curve order for the first (if the consensus pass runs) and the third
        if (int rc = launch_rotate_points(c, true)) return rc;
        if (int rc = launch_prep(c.rotated, c.ws_src, 3, Ns, radius, c.st, curve_src | 4)) return rc;
    } else {
        if (int rc = launch_prep(c.tgt_pts, c.ws_tgt, 1, Nt, radius, c.st)) return rc;
        if (c.coop_copy)
            if (int rc = launch_prep(c.tgt_pts, c.ws_tgth, 1, Nt, radius, c.st, 1)) return rc;
        if (int rc = launch_rotate_points(c, false)) return rc;
        if (int rc = launch_prep(c.rotated, c.ws_src, 1, Ns, radius, c.st, curve_src)) return rc;
    }
    if (c.coop_copy)
        if (int rc = chunk_boxes(c, c.ws_tgth)) return rc;
    if (c.ws.c_max && hipMemsetAsync(c.lat, 0, 256, c.st) != hipSuccess) { set_error("hipMemsetAsync(lattice header) failed"); return UMEREG_ELAUNCH; }
    if (!c.consensus) return UMEREG_OK;
    // the orders the consensus pass takes the hypotheses in: the median hypothesis, and per 64-point chunk of the source the order around it
    // (the global order: only the fallback of the chunk orders)
    if (int rc = launch_hyp_median(c)) return rc;
    if (c.M > kChunkOrderMax) {
        if (int rc = launch_hyp_err(c)) return rc;
        if (int rc = launch_hyp_order(c)) return rc;
    }
    if (int rc = launch_chunk_centroid(c)) return rc;
    if (int rc = launch_hyp_order_chunk(c)) return rc;
    corr_mark(1, c.st);
    return UMEREG_OK;
}

// consensus pass: scores every (source point, hypothesis) whose image lies near the consensus image of the point, and queues the rest
static int consensus_pass(const CorrCtx& c)
{
    const int flags = c.flags;
    if (flags & UMEREG_CORR_CONSENSUS_V1) {
        if (int rc = launch_corr_consensus(c)) return rc;
    } else {
        // images in empty parts of the target stage the ball of radius d_K + margin (in grid cells; flags bits 8..15 in
        // eighths of a cell, 0 = default, 255 = such points give up as in the first form)
        const int mf = (flags >> UMEREG_CORR_FAR_MARGIN_SHIFT) & 0xff;
        const float far_margin = mf == 0 ? kConsFarMarginCells : (mf == 0xff ? 0.f : (float)mf * 0.125f);
        if (!c.coop_copy)
            if (int rc = chunk_boxes(c, c.ws_tgt)) return rc;
        const float act_frac = (c.cell_pass && c.queries >= kCellMinQueries) ? 0.8f : 1.0f;
        if (int rc = launch_corr_consensus2(c, far_margin, act_frac)) return rc;
    }
    // who takes its leftovers: the grid kernel (few) or the lattice (many); decided on the device, both enqueued
    if (int rc = launch_leftover_decide(c, (c.cell_pass && c.queries < kCellMinQueries && !(flags & UMEREG_CORR_CELL_PASS)) ? kLeftMaxBound : kLeftMax)) return rc;
    if (hipMemsetAsync(c.partial, 0, (size_t)c.M * c.ws.n_chunks * 4, c.st) != hipSuccess) { set_error("hipMemsetAsync(partial) failed"); return UMEREG_ELAUNCH; }
    if (int rc = launch_leftover_queue(c)) return rc;
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
    const unsigned int c_max = c.ws.c_max;
    const bool far = c.far_cells && !second;                          // this pass bounds the queries of far cells
    if (second)
        if (int rc = launch_bound_pass2_gate(c)) return rc;
    if (hipMemsetAsync(c.lat + 256, 0, lat_ws(c_max).off_wave_tot - 256, c.st) != hipSuccess) { set_error("hipMemsetAsync(lattice marks) failed"); return UMEREG_ELAUNCH; }
    if (c.bound && !second) {
        // the bound's slack / survivor flags / norms / far-query plane, and what every bounding kernel needs before it runs
        // (one fill for the block -- slack, flags, norms, maximum, plane: the norms are written after it --, one launch for both sets of rows:
        // every launch of this chain is 4-5 us of a KITTI-test call whether it finds work or not; and the cell pass's counters right behind it: CorrWs, adjacency 3)
        if (hipMemsetAsync(c.b_slack, 0, far ? c.ws.bound_bytes + (size_t)c_max * 4 : c.ws.bound_head, c.st) != hipSuccess) { set_error("hipMemsetAsync(slack) failed"); return UMEREG_ELAUNCH; }
        if (int rc = launch_row_norm(c)) return rc;
    }
    if (c.cell_pass && !far && hipMemsetAsync(c.cw.cnt, 0, (size_t)c_max * 4, c.st) != hipSuccess) { set_error("hipMemsetAsync(cell counters) failed"); return UMEREG_ELAUNCH; }
    // the pass's queries: a clear bit in `served`, a set one in the far-query plane; without a consensus pass there is no plane, and every query is marked
    if (far) {
        if (!c.coop_copy)
            if (int rc = chunk_boxes(c, c.ws_tgt)) return rc;
        if (int rc = launch_lattice_far_table(c)) return rc;
    }
    if (int rc = second || c.served ? launch_lattice_mark_order(c, second) : launch_lattice_mark(c)) return rc;
    if (int rc = launch_lattice_compact(c)) return rc;
    if (!second) {
        if (!c.coop_copy)
            if (int rc = chunk_boxes(c, c.ws_tgt)) return rc;
        if (int rc = launch_lattice_posof(c)) return rc;
    }
    if (int rc = launch_lattice_list(c, second, second || c.queries >= kCellMinQueries)) return rc;
    if (!c.cell_pass) return UMEREG_OK;
    if (int rc = launch_cell_offsets(c)) return rc;
    if (int rc = launch_cell_scatter(c, second)) return rc;
    return launch_corr_cell(c, second);
}

// the queries the passes above left.  One lane per query: through the lattice's lists where there is a lattice (queueing what it cannot serve), the
// per-lane grid walk otherwise.  Then the records the score kernels queued: queries outside the lattice / in cells without a list, far-off chunks
// ... as a flat list of queries when they fit (header word 12 marks that the flat path ran), record by record otherwise
static int score_queries(const CorrCtx& c)
{
    const int flags = c.flags;
    if (c.ws.c_max) corr_mark(3, c.st);                             // (the lattice build and cell pass end where this stage begins)
    if (int rc = launch_corr_score(c)) return rc;
    if (!c.ws.c_max) return UMEREG_OK;
    corr_mark(4, c.st);
    // first one wavefront per record (a staged set of the record's neighbours, one lane per query); the records keep the lanes it could not serve
    if ((flags & UMEREG_CORR_RECORD_STAGE) && !(flags & UMEREG_CORR_NO_FLAT))
        if (int rc = launch_corr_score_record2(c)) return rc;
    if (!(flags & UMEREG_CORR_NO_FLAT)) {
        if (int rc = launch_leftover_flatten(c)) return rc;
        if (c.bound)
            if (int rc = launch_flat_bound(c, 1)) return rc;
        if (int rc = c.bound ? launch_corr_score_flat(c, 3, true) : launch_corr_score_flat(c, 0, false)) return rc;
        if (int rc = launch_leftover_sum(c, false)) return rc;
    }
    if (int rc = launch_corr_score_fallback(c)) return rc;
    corr_mark(5, c.st);
    return UMEREG_OK;
}

// scores = the chunks' partial sums + the consensus pass's plane, in a fixed order.  last: the call's final reduction (the plane summed
// in processing order and, in arg-max mode, for the surviving hypotheses only)
static int reduce_scores(const CorrCtx& c, bool last)
{
    if (c.val)
        if (int rc = launch_corr_val_slices(c, last)) return rc;
    if (int rc = launch_corr_reduce(c)) return rc;
    if (last) corr_mark(6, c.st);
    return UMEREG_OK;
}

// arg-max mode: the scores so far decide which hypotheses need their bounded queries; those queries, exactly; then (the caller) the sums once more
static int bounded_recompute(const CorrCtx& c)
{
    if (int rc = reduce_scores(c, false)) return rc;
    if (int rc = launch_bound_survivors(c)) return rc;
    if (int rc = launch_flat_bound(c, 2)) return rc;
    if (int rc = launch_corr_score_flat(c, 3, false)) return rc;
    if (int rc = launch_leftover_sum(c, true)) return rc;
    if (c.far_cells) {
        // ... and the queries bounded for lying in far lattice cells: through the lattice + cell pass once more, then one by one what that left
        if (int rc = lattice_build_and_cell_pass(c, true)) return rc;
        if (int rc = launch_far_recompute(c)) return rc;
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
    UMEREG_REQUIRE_WORKSPACE("corr_scores", workspace, workspace_bytes, ws.total);
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
    c.gorder = c.at<int>(c.consensus, ws.gorder); c.centroid = c.at<float4>(c.consensus, ws.centroid);
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
