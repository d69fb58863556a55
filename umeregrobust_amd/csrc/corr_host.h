// corr_host.h -- host side of SURVEY 8(f1) shared by its translation units: the workspace layout of one corr_scores call (CorrWs: filled by
// corr_ws, corr.hip), what every stage of the call works on (CorrCtx: set up by umereg_corr_scores_ex_f32, corr.hip), and the launchers of
// the kernels, grouped by the unit that defines kernel AND launcher.  No kernel is declared here or anywhere else outside its definition:
// a launcher owns its kernel's grid, block and LDS arithmetic, and a unit reaches another unit's kernel only through it.
#pragma once
#include "corr_dev.h"

namespace umereg {

// ---- the workspace of one corr_scores call: routing and layout, decided in ONE place (corr_ws) -------------------------------
// Byte offsets of the regions in workspace order (sizes: the `take` lines of corr_ws; table: DESIGN 4.11).  A region that is switched off
// has no bytes.  The host takes every pointer from here (CorrCtx).  Three things outside corr_ws rely on an ADJACENCY:
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

// ---- one call: what every stage and every launcher below works on ------------------------------------------------------------
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
    int* gorder;                         // the global order: perm [M] | inv [M] | err [M] (only the fallback of the chunk orders: M > kChunkOrderMax)
    float4* centroid;                    // of the source's 64-point chunks
    unsigned int *b_surv, *b_vqmax;
    CellWs cw; FlatWs fw;
    template <class P> P* at(bool on, size_t off) const { return on ? reinterpret_cast<P*>(ws_src + off) : nullptr; }
};

// ---- launchers: UMEREG_OK, or UMEREG_ELAUNCH with the error set ---------------------------------------------------------------
// `second`: the second lattice build and cell pass of the arg-max mode (lattice_build_and_cell_pass, corr.hip).
// corr_knn.hip
int launch_chunk_box(char* ws, size_t ws_stride, int N, int batch, hipStream_t st);
// corr_consensus.hip
int launch_mean_rotation(const CorrCtx& c);
int launch_rotate_points(const CorrCtx& c, bool with_target_copies);
int launch_hyp_median(const CorrCtx& c);
int launch_hyp_err(const CorrCtx& c);
int launch_hyp_order(const CorrCtx& c);
int launch_chunk_centroid(const CorrCtx& c);
int launch_hyp_order_chunk(const CorrCtx& c);
int launch_corr_consensus(const CorrCtx& c);
int launch_corr_consensus2(const CorrCtx& c, float far_margin_cells, float act_frac);
// corr_lattice.hip
int launch_leftover_decide(const CorrCtx& c, unsigned int left_max);
int launch_bound_pass2_gate(const CorrCtx& c);
int launch_lattice_far_table(const CorrCtx& c);
int launch_lattice_mark_order(const CorrCtx& c, bool second);
int launch_lattice_mark(const CorrCtx& c);
int launch_lattice_compact(const CorrCtx& c);
int launch_lattice_posof(const CorrCtx& c);
int launch_lattice_list(const CorrCtx& c, bool second, bool full_grid);
int launch_cell_offsets(const CorrCtx& c);
int launch_cell_scatter(const CorrCtx& c, bool second);
int launch_corr_cell(const CorrCtx& c, bool second);
int launch_far_recompute(const CorrCtx& c);
// corr_leftover.hip
int launch_row_norm(const CorrCtx& c);
int launch_leftover_queue(const CorrCtx& c);
int launch_corr_score(const CorrCtx& c);
int launch_corr_score_record2(const CorrCtx& c);
int launch_leftover_flatten(const CorrCtx& c);
int launch_flat_bound(const CorrCtx& c, int mode);
int launch_corr_score_flat(const CorrCtx& c, int mode, bool bounding);
int launch_leftover_sum(const CorrCtx& c, bool second_pass);
int launch_corr_score_fallback(const CorrCtx& c);
int launch_bound_survivors(const CorrCtx& c);
int launch_corr_val_slices(const CorrCtx& c, bool last);
int launch_corr_reduce(const CorrCtx& c);

}  // namespace umereg
