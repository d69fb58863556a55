// pair_match.hip -- a1..a5 of one registration pair in one call, and the same chain as a hipGraph.  Host composition only:
// every kernel belongs to the unit whose entry launches it (grid.hip, ume_moments.hip, ortho.hip, match*.hip).
#include "common.h"
#include "ball_search.h"
#include "match_dev.h"

using namespace umereg;

// ---- a1..a5 of one registration pair in ONE call -----------------------------------------------------------------
// reference evaluate.py:206-236: UME matrices of both clouds, matching, match probabilities -- everything up to the
// host RNG draw.  Pure composition of the layered entry points (same kernels, same results); exists because a pair
// is ~12 launches and a Python caller pays ~10 us per ctypes call.
UMEREG_API size_t umereg_pair_match_workspace_bytes_ex(int N, int n_kp, const umereg_match_opts* opts)
{
    if (N <= 0 || n_kp <= 0) return 0;
    const size_t m = umereg_ume_match_workspace_bytes_ex(1, n_kp, n_kp, opts);
    // (+ the 64-byte device record of a ragged pair, umereg_pair_match_ragged_f32, behind everything else)
    return m ? align_up(umereg_ume_moments_workspace_bytes(2, N), 256) + align_up(m, 256) + 256 : 0;
}
UMEREG_API size_t umereg_pair_match_workspace_bytes(int N, int n_kp) { return umereg_pair_match_workspace_bytes_ex(N, n_kp, nullptr); }

UMEREG_API int umereg_pair_match_f32(const float* pts, const float* feat, const int64_t* kp_index, int N, int n_kp, int K,
                                     float radius, float tau, float* F, int64_t* match_idx, float* match_dist,
                                     float* prob, void* workspace, size_t workspace_bytes, void* stream)
{
    return umereg_pair_match_ex_f32(pts, feat, kp_index, N, n_kp, K, radius, tau, F, match_idx, match_dist, prob, workspace,
                                    workspace_bytes, nullptr, stream);
}

// The chain itself.  desc_vals == nullptr: the stacked form (pts [2,N,3], feat [2,N,32], kp_index [2,n_kp]).  Otherwise the
// clouds of a RAGGED pair (N = the capacity the workspace and the launches are sized for): the record at the tail of the
// workspace is written first -- by a kernel that takes the values as arguments, so that nothing on the host has to outlive the call
// -- and every kernel of a1/a2 reads its cloud through it.  write_desc = false: the chain only (a graph capture; the record is
// written outside the graph, before every replay).
static PairDesc* desc_of(void* workspace, size_t need) { return (PairDesc*)((char*)workspace + need - 256); }

static int write_pair_desc(PairDesc* dev, const PairDesc& v, hipStream_t st) { return write_record(dev, v, st); }

static int ragged_args(const PairDesc& v, int N_cap, int n_kp, const char* who)
{
    UMEREG_REQUIRE(v.pts[0] && v.pts[1] && v.feat[0] && v.feat[1] && v.kp[0] && v.kp[1], "%s: null cloud pointer", who);
    UMEREG_REQUIRE(v.n_pts[0] > 0 && v.n_pts[1] > 0 && v.n_pts[0] <= N_cap && v.n_pts[1] <= N_cap,
                   "%s: cloud sizes (%d, %d) must be in [1, capacity %d]", who, v.n_pts[0], v.n_pts[1], N_cap);
    UMEREG_REQUIRE(((uintptr_t)v.feat[0] & 15) == 0 && ((uintptr_t)v.feat[1] & 15) == 0 && ((uintptr_t)v.pts[0] & 3) == 0 &&
                   ((uintptr_t)v.pts[1] & 3) == 0 && ((uintptr_t)v.kp[0] & 7) == 0 && ((uintptr_t)v.kp[1] & 7) == 0,
                   "%s: misaligned cloud pointer (features: 16 bytes)", who);
    (void)n_kp;
    return UMEREG_OK;
}

static int pair_match_chain(const float* pts, const float* feat, const int64_t* kp_index, const PairDesc* desc_vals, bool write_desc,
                            bool ragged, int N, int n_kp, int K, float radius, float tau, float* F, int64_t* match_idx,
                            float* match_dist, float* prob, void* workspace, size_t workspace_bytes, const umereg_match_opts* opts,
                            void* stream, const char* who)
{
    MatchOpts mo;
    if (int rc = resolve_opts(opts, mo, who)) return rc;
    UMEREG_REQUIRE(F && match_idx && match_dist, "%s: null output pointer", who);
    UMEREG_REQUIRE(ragged || (pts && feat && kp_index), "%s: null pointer", who);
    UMEREG_REQUIRE(N > 0 && n_kp > 0, "%s: N, n_kp must be positive (got %d, %d)", who, N, n_kp);
    UMEREG_REQUIRE(K > 0 && K <= kMaxBallK, "%s: K must be in [1, 7680] (got %d)", who, K);
    UMEREG_REQUIRE(radius > 0.f, "%s: radius must be positive", who);
    UMEREG_REQUIRE(!prob || tau > 0.f, "%s: tau must be positive when prob is requested", who);
    UMEREG_REQUIRE(!ragged || n_kp <= grid_ws(N).Npad, "%s: n_kp (%d) exceeds the capacity's keypoint buffer (%d): the reference draws "
                   "min(10000, N_src, N_tgt) keypoints (evaluate.py:197)", who, n_kp, grid_ws(N).Npad);
    UMEREG_REQUIRE(((uintptr_t)F & 15) == 0 && (ragged || ((uintptr_t)feat & 15) == 0), "%s: feat and F must be 16-byte aligned", who);
    if (int rc = check_device()) return rc;
    const size_t need = umereg_pair_match_workspace_bytes_ex(N, n_kp, opts);
    UMEREG_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    char* ws_mom = (char*)workspace;
    const size_t mom_bytes = align_up(umereg_ume_moments_workspace_bytes(2, N), 256);
    char* ws_match = ws_mom + mom_bytes;
    const PairDesc* desc = ragged ? desc_of(workspace, need) : nullptr;
    if (ragged && write_desc) {
        if (int rc = ragged_args(*desc_vals, N, n_kp, who)) return rc;
        if (int rc = write_pair_desc(desc_of(workspace, need), *desc_vals, st)) return rc;
    }
    if (int rc = launch_prep(pts, ws_mom, 2, N, radius, st, 0, desc)) return rc;
    const bool ordered = keypoint_order_pays(N, n_kp);
    if (ordered)
        if (int rc = launch_query_order(ws_mom, nullptr, kp_index, 2, N, n_kp, radius, st, desc)) return rc;
    if (int rc = launch_moments(ws_mom, nullptr, kp_index, feat, 2, N, n_kp, K, radius, ordered ? UMEREG_MOMENTS_ORDERED : 0, F, nullptr,
                                nullptr, st, desc))
        return rc;
    // the matcher walks both clouds in the cell order the moment kernel just used (its early exit lives on neighbouring rows
    // sharing their good targets, match_f16r.hip); the f16 bases it fills are private to this workspace, the results are
    // keyed on the caller's keypoint indices either way
    const int* order1 = ordered ? (const int*)(ws_mom + grid_ws(N).off_kperm) : nullptr;
    const int* order2 = ordered ? (const int*)(ws_mom + grid_ws(N).total + grid_ws(N).off_kperm) : nullptr;
    if (int rc = match_f16r_ordered(F, F + (size_t)n_kp * 128, n_kp, n_kp, order1, order2, match_idx, match_dist, ws_match,
                                    need - 256 - mom_bytes, opts, stream))
        return rc;
    if (prob)
        if (int rc = umereg_match_prob_f32(match_dist, n_kp, tau, prob, stream)) return rc;
    return UMEREG_OK;
}

UMEREG_API int umereg_pair_match_ex_f32(const float* pts, const float* feat, const int64_t* kp_index, int N, int n_kp, int K,
                                        float radius, float tau, float* F, int64_t* match_idx, float* match_dist,
                                        float* prob, void* workspace, size_t workspace_bytes, const umereg_match_opts* opts,
                                        void* stream)
{
    return pair_match_chain(pts, feat, kp_index, nullptr, false, false, N, n_kp, K, radius, tau, F, match_idx, match_dist, prob, workspace,
                            workspace_bytes, opts, stream, "pair_match");
}

// ---- the same for a pair whose clouds DIFFER in size and live in separate buffers --------------------------------------------
// reference datasets/kitti/kitti_dataset.py:568-569 dilutes source and target independently; evaluate.py:195-204 draws
// min(10000, N_src, N_tgt) keypoints from each: n_kp is common to both clouds, N is not.
UMEREG_API int umereg_pair_match_ragged_f32(const float* src_pts, const float* tgt_pts, const float* src_feat, const float* tgt_feat,
                                            const int64_t* src_kp, const int64_t* tgt_kp, int N_src, int N_tgt, int n_kp, int K,
                                            float radius, float tau, float* F, int64_t* match_idx, float* match_dist, float* prob,
                                            void* workspace, size_t workspace_bytes, const umereg_match_opts* opts, void* stream)
{
    UMEREG_REQUIRE(N_src > 0 && N_tgt > 0, "pair_match_ragged: cloud sizes must be positive (got %d, %d)", N_src, N_tgt);
    const PairDesc v = {{src_pts, tgt_pts}, {src_feat, tgt_feat}, {src_kp, tgt_kp}, {N_src, N_tgt}, n_kp, 0};
    return pair_match_chain(nullptr, nullptr, nullptr, &v, true, true, N_src > N_tgt ? N_src : N_tgt, n_kp, K, radius, tau, F, match_idx,
                            match_dist, prob, workspace, workspace_bytes, opts, stream, "pair_match_ragged");
}

// ---- the same as ONE hipGraph -------------------------------------------------------------------------------------
// a1..a5 of a pair is a chain of 12 dependent launches (2 memsets, pack, cell histogram / scan / scatter, keypoint
// order, moments, bases, coarse filter, refine, softmax): ~0.10 ms of host time to enqueue, against ~0.30 ms of GPU
// time per pair.  For a caller that processes many pairs out of the same buffers (an evaluation loop with resident or
// double-buffered inputs) the chain is captured once and replayed with a single launch.  The handle owns nothing but
// the executable graph: buffers stay the caller's and must stay where they were at capture time.
struct PairMatchGraph {
    hipGraph_t graph;
    hipGraphExec_t exec;
    const float* F;            // [2, n_kp, 32, 4]: the captured chain's outputs, for the fused continuation below
    const int64_t* match_idx;
    const float* prob;
    int n_kp;
    // the input buffers the chain was captured over (umereg_pair_match_graph_launch_from refills them)
    float* pts;                // [2, N, 3]
    float* feat;               // [2, N, 32]
    int64_t* kp_index;         // [2, n_kp]
    int N;
    PairDesc* desc;            // capacity form (umereg_pair_match_graph_create_cap): the record the captured kernels read; else NULL
};

// Capture what `enqueue` puts on `stream` and instantiate it.  A chain that refuses its arguments ends the capture and
// reports its own error; nothing is left behind on any failure.
template <class Enqueue>
static int capture_chain(void* stream, const char* who, Enqueue enqueue, hipGraph_t* graph, hipGraphExec_t* exec)
{
    UMEREG_REQUIRE(stream, "%s: capture needs a non-default stream", who);
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: hipStreamBeginCapture failed", who);
        return UMEREG_ELAUNCH;
    }
    const int rc = enqueue();
    *graph = nullptr;
    const hipError_t e_end = hipStreamEndCapture(st, graph);
    if (rc != UMEREG_OK) { if (*graph) (void)hipGraphDestroy(*graph); return rc; }
    if (e_end != hipSuccess || !*graph) {
        (void)hipGetLastError();
        set_error("%s: hipStreamEndCapture failed (%s)", who, hipGetErrorString(e_end));
        return UMEREG_ELAUNCH;
    }
    *exec = nullptr;
    const hipError_t e_inst = hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0);
    if (e_inst != hipSuccess || !*exec) {
        (void)hipGraphDestroy(*graph);
        (void)hipGetLastError();
        set_error("%s: hipGraphInstantiate failed (%s)", who, hipGetErrorString(e_inst));
        return UMEREG_ELAUNCH;
    }
    return UMEREG_OK;
}

// what = which copy, as the message names it: "(prob)", "(cond)", " (device to device)"
static int copy_async(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, void* stream, const char* who, const char* what)
{
    if (hipMemcpyAsync(dst, src, bytes, kind, (hipStream_t)stream) == hipSuccess) return UMEREG_OK;
    (void)hipGetLastError();
    set_error("%s: hipMemcpyAsync%s failed", who, what);
    return UMEREG_ELAUNCH;
}

// Replay + (prob_host non-NULL) the device -> host copy of the match probabilities, the operand of the host draw (evaluate.py:238).
static int replay(const PairMatchGraph* h, float* prob_host, void* stream, const char* who)
{
    const hipError_t e = hipGraphLaunch(h->exec, (hipStream_t)stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: hipGraphLaunch failed (%s)", who, hipGetErrorString(e));
        return UMEREG_ELAUNCH;
    }
    if (prob_host && h->prob) return copy_async(prob_host, h->prob, (size_t)h->n_kp * sizeof(float), hipMemcpyDeviceToHost, stream, who, "(prob)");
    return UMEREG_OK;
}

UMEREG_API int umereg_pair_match_graph_create(const float* pts, const float* feat, const int64_t* kp_index, int N, int n_kp, int K,
                                              float radius, float tau, float* F, int64_t* match_idx, float* match_dist,
                                              float* prob, void* workspace, size_t workspace_bytes, void* stream, void** graph_out)
{
    return umereg_pair_match_graph_create_ex(pts, feat, kp_index, N, n_kp, K, radius, tau, F, match_idx, match_dist, prob, workspace,
                                             workspace_bytes, nullptr, stream, graph_out);
}

UMEREG_API int umereg_pair_match_graph_create_ex(const float* pts, const float* feat, const int64_t* kp_index, int N, int n_kp, int K,
                                                 float radius, float tau, float* F, int64_t* match_idx, float* match_dist,
                                                 float* prob, void* workspace, size_t workspace_bytes,
                                                 const umereg_match_opts* opts, void* stream, void** graph_out)
{
    UMEREG_REQUIRE(graph_out, "pair_match_graph_create: null graph_out");
    *graph_out = nullptr;
    hipGraph_t g; hipGraphExec_t ex;
    if (int rc = capture_chain(stream, "pair_match_graph_create", [&] {
            return umereg_pair_match_ex_f32(pts, feat, kp_index, N, n_kp, K, radius, tau, F, match_idx, match_dist, prob, workspace,
                                            workspace_bytes, opts, stream);
        }, &g, &ex))
        return rc;
    *graph_out = new PairMatchGraph{g, ex, F, match_idx, prob, n_kp, (float*)pts, (float*)feat, (int64_t*)kp_index, N, nullptr};
    return UMEREG_OK;
}

// ---- ONE graph for every pair that fits a capacity -------------------------------------------------------------------------------
// The chain captured with its kernels reading the clouds through the device record at the tail of the workspace (PairDesc, grid.h):
// a replay for a NEW pair -- other buffers, other N_src / N_tgt -- is umereg_pair_match_graph_launch_ragged: one 64-byte record
// written by a one-thread kernel, then the replay.  No staging copy, no re-capture; what stays baked in is the capacity (every
// cloud must have <= N_cap points), the keypoint count n_kp (= min(10000, N_src, N_tgt) at evaluate.py:197: 10 000 for every pair of
// the KITTI benchmarks) and K, radius, tau, the options.
UMEREG_API int umereg_pair_match_graph_create_cap(int N_cap, int n_kp, int K, float radius, float tau, float* F, int64_t* match_idx,
                                                  float* match_dist, float* prob, void* workspace, size_t workspace_bytes,
                                                  const umereg_match_opts* opts, void* stream, void** graph_out)
{
    UMEREG_REQUIRE(graph_out, "pair_match_graph_create_cap: null graph_out");
    *graph_out = nullptr;
    hipGraph_t g; hipGraphExec_t ex;
    if (int rc = capture_chain(stream, "pair_match_graph_create_cap", [&] {
            return pair_match_chain(nullptr, nullptr, nullptr, nullptr, false, true, N_cap, n_kp, K, radius, tau, F, match_idx, match_dist,
                                    prob, workspace, workspace_bytes, opts, stream, "pair_match_graph_create_cap");
        }, &g, &ex))
        return rc;
    PairDesc* desc = desc_of(workspace, umereg_pair_match_workspace_bytes_ex(N_cap, n_kp, opts));
    *graph_out = new PairMatchGraph{g, ex, F, match_idx, prob, n_kp, nullptr, nullptr, nullptr, N_cap, desc};
    return UMEREG_OK;
}

UMEREG_API int umereg_pair_match_graph_launch_ragged(void* graph, const float* src_pts, const float* tgt_pts, const float* src_feat,
                                                     const float* tgt_feat, const int64_t* src_kp, const int64_t* tgt_kp, int N_src,
                                                     int N_tgt, float* prob_host, void* stream)
{
    UMEREG_REQUIRE(graph, "pair_match_graph_launch_ragged: null graph");
    PairMatchGraph* h = (PairMatchGraph*)graph;
    UMEREG_REQUIRE(h->desc, "pair_match_graph_launch_ragged: this graph was captured over fixed buffers (umereg_pair_match_graph_create), "
                            "not at a capacity");
    const PairDesc v = {{src_pts, tgt_pts}, {src_feat, tgt_feat}, {src_kp, tgt_kp}, {N_src, N_tgt}, h->n_kp, 0};
    if (int rc = ragged_args(v, h->N, h->n_kp, "pair_match_graph_launch_ragged")) return rc;
    if (int rc = write_pair_desc(h->desc, v, (hipStream_t)stream)) return rc;
    return replay(h, prob_host, stream, "pair_match_graph_launch_ragged");
}

// A handle over fixed buffers.  A plain replay of a capacity graph would run kernels that read a record nobody wrote for it:
// refused here, before anything is launched.
static int fixed_graph(const void* graph, const char* who)
{
    UMEREG_REQUIRE(graph, "%s: null graph", who);
    UMEREG_REQUIRE(!((const PairMatchGraph*)graph)->desc, "%s: this graph was captured at a capacity: use umereg_pair_match_graph_launch_ragged", who);
    return UMEREG_OK;
}

UMEREG_API int umereg_pair_match_graph_launch(void* graph, void* stream)
{
    if (int rc = fixed_graph(graph, "pair_match_graph_launch")) return rc;
    return replay((PairMatchGraph*)graph, nullptr, stream, "pair_match_graph_launch");
}

UMEREG_API int umereg_pair_match_graph_launch_ex(void* graph, float* prob_host, void* stream)
{
    if (int rc = fixed_graph(graph, "pair_match_graph_launch_ex")) return rc;
    return replay((PairMatchGraph*)graph, prob_host, stream, "pair_match_graph_launch_ex");
}

// Replay for ANOTHER pair of the same shape (an evaluation loop over distinct pairs, reference evaluate.py:175): the new pair's
// inputs are copied device to device into the buffers the chain was captured over (14 MB at KITTI size: ~5 us of HBM time), then
// the graph is replayed and the probabilities are downloaded -- one call, no re-capture.  The capture buffers must be the
// caller's to overwrite (a pipeline slot's persistent staging buffers), and as with every replay launches of one handle must not
// overlap.  A source pointer equal to the captured one is skipped (NULL = that input is already in place).
UMEREG_API int umereg_pair_match_graph_launch_from(void* graph, const float* pts, const float* feat, const int64_t* kp_index,
                                                   float* prob_host, void* stream)
{
    if (int rc = fixed_graph(graph, "pair_match_graph_launch_from")) return rc;
    PairMatchGraph* h = (PairMatchGraph*)graph;
    const struct { const void* src; void* dst; size_t bytes; } cp[3] = {
        {pts, h->pts, (size_t)2 * h->N * 3 * sizeof(float)},
        {feat, h->feat, (size_t)2 * h->N * UMEREG_FEAT_DIM * sizeof(float)},
        {kp_index, h->kp_index, (size_t)2 * h->n_kp * sizeof(int64_t)}};
    for (const auto& c : cp) {
        if (!c.src || c.src == c.dst) continue;
        if (int rc = copy_async(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, stream, "pair_match_graph_launch_from", " (device to device)"))
            return rc;
    }
    return replay(h, prob_host, stream, "pair_match_graph_launch_from");
}

// The continuation after the host draw (evaluate.py:238-254): upload the kept match indices and solve one SE(3) per kept
// match from the graph's own outputs -- T[k] from (F_src[cond[k]], F_tgt[match[cond[k]]]).  cond_host NULL: every match.
//   cond_host int64 [n_cond] (pinned host memory for an asynchronous copy), cond_dev int64 [n_cond] and T_out f32
//   [n_cond, 4, 4] device buffers of the caller.
UMEREG_API int umereg_pair_match_graph_solve(void* graph, const int64_t* cond_host, int n_cond, int64_t* cond_dev, float* T_out,
                                             void* stream)
{
    UMEREG_REQUIRE(graph && T_out, "pair_match_graph_solve: null pointer");
    PairMatchGraph* h = (PairMatchGraph*)graph;
    const float* Fs = h->F;
    const float* Ft = h->F + (size_t)h->n_kp * 128;
    if (!cond_host)
        return umereg_rtume_solve_f32(Fs, Ft, nullptr, nullptr, h->match_idx, h->n_kp, h->n_kp, h->n_kp, T_out, nullptr, stream);
    UMEREG_REQUIRE(cond_dev && n_cond > 0 && n_cond <= h->n_kp, "pair_match_graph_solve: bad cond buffers / count (%d)", n_cond);
    if (int rc = copy_async(cond_dev, cond_host, (size_t)n_cond * sizeof(int64_t), hipMemcpyHostToDevice, stream, "pair_match_graph_solve", "(cond)"))
        return rc;
    return umereg_rtume_solve_f32(Fs, Ft, cond_dev, nullptr, h->match_idx, h->n_kp, h->n_kp, n_cond, T_out, nullptr, stream);
}

UMEREG_API int umereg_pair_match_graph_destroy(void* graph)
{
    if (!graph) return UMEREG_OK;
    PairMatchGraph* h = (PairMatchGraph*)graph;
    (void)hipGraphExecDestroy(h->exec);
    (void)hipGraphDestroy(h->graph);
    delete h;
    return UMEREG_OK;
}
