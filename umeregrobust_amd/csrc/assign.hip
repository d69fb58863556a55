// assign.hip -- the linear sum assignment of include/umereg_assign.h: an exact shortest-augmenting-path solver with fp64 duals
// over fp32 costs, for a batch of matrices read through a row stride and a batch stride.
//
//   init        row4col = col4row = -1, claim = INT_MAX, v = +inf (square) or 0 (n_rows < n_cols), status = 0, counters = 0
//   row_min     one workgroup per row: u[i] = min_j c[i][j]; a non-finite cost sets the matrix's status word (every writer
//               stores the same 1) and every later kernel returns at once for that matrix
//   col_min     square matrices only: v[j] = min_i (c[i][j] - u[i]).  The reduced costs are non-negative doubles, whose bit
//               patterns order like unsigned integers: a thread folds a chunk of rows in a register, the chunks meet in an
//               INTEGER atomicMin.  With n_rows < n_cols a column that stays free must keep v = 0, so v starts at 0 there.
//   first_zero  one workgroup per free row: the lowest free column of zero reduced cost -> zcol[i], atomicMin(claim[zcol], i)
//   commit      a row whose column's claim is its own index takes the column        (these two UMEREG_ASSIGN_START_ROUNDS times)
//   search      ONE workgroup of 1024 threads per matrix: the rows still free in ascending order (one ordered compaction at the
//               start; a search never frees a row), each by a Dijkstra search.  Thread t owns the columns t, t + 1024, ...: one
//               step is one coalesced read of cost row i against the owned columns' state, one arg-min over the workgroup
//               (lowest index on ties; a DPP butterfly per wave, the 16 wave results through LDS, ONE barrier per step on alternating
//               slots) and one look at row4col of the winner.  Then the duals of the visited rows and columns, the path flip
//               by thread 0, and at the very end the pairs and the total (wave 0, in row order).
//
// Where the per-column state lives: `shortest`, v, `pred`, `visited`, row4col and u go into the workgroup's dynamic LDS in
// this order, each as long as it still fits kAssignLdsBytes; what does not fit stays in the matrix's workspace slice (read and
// written by its owner thread only, so it sits in the CU's cache).  At n_cols = 1000 everything is in LDS, at 2500 all but
// row4col and u, at 10000 only `pred` and `visited` (nothing of eight bytes per column).
//
// Termination is structural: the outer loop runs over the compacted free rows (<= n_rows), the inner loop is counted to n_cols
// and each step marks one more column visited (if no finite candidate is left the arg-min's tie rule yields the lowest unvisited
// index), the path flip is counted to n_rows; every loop condition is uniform over the workgroup and comes out of a barrier.
#include <limits.h>

#include "common.h"
#include "umereg_assign.h"

namespace umereg {

constexpr int kAssignBlock = 256;             // start kernels
constexpr int kAssignSearchBlock = 1024;      // the search: one workgroup per matrix
constexpr int kAssignUnroll = 4;              // owned columns whose loads the search issues together
constexpr int kAssignColChunks = 512;         // at most this many row chunks in col_min
constexpr int kAssignLdsBytes = 60 * 1024;    // dynamic LDS of the search (64 KiB less its static slots)
constexpr int64_t kAssignMaxN = (int64_t)1 << 31;
constexpr int64_t kAssignMaxBatch = 65536;    // the batch is a grid's y (z) dimension

struct AssignWs {
    size_t off_stats, off_u, off_v, off_shortest, off_pred, off_row4col, off_claim, off_col4row, off_zcol, off_free, off_visited, total;
};

inline AssignWs assign_ws(int n_rows, int n_cols)
{
    AssignWs w;
    size_t o = 0;
    const size_t r = (size_t)n_rows, c = (size_t)n_cols;
    w.off_stats = o;    o += 256;
    w.off_u = o;        o += align_up(r * 8, 256);
    w.off_v = o;        o += align_up(c * 8, 256);
    w.off_shortest = o; o += align_up(c * 8, 256);
    w.off_pred = o;     o += align_up(c * 4, 256);
    w.off_row4col = o;  o += align_up(c * 4, 256);
    w.off_claim = o;    o += align_up(c * 4, 256);
    w.off_col4row = o;  o += align_up(r * 4, 256);
    w.off_zcol = o;     o += align_up(r * 4, 256);
    w.off_free = o;     o += align_up(r * 4, 256);
    w.off_visited = o;  o += align_up(c, 256);
    w.total = o;
    return w;
}

// byte offsets into the search's dynamic LDS; -1: the array stays in the workspace
struct AssignLds {
    int shortest, v, pred, visited, row4col, u, total;
};

inline AssignLds assign_lds(int n_rows, int n_cols)
{
    AssignLds l;
    size_t o = 0;
    const auto place = [&o](size_t bytes) {
        bytes = align_up(bytes, 16);
        if (o + bytes > (size_t)kAssignLdsBytes) return -1;
        const int at = (int)o;
        o += bytes;
        return at;
    };
    l.shortest = place((size_t)n_cols * 8);
    l.v = place((size_t)n_cols * 8);
    l.pred = place((size_t)n_cols * 4);
    l.visited = place((size_t)n_cols);
    l.row4col = place((size_t)n_cols * 4);
    l.u = place((size_t)n_rows * 8);
    l.total = (int)o;
    return l;
}

struct AssignArgs {
    const float* cost;
    int64_t row_stride, batch_stride;
    int n_rows, n_cols;
    int64_t* out_pairs;
    double* out_total;
    int* out_status;
    char* ws;
    size_t ws_stride;
    AssignWs w;
    AssignLds l;
};

__device__ __forceinline__ bool assign_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ double assign_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

__global__ __launch_bounds__(kAssignBlock) void assign_init_kernel(AssignArgs a, int square)
{
    const int64_t i = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    char* ws = a.ws + (size_t)blockIdx.y * a.ws_stride;
    if (i < a.n_cols) {
        reinterpret_cast<int*>(ws + a.w.off_row4col)[i] = -1;
        reinterpret_cast<int*>(ws + a.w.off_claim)[i] = INT_MAX;
        reinterpret_cast<double*>(ws + a.w.off_v)[i] = square ? assign_inf() : 0.0;
    }
    if (i < a.n_rows) reinterpret_cast<int*>(ws + a.w.off_col4row)[i] = -1;
    if (i < 2) reinterpret_cast<long long*>(ws + a.w.off_stats)[i] = 0;
    if (i == 0) a.out_status[blockIdx.y] = 0;
}

// u[i] = min_j c[i][j]; the matrix's status word is set if the row holds a NaN or an infinity
__global__ __launch_bounds__(kAssignBlock) void assign_row_min_kernel(AssignArgs a)
{
    __shared__ float s_min[kAssignBlock / kWave];
    const int i = blockIdx.x, b = blockIdx.y;
    const float* row = a.cost + (int64_t)b * a.batch_stride + (int64_t)i * a.row_stride;
    float m = __uint_as_float(0x7f800000u);
    bool bad = false;
    for (int j = threadIdx.x; j < a.n_cols; j += kAssignBlock) {
        const float x = row[j];
        bad |= assign_nonfinite(x);
        m = x < m ? x : m;
    }
    if (__any(bad) && lane_id() == 0) a.out_status[b] = 1;
    for (int off = 32; off; off >>= 1) {
        const float o = __shfl_xor(m, off, kWave);
        m = o < m ? o : m;
    }
    if (lane_id() == 0) s_min[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kAssignBlock / kWave; ++k) m = s_min[k] < m ? s_min[k] : m;
        reinterpret_cast<double*>(a.ws + (size_t)b * a.ws_stride + a.w.off_u)[i] = (double)m;
    }
}

// square matrices: v[j] = min_i (c[i][j] - u[i]); blockIdx.y = a chunk of rows_per rows, blockIdx.z = the matrix
__global__ __launch_bounds__(kAssignBlock) void assign_col_min_kernel(AssignArgs a, int rows_per)
{
    const int b = blockIdx.z;
    if (a.out_status[b]) return;
    const int j = blockIdx.x * kAssignBlock + threadIdx.x;
    if (j >= a.n_cols) return;
    char* ws = a.ws + (size_t)b * a.ws_stride;
    const double* u = reinterpret_cast<const double*>(ws + a.w.off_u);
    const int i0 = blockIdx.y * rows_per, i1 = min(i0 + rows_per, a.n_rows);
    const float* col = a.cost + (int64_t)b * a.batch_stride + j;
    double m = assign_inf();
    for (int i = i0; i < i1; ++i) {
        const double r = (double)col[(int64_t)i * a.row_stride] - u[i];      // >= +0: u[i] is the row's minimum
        m = r < m ? r : m;
    }
    // (fabs: -0.0f less +0.0 is -0.0, whose bit pattern would order last)
    if (i0 < i1) atomicMin(reinterpret_cast<unsigned long long*>(ws + a.w.off_v) + j, (unsigned long long)__double_as_longlong(fabs(m)));
}

// a free row names the lowest free column of zero reduced cost
__global__ __launch_bounds__(kAssignBlock) void assign_first_zero_kernel(AssignArgs a)
{
    __shared__ int s_min[kAssignBlock / kWave];
    const int i = blockIdx.x, b = blockIdx.y;
    if (a.out_status[b]) return;
    char* ws = a.ws + (size_t)b * a.ws_stride;
    int* zcol = reinterpret_cast<int*>(ws + a.w.off_zcol);
    if (reinterpret_cast<const int*>(ws + a.w.off_col4row)[i] >= 0) return;      // (uniform over the workgroup)
    const double* v = reinterpret_cast<const double*>(ws + a.w.off_v);
    const int* row4col = reinterpret_cast<const int*>(ws + a.w.off_row4col);
    const double u_i = reinterpret_cast<const double*>(ws + a.w.off_u)[i];
    const float* row = a.cost + (int64_t)b * a.batch_stride + (int64_t)i * a.row_stride;
    int z = INT_MAX;
    for (int j = threadIdx.x; j < a.n_cols; j += kAssignBlock)
        if (((double)row[j] - u_i) - v[j] == 0.0 && row4col[j] < 0) {
            z = j;
            break;
        }
    for (int off = 32; off; off >>= 1) z = min(z, __shfl_xor(z, off, kWave));
    if (lane_id() == 0) s_min[threadIdx.x >> 6] = z;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kAssignBlock / kWave; ++k) z = min(z, s_min[k]);
        zcol[i] = z;
        if (z != INT_MAX) atomicMin(reinterpret_cast<int*>(ws + a.w.off_claim) + z, i);
    }
}

// a column goes to the lowest row that named it
__global__ __launch_bounds__(kAssignBlock) void assign_commit_kernel(AssignArgs a)
{
    const int b = blockIdx.y;
    if (a.out_status[b]) return;
    const int64_t i = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (i >= a.n_rows) return;
    char* ws = a.ws + (size_t)b * a.ws_stride;
    int* col4row = reinterpret_cast<int*>(ws + a.w.off_col4row);
    if (col4row[i] >= 0) return;
    const int z = reinterpret_cast<const int*>(ws + a.w.off_zcol)[i];
    if (z == INT_MAX || reinterpret_cast<const int*>(ws + a.w.off_claim)[z] != (int)i) return;
    col4row[i] = z;
    reinterpret_cast<int*>(ws + a.w.off_row4col)[z] = (int)i;
}

struct AssignCand {
    double val;
    int idx;
};

__device__ __forceinline__ bool assign_before(const AssignCand& x, const AssignCand& y)
{
    return x.val < y.val || (x.val == y.val && x.idx < y.idx);
}

// one butterfly step of the arg-min over aligned groups of 32 lanes (common.h: partner32_*; valid for any idempotent, commutative
// fold whose operands are uniform over the lanes combined so far -- the order below is total, so they are)
template <int S>
__device__ __forceinline__ AssignCand assign_fold32(AssignCand c)
{
    const AssignCand o = {partner32_f64<S>(c.val), partner32_i32<S>(c.idx)};
    return assign_before(o, c) ? o : c;
}

// arg-min over the workgroup (least value, lowest index on ties), to every thread.  One barrier; `slot` alternates between calls,
// so a wave that runs ahead into the next call writes the other slot while a slower wave still reads this one.
__device__ __forceinline__ AssignCand assign_block_argmin(AssignCand c, double (*s_val)[kAssignSearchBlock / kWave],
                                                          int (*s_idx)[kAssignSearchBlock / kWave], int slot)
{
    c = assign_fold32<0>(c);
    c = assign_fold32<1>(c);
    c = assign_fold32<2>(c);
    c = assign_fold32<3>(c);
    c = assign_fold32<4>(c);
    const AssignCand o = {shfl_xor_f64(c.val, 32), __shfl_xor(c.idx, 32, kWave)};
    if (assign_before(o, c)) c = o;
    if (lane_id() == 0) {
        s_val[slot][threadIdx.x >> 6] = c.val;
        s_idx[slot][threadIdx.x >> 6] = c.idx;
    }
    __syncthreads();
    static_assert(kAssignSearchBlock / kWave == 16, "the second stage folds 16 wave results");
    c.val = s_val[slot][threadIdx.x & 15];
    c.idx = s_idx[slot][threadIdx.x & 15];
    c = assign_fold32<0>(c);
    c = assign_fold32<1>(c);
    c = assign_fold32<2>(c);
    c = assign_fold32<3>(c);
    return c;
}

__global__ __launch_bounds__(kAssignSearchBlock) void assign_search_kernel(AssignArgs a)
{
    constexpr int T = kAssignSearchBlock, W = kAssignSearchBlock / kWave;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ double s_val[2][W];
    __shared__ int s_idx[2][W];
    __shared__ int s_cnt[W];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_rows = a.n_rows, n_cols = a.n_cols;
    int64_t* pairs = a.out_pairs + (int64_t)b * n_rows * 2;
    if (a.out_status[b]) {                                              // (uniform: written by an earlier launch)
        for (int i = tid; i < n_rows; i += T) {
            pairs[2 * (int64_t)i] = i;
            pairs[2 * (int64_t)i + 1] = -1;
        }
        if (tid == 0 && a.out_total) a.out_total[b] = 0.0;
        return;
    }
    char* ws = a.ws + (size_t)b * a.ws_stride;
    const float* cost = a.cost + (int64_t)b * a.batch_stride;
    double* u_g = reinterpret_cast<double*>(ws + a.w.off_u);
    double* v_g = reinterpret_cast<double*>(ws + a.w.off_v);
    int* row4col_g = reinterpret_cast<int*>(ws + a.w.off_row4col);
    int* col4row = reinterpret_cast<int*>(ws + a.w.off_col4row);
    int* free_rows = reinterpret_cast<int*>(ws + a.w.off_free);
    double* shortest = a.l.shortest >= 0 ? reinterpret_cast<double*>(lds + a.l.shortest) : reinterpret_cast<double*>(ws + a.w.off_shortest);
    double* v = a.l.v >= 0 ? reinterpret_cast<double*>(lds + a.l.v) : v_g;
    int* pred = a.l.pred >= 0 ? reinterpret_cast<int*>(lds + a.l.pred) : reinterpret_cast<int*>(ws + a.w.off_pred);
    unsigned char* visited = a.l.visited >= 0 ? reinterpret_cast<unsigned char*>(lds + a.l.visited)
                                              : reinterpret_cast<unsigned char*>(ws + a.w.off_visited);
    int* row4col = a.l.row4col >= 0 ? reinterpret_cast<int*>(lds + a.l.row4col) : row4col_g;
    double* u = a.l.u >= 0 ? reinterpret_cast<double*>(lds + a.l.u) : u_g;
    const double inf = assign_inf();

    for (int j = tid; j < n_cols; j += T) {
        shortest[j] = inf;
        visited[j] = 0;
        if (a.l.v >= 0) v[j] = v_g[j];
        if (a.l.row4col >= 0) row4col[j] = row4col_g[j];
    }
    if (a.l.u >= 0)
        for (int i = tid; i < n_rows; i += T) u[i] = u_g[i];
    // the rows the start left free, ascending
    int n_free = 0;
    for (int r0 = 0; r0 < n_rows; r0 += T) {
        const int i = r0 + tid;
        const bool is_free = i < n_rows && col4row[i] < 0;
        const unsigned long long m = __ballot(is_free);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < W; ++k) {
            const int c = s_cnt[k];
            before += k < wave ? c : 0;
            total += c;
        }
        if (is_free) free_rows[n_free + before + mbcnt(m)] = i;
        n_free += total;
        __syncthreads();
    }

    long long steps = 0;
    int slot = 0;
    bool failed = false;
    for (int k = 0; k < n_free && !failed; ++k) {
        const int cur = free_rows[k];
        int i = cur, sink = -1;
        double u_i = u[i], min_val = 0.0;
        for (int cnt = 0; cnt < n_cols; ++cnt) {
            const float* row = cost + (int64_t)i * a.row_stride;
            AssignCand best = {inf, INT_MAX};
            // four owned columns at a time: every load first (index clamped, so none waits for `visited`), then the updates
            for (int j0 = tid; j0 < n_cols; j0 += kAssignUnroll * T) {
                float c_ij[kAssignUnroll];
                double v_j[kAssignUnroll], s_j[kAssignUnroll];
                bool open[kAssignUnroll];
#pragma unroll
                for (int q = 0; q < kAssignUnroll; ++q) {
                    const int j = min(j0 + q * T, n_cols - 1);
                    open[q] = j0 + q * T < n_cols && !visited[j];
                    c_ij[q] = row[j];
                    v_j[q] = v[j];
                    s_j[q] = shortest[j];
                }
#pragma unroll
                for (int q = 0; q < kAssignUnroll; ++q) {
                    if (!open[q]) continue;
                    const int j = j0 + q * T;
                    const double r = ((min_val + (double)c_ij[q]) - u_i) - v_j[q];
                    double s = s_j[q];
                    if (r < s) {
                        s = r;
                        shortest[j] = r;
                        pred[j] = i;
                    }
                    if (s < best.val || best.idx == INT_MAX) best = {s, j};    // (j ascends: the first of equal values stays)
                }
            }
            best = assign_block_argmin(best, s_val, s_idx, slot);
            slot ^= 1;
            ++steps;
            const int js = best.idx;
            if (js >= n_cols) break;                                            // no unvisited column: not while cnt < n_cols
            min_val = best.val;
            if ((js & (T - 1)) == tid) visited[js] = 1;
            const int r4c = row4col[js];
            if (r4c < 0) {
                sink = js;
                break;
            }
            i = r4c;
            u_i = u[i];
        }
        if (sink < 0) {                                                         // (cannot happen with finite costs)
            if (tid == 0) a.out_status[b] = 1;
            failed = true;
            continue;
        }
        // duals of the visited columns and of the rows they were matched to; the owned state back to "nothing seen"
        for (int j = tid; j < n_cols; j += T) {
            if (visited[j]) {
                const double d = min_val - shortest[j];
                v[j] = v[j] - d;
                if (j != sink) {
                    const int r = row4col[j];
                    u[r] = u[r] + d;
                }
                visited[j] = 0;
            }
            shortest[j] = inf;
        }
        if (tid == 0) u[cur] = u[cur] + min_val;
        __syncthreads();
        if (tid == 0) {                                                         // flip the path sink -> cur
            int j = sink;
            for (int g = 0; g < n_rows; ++g) {
                const int r = pred[j];
                row4col[j] = r;
                const int jn = col4row[r];
                col4row[r] = j;
                j = jn;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }

    // the pairs, and the chosen costs into `shortest` (n_rows <= n_cols) for the ordered sum
    __syncthreads();
    for (int i = tid; i < n_rows; i += T) {
        const int j = col4row[i];
        pairs[2 * (int64_t)i] = i;
        pairs[2 * (int64_t)i + 1] = j;
        shortest[i] = j >= 0 ? (double)cost[(int64_t)i * a.row_stride + j] : 0.0;
    }
    __syncthreads();
    if (wave == 0) {                                                            // row order: 64 loads at a time, added lane by lane
        double total = 0.0;
        for (int i0 = 0; i0 < n_rows; i0 += kWave) {
            const double x = i0 + lane < n_rows ? shortest[i0 + lane] : 0.0;
            const int n = min(kWave, n_rows - i0);
            for (int l = 0; l < n; ++l) total += shfl_f64(x, l);
        }
        if (lane == 0) {
            if (a.out_total) a.out_total[b] = failed ? 0.0 : total;
            long long* stats = reinterpret_cast<long long*>(ws + a.w.off_stats);
            stats[0] = n_rows - n_free;
            stats[1] = steps;
        }
    }
}

static bool assign_sizes_ok(int64_t batch, int64_t n_rows, int64_t n_cols)
{
    return batch > 0 && batch < kAssignMaxBatch && n_rows > 0 && n_rows <= n_cols && n_cols < kAssignMaxN;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_assign_workspace_bytes(int64_t batch, int64_t n_rows, int64_t n_cols)
{
    return assign_sizes_ok(batch, n_rows, n_cols) ? (size_t)batch * assign_ws((int)n_rows, (int)n_cols).total : 0;
}

UMEREG_API int umereg_linear_sum_assignment(const float* cost, int64_t batch, int64_t n_rows, int64_t n_cols, int64_t row_stride,
                                            int64_t batch_stride, int64_t* out_pairs, double* out_total, int* out_status,
                                            void* workspace, size_t workspace_bytes, void* stream)
{
    const char* who = "linear_sum_assignment";
    UMEREG_REQUIRE(assign_sizes_ok(batch, n_rows, n_cols),
                   "%s: needs 0 < n_rows <= n_cols < 2^31 and 0 < batch < 65536 (got batch %lld, %lld x %lld); solve the transpose of a tall matrix",
                   who, (long long)batch, (long long)n_rows, (long long)n_cols);
    UMEREG_REQUIRE(row_stride >= n_cols && batch_stride >= 0, "%s: row_stride must be at least n_cols and batch_stride not negative (got %lld, %lld)",
                   who, (long long)row_stride, (long long)batch_stride);
    UMEREG_REQUIRE(cost && out_pairs && out_status, "%s: null pointer (cost, out_pairs, out_status)", who);
    if (int rc = check_device()) return rc;
    AssignArgs a;
    a.w = assign_ws((int)n_rows, (int)n_cols);
    UMEREG_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, (size_t)batch * a.w.total);
    a.l = assign_lds((int)n_rows, (int)n_cols);
    a.cost = cost;
    a.row_stride = row_stride;
    a.batch_stride = batch_stride;
    a.n_rows = (int)n_rows;
    a.n_cols = (int)n_cols;
    a.out_pairs = out_pairs;
    a.out_total = out_total;
    a.out_status = out_status;
    a.ws = (char*)workspace;
    a.ws_stride = a.w.total;
    hipStream_t st = (hipStream_t)stream;
    const auto blocks = [](int64_t n) { return (unsigned)((n + kAssignBlock - 1) / kAssignBlock); };
    const unsigned nb = (unsigned)batch;
    const int square = n_rows == n_cols;
    hipLaunchKernelGGL(assign_init_kernel, dim3(blocks(n_cols), nb), dim3(kAssignBlock), 0, st, a, square);
    UMEREG_CHECK_LAUNCH("assign_init_kernel");
    hipLaunchKernelGGL(assign_row_min_kernel, dim3((unsigned)n_rows, nb), dim3(kAssignBlock), 0, st, a);
    UMEREG_CHECK_LAUNCH("assign_row_min_kernel");
    if (square) {
        const int64_t chunks = (n_rows + 31) / 32 < kAssignColChunks ? (n_rows + 31) / 32 : kAssignColChunks;
        const int rows_per = (int)((n_rows + chunks - 1) / chunks);
        hipLaunchKernelGGL(assign_col_min_kernel, dim3(blocks(n_cols), (unsigned)((n_rows + rows_per - 1) / rows_per), nb),
                           dim3(kAssignBlock), 0, st, a, rows_per);
        UMEREG_CHECK_LAUNCH("assign_col_min_kernel");
    }
    for (int round = 0; round < UMEREG_ASSIGN_START_ROUNDS; ++round) {
        hipLaunchKernelGGL(assign_first_zero_kernel, dim3((unsigned)n_rows, nb), dim3(kAssignBlock), 0, st, a);
        UMEREG_CHECK_LAUNCH("assign_first_zero_kernel");
        hipLaunchKernelGGL(assign_commit_kernel, dim3(blocks(n_rows), nb), dim3(kAssignBlock), 0, st, a);
        UMEREG_CHECK_LAUNCH("assign_commit_kernel");
    }
    hipLaunchKernelGGL(assign_search_kernel, dim3(nb), dim3(kAssignSearchBlock), (size_t)a.l.total, st, a);
    UMEREG_CHECK_LAUNCH("assign_search_kernel");
    return UMEREG_OK;
}
