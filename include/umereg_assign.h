/* umereg_assign.h -- C ABI of the linear sum assignment on the device: what scipy.optimize.linear_sum_assignment does for the
 * reference on the host (utils/eval_utils.py:40-47, evaluate.py:216-222), as an exact solver in HIP kernels, for a batch of
 * fp32 cost matrices read where they lie.
 *
 * Same conventions as umereg.h: outputs and workspace belong to the caller, the compute entry takes a HIP stream (NULL = the
 * default stream), returns UMEREG_OK or a negative UMEREG_E* code, reports argument errors before it probes for a device, returns
 * UMEREG_ENODEV where no HIP device is visible, allocates nothing and never waits for the device.  The size query is host
 * arithmetic and returns 0 for arguments the compute entry would refuse.  The entry points here are typed by their own table
 * (umeregrobust_amd/assign.py: ASSIGN_SIGNATURES).
 *
 * The scheme is the shortest augmenting path method with fp64 duals over the fp32 costs:
 *   start    u[i] = min_j c[i][j];  for a SQUARE matrix v[j] = min_i (c[i][j] - u[i]), for n_rows < n_cols v = 0 (a column that
 *            stays free must keep a zero dual);  then UMEREG_ASSIGN_START_ROUNDS rounds of: every free row names the lowest free
 *            column j with (c[i][j] - u[i]) - v[j] == 0, a column takes the lowest row that named it (integer atomicMin).
 *   search   the rows still free, in ascending order, each by one Dijkstra search over the reduced costs
 *            (min_val + c[i][j]) - u[i] - v[j]; the unvisited column of least distance is taken next, the lowest index on ties;
 *            the search ends at the first free column; duals and matching are updated along the path.
 * Every minimum is order-independent and every sum runs in one fixed order: there is no floating-point atomic, no workspace word
 * is read that the same call did not write, and two runs give the same bytes whatever the workspace held.  Every loop is bounded
 * by a count (rows, columns), not by a numerical condition: a matrix with a NaN or an infinite cost gets status 1 from the first
 * pass and is not searched. */
#ifndef UMEREG_ASSIGN_H
#define UMEREG_ASSIGN_H

#include <stddef.h>
#include <stdint.h>

#include "umereg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UMEREG_ASSIGN_START_ROUNDS 2

/* workspace of one umereg_linear_sum_assignment call; 16-byte aligned memory.  0 unless 0 < n_rows <= n_cols < 2^31 and
 * 0 < batch < 65536.  It is batch equal slices (workspace_bytes(1, n_rows, n_cols) each); after the call a slice begins with
 * int64 {rows matched by the start, Dijkstra steps taken by the search}, for whoever measures. */
size_t umereg_assign_workspace_bytes(int64_t batch, int64_t n_rows, int64_t n_cols);

/* cost        f32 device memory: c[b][i][j] = cost[b * batch_stride + i * row_stride + j]; row_stride >= n_cols, batch_stride >= 0
 *             (in elements)
 * out_pairs   i64 [batch][n_rows][2] = (row, column), rows ascending
 * out_total   f64 [batch]: the chosen costs, widened to fp64, summed in row order; NULL allowed
 * out_status  i32 [batch]: 0, or 1 for a matrix with a non-finite cost, whose pairs are then (row, -1) and whose total is 0 */
int umereg_linear_sum_assignment(const float* cost, int64_t batch, int64_t n_rows, int64_t n_cols, int64_t row_stride,
                                 int64_t batch_stride, int64_t* out_pairs, double* out_total, int* out_status, void* workspace,
                                 size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
