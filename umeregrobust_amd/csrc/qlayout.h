// qlayout.h -- MFMA fragment orders of the orthonormal bases, shared by ortho.hip (writer) and
// ume_dist.hip / match_f16r.hip (readers).  Not part of the C ABI.
#pragma once
#include "common.h"

namespace umereg {

// Fragment orders (see ume_dist.hip).  k = feature channel 0..31, split as
// h = k>>4 (which half of the wave feeds it to v_mfma_f32_32x32x2_f32), kk4 = (k>>2)&3, e = k&3.
//   ROWS: source keypoint i, basis column a -> MFMA row 4*(i&7)+a of tile i>>3
//         float offset = (((i>>3)*4 + kk4)*64 + h*32 + (i&7)*4 + a)*4 + e
//   COLS: target keypoint j, basis column b -> MFMA column j&31 of tile (j>>5, b)
//         float offset = ((((j>>5)*4 + b)*4 + kk4)*64 + h*32 + (j&31))*4 + e
__device__ __forceinline__ size_t qoff_rows(int i, int a, int k)
{
    const int h = k >> 4, kk4 = (k >> 2) & 3, e = k & 3;
    return ((((size_t)(i >> 3) * 4 + kk4) * 64) + h * 32 + (i & 7) * 4 + a) * 4 + e;
}
__device__ __forceinline__ size_t qoff_cols(int j, int b, int k)
{
    const int h = k >> 4, kk4 = (k >> 2) & 3, e = k & 3;
    return (((((size_t)(j >> 5) * 4 + b) * 4 + kk4) * 64) + h * 32 + (j & 31)) * 4 + e;
}

// split-f16 fragment orders (ume_dist.hip, ume_dist_h_kernel; match_f16r.hip).  v_mfma_f32_32x32x16_f16 takes
// 8 halfs per lane: lane l feeds row/col (l&31) with k-block (l>>5).  Channel k is split as
// s = k>>4 (which of the two K=16 MFMA steps), h = (k>>3)&1 (lane half), e = k&7.
//   ROWS_F16X2: half offset = ((((i>>3)*2 + s)*2 + plane)*64 + h*32 + (i&7)*4 + a)*8 + e
//   COLS_F16X2: half offset = (((((j>>5)*4 + b)*2 + s)*2 + plane)*64 + h*32 + (j&31))*8 + e
// plane 0 = hi = f16(q), plane 1 = lo = f16(q - hi)  (|q| <= 1: lo's absolute error <= 2^-25).
__device__ __forceinline__ size_t hoff_rows(int i, int a, int k, int plane)
{
    const int s = k >> 4, h = (k >> 3) & 1, e = k & 7;
    return (((((size_t)(i >> 3) * 2 + s) * 2 + plane) * 64) + h * 32 + (i & 7) * 4 + a) * 8 + e;
}
__device__ __forceinline__ size_t hoff_cols(int j, int b, int k, int plane)
{
    const int s = k >> 4, h = (k >> 3) & 1, e = k & 7;
    return ((((((size_t)(j >> 5) * 4 + b) * 2 + s) * 2 + plane) * 64) + h * 32 + (j & 31)) * 8 + e;
}

// ---- slot order of a matching problem whose keypoints come with a processing order (the pair chain, pair_match.hip) ----
// order[p] = the keypoint at position p of the cell-sorted order (kp_order_kernel).  Source slot s holds keypoint order1[s].
// Target slot s holds keypoint order2[target_slot_pos(s, n)]: the first ceil(n / kSubStride) slots are a spatially uniform
// subsample (every kSubStride-th position), the other positions follow in order.  After the subsample's tiles every source
// row has met a target from its own neighbourhood, so its limit is close to the final one when the bulk begins (the early
// exit of ume_coarse_h_kernel lives on that).  A bijection of [0, n) onto itself for every n >= 1.
#ifndef UMEREG_SUB_STRIDE
#define UMEREG_SUB_STRIDE 8   // (16 for an A/B: half the subsample)
#endif
constexpr int kSubStride = UMEREG_SUB_STRIDE;
__host__ __device__ inline int target_slot_pos(int s, int n)
{
    const int n_sub = (n + kSubStride - 1) / kSubStride;
    if (s < n_sub) return s * kSubStride;
    const int r = s - n_sub;
    return r + r / (kSubStride - 1) + 1;
}

}  // namespace umereg
