// compact.h -- the two device functions of the ordered stream compaction that voxel.hip, sparse_map.hip, gt_match.hip,
// collate.hip and scan_prep.hip share (private; no kernel and no translation unit of its own).
//
// The scheme is three launches, each unit with kernels of its own around these two functions:
//   count    blocks of BLOCK rows, one thread per row: block_rank(keep).total -> bcnt[block]
//   scan     ONE block: scan_counts turns bcnt into the blocks' offsets (in place) and returns the number of kept rows
//   scatter  the same predicate again: a kept row goes to bcnt[block] + block_rank(keep).before
// Order comes from the scan, never from atomics: kept rows come out in ascending row index, the same in every run.
#pragma once
#include "common.h"

namespace umereg {

struct BlockRank {
    int before;     // kept threads of this block with a lower threadIdx.x
    int total;      // kept threads of this block
};

// Contract: EVERY thread of a block of exactly BLOCK threads (one-dimensional) calls this exactly once per kernel, from uniform
// control flow -- it holds a barrier, and a second call would overwrite wave counts that slower waves still read.  A whole block
// that returns before the call is uniform (fn_compact_kernel does); a thread without a row calls it with keep = false.
// One ballot per wave, the waves' counts through BLOCK / 64 ints of LDS, one barrier; the rank inside the wave is mbcnt's.
template <int BLOCK>
__device__ __forceinline__ BlockRank block_rank(bool keep)
{
    static_assert(BLOCK % kWave == 0 && BLOCK <= 1024, "whole waves of one workgroup");
    __shared__ int wave_cnt[BLOCK / kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < BLOCK / kWave; ++k) {
        const int c = wave_cnt[k];
        before += k < wave ? c : 0;
        total += c;
    }
    return {before + mbcnt(b), total};
}

// Exclusive scan of in[0 .. n) into out (and out2 unless null) by ONE block of exactly THREADS threads, all of which call it
// once from uniform control flow; returns the sum of in[0 .. n) to every thread.  `in` and `out` may be the same array (hence
// no __restrict__): a thread owns one contiguous slice and reads each element before it writes it.  Slices are
// ceil(n / THREADS) long, clamped to n at both ends: up to THREADS counts a thread owns one, beyond that several.
template <int THREADS>
__device__ __forceinline__ int scan_counts(const int* in, int* out, int* out2, int n)
{
    static_assert((THREADS & (THREADS - 1)) == 0 && THREADS <= 1024, "one workgroup");
    __shared__ int part[THREADS];
    const int per = (n + THREADS - 1) / THREADS;
    const int a = min((int)threadIdx.x * per, n), b = min(a + per, n);
    int s = 0;
    for (int k = a; k < b; ++k) s += in[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {      // Hillis-Steele, inclusive, over the threads' sums
        const int v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int k = a; k < b; ++k) {
        const int t = in[k];
        out[k] = run;
        if (out2) out2[k] = run;
        run += t;
    }
    return part[THREADS - 1];
}

}  // namespace umereg
