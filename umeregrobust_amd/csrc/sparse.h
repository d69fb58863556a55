// sparse.h -- coordinate maps of the sparse feature network (sparse_map.hip builds them; featnet.hip, sparse_conv_pairs.hip and
// sparse_wgrad.hip convolve over them): the workspace carve-up with its check and its table pointers, the coordinate key, the
// kernel-offset table, and the argument record of the convolution kernels of both engines.  Not part of the C ABI.
//
// MinkowskiEngine 0.5.4 semantics restated here (parity unpinned):
//   * strided output map: unique(floor(c / (ts s)) ts s) per axis, batch index kept (fn_coarsen);
//   * kernel offsets {-1,0,1} ts_in per axis, index k = (dx+1) + 3(dy+1) + 9(dz+1), x fastest (fn_offset);
//   * convolution: out[o] = sum_k in[o + off_k(ts_in)] @ W[k]; transposed convolution onto the finer encoder map:
//     out[f] = sum_k in[f - off_k(ts_out)] @ W[k] -- both as gathers through one neighbour table per (output map, input map).
#pragma once
#include "common.h"
#include "umereg_featnet.h"

namespace umereg {

constexpr int kFnLevels = 5;                 // tensor strides 1, 2, 4, 8, 24
constexpr int kFnTables = kFnLevels + 1;     // one hash table per level + the locality cells
constexpr int kFnSortTable = kFnLevels;
constexpr int kFnCellStride = 8;             // locality cells of the level-0 row order: 8^3 voxels (<= 512 points per cloud)
constexpr int kFnVol = 27;
constexpr int kFnMaps = 13;                  // 5 self maps, 4 strided (l -> l+1), 4 transposed (l+1 -> l)
constexpr int kFnCoordLim = 1 << 17;         // accepted input coordinates: [-2^17, 2^17)
constexpr int kFnKeyBias = 1 << 18;          // key coordinates (inputs +- one coarse cell): [-2^18, 2^18), 19 bits
constexpr int kFnScanBlock = 1024;
constexpr unsigned long long kFnEmpty = ~0ull;

__host__ __device__ constexpr int fn_tstride(int l) { return l == 0 ? 1 : l == 1 ? 2 : l == 2 ? 4 : l == 3 ? 8 : 24; }
// map indices: self l, strided l -> l+1, transposed l+1 -> l
__host__ __device__ constexpr int fn_map_self(int l) { return l; }
__host__ __device__ constexpr int fn_map_down(int l) { return kFnLevels + l; }
__host__ __device__ constexpr int fn_map_up(int l) { return kFnLevels + 4 + l; }
// the level whose rows a map's table has one row for (its outputs)
__host__ __device__ constexpr int fn_map_out_level(int m) { return m < kFnLevels ? m : m < kFnLevels + 4 ? m - kFnLevels + 1 : m - kFnLevels - 4; }

// THE kernel-offset table (assumed to be MinkowskiEngine's hypercube order): k = (dx+1) + 3(dy+1) + 9(dz+1)
__host__ __device__ inline void fn_offset(int k, int& dx, int& dy, int& dz)
{
    dx = k % 3 - 1;
    dy = (k / 3) % 3 - 1;
    dz = k / 9 - 1;
}

// THE strided output coordinate: floor(c / t) t (floor, not truncation: KITTI voxel coordinates are negative too)
__host__ __device__ inline int fn_coarsen(int c, int t)
{
    const int q = c / t;
    return (q * t != c && c < 0 ? q - 1 : q) * t;
}

// (batch 7 bits | x, y, z 19 bits each, biased); batch <= 126 keeps every key != kFnEmpty
__device__ __forceinline__ bool fn_key(int b, int x, int y, int z, unsigned long long& key)
{
    if (x < -kFnKeyBias || x >= kFnKeyBias || y < -kFnKeyBias || y >= kFnKeyBias || z < -kFnKeyBias || z >= kFnKeyBias) return false;
    key = ((unsigned long long)b << 57) | ((unsigned long long)(x + kFnKeyBias) << 38) | ((unsigned long long)(y + kFnKeyBias) << 19) |
          (unsigned long long)(z + kFnKeyBias);
    return true;
}

__device__ __forceinline__ unsigned int fn_hash(unsigned long long key, unsigned int cap)
{
    return (unsigned int)((key * 0x9E3779B97F4A7C15ull) >> 32) & (cap - 1u);
}

struct FnWs {
    unsigned int cap;       // slots per hash table (power of two, >= 2 n)
    int n, nblk;
    size_t off_keys, off_min, ones_end;         // [kFnTables][cap] u64 keys, u32 first rows: all ones before a pass
    size_t off_cnt, off_mask, zero_end;         // [n] points per locality cell, [kFnMaps][n] offset masks: zero before a pass
    size_t off_row, off_slot, off_flag, off_newid, off_bcnt, off_start, off_cursor, off_tmp, off_perm;
    size_t off_coords;                          // [kFnLevels][n] int4 (batch, x, y, z)
    size_t off_nbr;                             // [kFnMaps][n][27] neighbour rows (-1: none)
    size_t off_x, off_s4, off_cat[4];           // features (every level has at most n rows)
    size_t total;
};

constexpr int kFnCatCols[4] = {96, 128, 192, 256};     // [decoder | encoder] channels of levels 0..3
constexpr int kFnCatTr[4] = {64, 64, 128, 128};        // the decoder block's share (first columns)

inline FnWs fn_ws(int n)
{
    FnWs w;
    unsigned int cap = 1024u;
    while (cap < 2u * (unsigned int)n) cap <<= 1;
    w.cap = cap;
    w.n = n;
    w.nblk = (n + kFnScanBlock - 1) / kFnScanBlock;
    const size_t N = (size_t)n;
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o = align_up(o + bytes, 256); return at; };
    w.off_keys = take((size_t)kFnTables * cap * 8);
    w.off_min = take((size_t)kFnTables * cap * 4);
    w.ones_end = o;
    w.off_cnt = take(N * 4);
    w.off_mask = take((size_t)kFnMaps * N * 4);
    w.zero_end = o;
    w.off_row = take((size_t)kFnTables * cap * 4);
    w.off_slot = take(N * 4);
    w.off_flag = take(N * 4);
    w.off_newid = take(N * 4);
    w.off_bcnt = take(((size_t)w.nblk + 1) * 4);
    w.off_start = take(N * 4);
    w.off_cursor = take(N * 4);
    w.off_tmp = take(N * 4);
    w.off_perm = take(N * 4);
    w.off_coords = take((size_t)kFnLevels * N * 16);
    w.off_nbr = take((size_t)kFnMaps * N * kFnVol * 4);
    w.off_x = take(N * 256 * 4);
    w.off_s4 = take(N * 256 * 4);
    for (int l = 0; l < 4; ++l) w.off_cat[l] = take(N * kFnCatCols[l] * 4);
    w.total = o;
    return w;
}

// neighbour table `table` of a workspace as the convolution kernels take it; -1: no table (a 1x1 layer over level 0)
struct FnTable {
    const int* nbr;             // [rows][27]
    const unsigned int* mask;   // [rows]
    int level;                  // the level of its output rows: their count is status[1 + level]
};

inline FnTable fn_table(const void* ws, const FnWs& w, int table)
{
    if (table < 0) return {nullptr, nullptr, 0};
    const char* p = (const char*)ws;
    return {reinterpret_cast<const int*>(p + w.off_nbr) + (size_t)table * w.n * kFnVol,
            reinterpret_cast<const unsigned int*>(p + w.off_mask) + (size_t)table * w.n, fn_map_out_level(table)};
}

// the caller's workspace of an n-point pass: there, at least fn_ws(n).total bytes and 256-byte aligned, or UMEREG_EWORKSPACE
inline int fn_check_ws(const char* who, const void* ws, size_t bytes, int n)
{
    const size_t need = fn_ws(n).total;
    if (ws && bytes >= need && ((uintptr_t)ws & 255) == 0) return UMEREG_OK;
    set_error("%s: workspace too small or not 256-byte aligned (%zu < %zu)", who, bytes, need);
    return UMEREG_EWORKSPACE;
}

// one convolution launch as the kernels of featnet.hip (the "union" engine) and of sparse_conv_pairs.hip (the "pairs" engine) take it
struct ConvArgs {
    const float* in;        // input rows (already offset to the first input column)
    const float* W;         // [K][cin][cout]
    const float* scale;
    const float* shift;
    const float* res;       // residual rows [., ld_res] or null
    float* out;             // output rows (already offset to the first output column)
    const int* nbr;         // [rows][27] or null (K = 1: output row o reads input row o)
    const unsigned int* mask;
    const int32_t* n_out;   // output rows (device)
    int ld_in, ld_res, ld_out, cin, cout, K, relu;
};

struct ConvArgsF16 {
    ConvArgs c;
    int32_t* range;         // status word that takes UMEREG_FN_ERR_F16_RANGE when a stored value is not within +-65504 (or null)
};

// a 27-offset layer on the pair-compacted engine (sparse_conv_pairs.hip; include/umereg_sparse_conv_pairs.h) over at most
// `rows_bound` output rows; `range` as ConvArgsF16
int fn_launch_conv_pairs(const ConvArgs& a, bool f16, int32_t* range, int rows_bound, hipStream_t st);

// builds every level and every neighbour table of a forward pass (sparse_map.hip); status as umereg_featnet_forward_f32
int fn_build_maps(const int32_t* coords, int n, int batch, char* ws, int32_t* status, hipStream_t st);

}  // namespace umereg
