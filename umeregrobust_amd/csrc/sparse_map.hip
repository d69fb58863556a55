// sparse_map.hip -- the coordinate maps of the sparse feature network: five levels (tensor strides 1, 2, 4, 8, 24) and the
// 13 neighbour tables its convolutions gather through.  Every table is an open-addressing hash over the 64-bit coordinate
// key (the voxel.hip pattern); nothing waits for the host: level sizes live in `status`, launches are sized by n.
//
// Level-0 row order (locality): the collate hands points over in random order, and a tile of random rows touches nearly
// every offset and every cache line of the layer below.  Rows are counting-sorted by their 8^3 cell (cells numbered by first
// occurrence), stable: inside a cell by input index -- a cell holds at most 512 points of a cloud, so a point's rank is
// counted directly among its cell's points.  Deterministic throughout: every later level takes the FIRST row (in the order
// of the level below) that falls into a cell as the cell's representative, compacted by a scan.
#include "compact.h"
#include "sparse.h"

namespace umereg {

namespace {

constexpr int kB = 256;

__device__ __forceinline__ unsigned long long* fn_keys(char* ws, const FnWs& w, int t)
{
    return reinterpret_cast<unsigned long long*>(ws + w.off_keys) + (size_t)t * w.cap;
}
__device__ __forceinline__ unsigned int* fn_mins(char* ws, const FnWs& w, int t)
{
    return reinterpret_cast<unsigned int*>(ws + w.off_min) + (size_t)t * w.cap;
}
__device__ __forceinline__ int* fn_rows(char* ws, const FnWs& w, int t)
{
    return reinterpret_cast<int*>(ws + w.off_row) + (size_t)t * w.cap;
}
__device__ __forceinline__ int4* fn_coords(char* ws, const FnWs& w, int l)
{
    return reinterpret_cast<int4*>(ws + w.off_coords) + (size_t)l * w.n;
}

// insert: slot of `key` (claimed if new); *fresh = the key was not there before
__device__ __forceinline__ unsigned int fn_insert(unsigned long long* keys, unsigned int cap, unsigned long long key, bool* fresh)
{
    unsigned int s = fn_hash(key, cap);
    for (;;) {
        const unsigned long long old = atomicCAS(&keys[s], kFnEmpty, key);
        if (old == kFnEmpty || old == key) {
            *fresh = old == kFnEmpty;
            return s;
        }
        s = (s + 1u) & (cap - 1u);
    }
}

__device__ __forceinline__ int fn_lookup(const unsigned long long* keys, unsigned int cap, unsigned long long key)
{
    unsigned int s = fn_hash(key, cap);
    for (;;) {
        const unsigned long long k = keys[s];
        if (k == key) return (int)s;
        if (k == kFnEmpty) return -1;
        s = (s + 1u) & (cap - 1u);
    }
}

// ones over the hash tables, zeros over the cell counts and the offset masks, status = {0, n, 0...}
__global__ __launch_bounds__(kB) void fn_init_kernel(char* __restrict__ ws, FnWs w, int32_t* __restrict__ status)
{
    const size_t ones = w.ones_end / 16, zeros = (w.zero_end - w.ones_end) / 16;
    uint4* p = reinterpret_cast<uint4*>(ws);
    for (size_t i = (size_t)blockIdx.x * kB + threadIdx.x; i < ones + zeros; i += (size_t)gridDim.x * kB) {
        const unsigned int v = i < ones ? 0xffffffffu : 0u;
        p[i] = make_uint4(v, v, v, v);
    }
    if (blockIdx.x == 0 && threadIdx.x < UMEREG_FEATNET_STATUS) status[threadIdx.x] = threadIdx.x == 1 ? w.n : 0;
}

// input row i, validated and clamped (an invalid row raises error bit 1 and is still given a place, so nothing goes out of bounds)
__device__ __forceinline__ int4 fn_input(const int32_t* __restrict__ coords, int i, int batch, int32_t* status)
{
    const int4 c = reinterpret_cast<const int4*>(coords)[i];
    const bool bad = c.x < 0 || c.x >= batch || c.y < -kFnCoordLim || c.y >= kFnCoordLim || c.z < -kFnCoordLim || c.z >= kFnCoordLim ||
                     c.w < -kFnCoordLim || c.w >= kFnCoordLim;
    if (!bad) return c;
    atomicOr(&status[0], 1);
    return make_int4(min(max(c.x, 0), batch - 1), min(max(c.y, -kFnCoordLim), kFnCoordLim - 1), min(max(c.z, -kFnCoordLim), kFnCoordLim - 1),
                     min(max(c.w, -kFnCoordLim), kFnCoordLim - 1));
}

// locality cells: first input index per 8^3 cell
__global__ __launch_bounds__(kB) void fn_cell_insert_kernel(const int32_t* __restrict__ coords, int batch, char* __restrict__ ws, FnWs w,
                                                            int32_t* __restrict__ status)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= w.n) return;
    const int4 c = fn_input(coords, i, batch, status);
    unsigned long long key;
    fn_key(c.x, fn_coarsen(c.y, kFnCellStride), fn_coarsen(c.z, kFnCellStride), fn_coarsen(c.w, kFnCellStride), key);
    bool fresh;
    const unsigned int s = fn_insert(fn_keys(ws, w, kFnSortTable), w.cap, key, &fresh);
    atomicMin(&fn_mins(ws, w, kFnSortTable)[s], (unsigned int)i);
    reinterpret_cast<unsigned int*>(ws + w.off_slot)[i] = s;
}

// flag[r] = row r is the first of its cell in table t (rows < *n_ptr)
__global__ __launch_bounds__(kB) void fn_flag_kernel(char* __restrict__ ws, FnWs w, int t, const int32_t* __restrict__ n_ptr)
{
    const int r = blockIdx.x * kB + threadIdx.x;
    if (r >= *n_ptr) return;
    const unsigned int s = reinterpret_cast<const unsigned int*>(ws + w.off_slot)[r];
    reinterpret_cast<int*>(ws + w.off_flag)[r] = fn_mins(ws, w, t)[s] == (unsigned int)r;
}

// compaction of the flags (compact.h), pass 0: flagged rows per block of kFnScanBlock; pass 1: newid[r] = rank of a flagged row
template <int PASS>
__global__ __launch_bounds__(kFnScanBlock) void fn_compact_kernel(char* __restrict__ ws, FnWs w, const int32_t* __restrict__ n_ptr)
{
    const int n = *n_ptr;
    if ((int)blockIdx.x * kFnScanBlock >= n) return;      // (whole blocks: uniform, in front of block_rank)
    const int* flag = reinterpret_cast<const int*>(ws + w.off_flag);
    int* bcnt = reinterpret_cast<int*>(ws + w.off_bcnt);
    const int r = blockIdx.x * kFnScanBlock + threadIdx.x;
    const bool f = r < n && flag[r];
    const BlockRank k = block_rank<kFnScanBlock>(f);
    if (PASS == 0) {
        if (threadIdx.x == 0) bcnt[blockIdx.x] = k.total;
    } else if (r < n) {
        reinterpret_cast<int*>(ws + w.off_newid)[r] = f ? bcnt[blockIdx.x] + k.before : -1;
    }
}

// exclusive scan (one workgroup) of in[0 .. ceil(*n_ptr / div)) -> out (and out2), sum -> *total; in and out may be one array
__global__ __launch_bounds__(1024) void fn_scan_kernel(const int* in, int* out, int* __restrict__ out2, const int32_t* __restrict__ n_ptr,
                                                       int div, int32_t* __restrict__ total)
{
    const int sum = scan_counts<1024>(in, out, out2, (*n_ptr + div - 1) / div);
    if (threadIdx.x == 1023 && total) *total = sum;
}

// cell ids of the representatives -> the table's row array
__global__ __launch_bounds__(kB) void fn_cell_id_kernel(char* __restrict__ ws, FnWs w)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= w.n) return;
    const unsigned int s = reinterpret_cast<const unsigned int*>(ws + w.off_slot)[i];
    const int id = reinterpret_cast<const int*>(ws + w.off_newid)[i];
    if (id >= 0) fn_rows(ws, w, kFnSortTable)[s] = id;
}

// pass 0: points per cell; pass 1: every point into its cell's range (order inside the range: arbitrary, fixed by the rank below)
__global__ __launch_bounds__(kB) void fn_cell_place_kernel(char* __restrict__ ws, FnWs w, int pass)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= w.n) return;
    const unsigned int s = reinterpret_cast<const unsigned int*>(ws + w.off_slot)[i];
    const int cell = fn_rows(ws, w, kFnSortTable)[s];
    int* cnt = reinterpret_cast<int*>(ws + w.off_cnt);
    if (pass == 0) {
        atomicAdd(&cnt[cell], 1);
    } else {
        const int p = atomicAdd(&reinterpret_cast<int*>(ws + w.off_cursor)[cell], 1);
        reinterpret_cast<int*>(ws + w.off_tmp)[p] = i;
    }
}

// stable order inside a cell: rank = points of the cell with a smaller input index
__global__ __launch_bounds__(kB) void fn_cell_rank_kernel(char* __restrict__ ws, FnWs w)
{
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= w.n) return;
    const unsigned int s = reinterpret_cast<const unsigned int*>(ws + w.off_slot)[i];
    const int cell = fn_rows(ws, w, kFnSortTable)[s];
    const int a = reinterpret_cast<const int*>(ws + w.off_start)[cell];
    const int e = a + reinterpret_cast<const int*>(ws + w.off_cnt)[cell];
    const int* tmp = reinterpret_cast<const int*>(ws + w.off_tmp);
    int rank = 0;
    for (int q = a; q < e; ++q) rank += tmp[q] < i;
    reinterpret_cast<int*>(ws + w.off_perm)[a + rank] = i;
}

// level 0: rows in cell order, one table entry each; a second entry of a key is a duplicate coordinate (error bit 2)
__global__ __launch_bounds__(kB) void fn_level0_kernel(const int32_t* __restrict__ coords, int batch, char* __restrict__ ws, FnWs w,
                                                       int32_t* __restrict__ status)
{
    const int r = blockIdx.x * kB + threadIdx.x;
    if (r >= w.n) return;
    const int i = reinterpret_cast<const int*>(ws + w.off_perm)[r];
    const int4 c = fn_input(coords, i, batch, status);
    fn_coords(ws, w, 0)[r] = c;
    unsigned long long key;
    fn_key(c.x, c.y, c.z, c.w, key);
    bool fresh;
    const unsigned int s = fn_insert(fn_keys(ws, w, 0), w.cap, key, &fresh);
    if (fresh)
        fn_rows(ws, w, 0)[s] = r;
    else
        atomicOr(&status[0], 2);
}

__device__ __forceinline__ int4 fn_coarse(int4 c, int t)
{
    return make_int4(c.x, fn_coarsen(c.y, t), fn_coarsen(c.z, t), fn_coarsen(c.w, t));
}

// level l + 1 from level l: first row of every coarse cell
__global__ __launch_bounds__(kB) void fn_coarse_insert_kernel(char* __restrict__ ws, FnWs w, int l, const int32_t* __restrict__ status)
{
    const int r = blockIdx.x * kB + threadIdx.x;
    if (r >= status[1 + l]) return;
    const int4 c = fn_coarse(fn_coords(ws, w, l)[r], fn_tstride(l + 1));
    unsigned long long key;
    fn_key(c.x, c.y, c.z, c.w, key);
    bool fresh;
    const unsigned int s = fn_insert(fn_keys(ws, w, l + 1), w.cap, key, &fresh);
    atomicMin(&fn_mins(ws, w, l + 1)[s], (unsigned int)r);
    reinterpret_cast<unsigned int*>(ws + w.off_slot)[r] = s;
}

__global__ __launch_bounds__(kB) void fn_coarse_scatter_kernel(char* __restrict__ ws, FnWs w, int l, const int32_t* __restrict__ status)
{
    const int r = blockIdx.x * kB + threadIdx.x;
    if (r >= status[1 + l]) return;
    const int id = reinterpret_cast<const int*>(ws + w.off_newid)[r];
    if (id < 0) return;
    fn_coords(ws, w, l + 1)[id] = fn_coarse(fn_coords(ws, w, l)[r], fn_tstride(l + 1));
    fn_rows(ws, w, l + 1)[reinterpret_cast<const unsigned int*>(ws + w.off_slot)[r]] = id;
}

// neighbour tables: map m, query row q of level ql -> row of level tl at q + sign off_k ts (or -1); one thread per (row, offset),
// the row's 27-bit offset mask by integer atomicOr (order-free)
struct FnMapDesc {
    int ql[kFnMaps], tl[kFnMaps], ts[kFnMaps], sign[kFnMaps];
};

__global__ __launch_bounds__(kB) void fn_map_kernel(char* __restrict__ ws, FnWs w, FnMapDesc d, const int32_t* __restrict__ status)
{
    const int m = blockIdx.y;
    const int e = blockIdx.x * kB + threadIdx.x;
    const int q = e / kFnVol, k = e - q * kFnVol;
    const int ql = d.ql[m], tl = d.tl[m], ts = d.ts[m] * d.sign[m];
    if (q >= status[1 + ql]) return;
    const int4 c = fn_coords(ws, w, ql)[q];
    int dx, dy, dz;
    fn_offset(k, dx, dy, dz);
    unsigned long long key;
    int row = -1;
    if (fn_key(c.x, c.y + dx * ts, c.z + dy * ts, c.w + dz * ts, key)) {
        const int s = fn_lookup(fn_keys(ws, w, tl), w.cap, key);
        row = s >= 0 ? fn_rows(ws, w, tl)[s] : -1;
    }
    reinterpret_cast<int*>(ws + w.off_nbr)[((size_t)m * w.n + q) * kFnVol + k] = row;
    if (row >= 0) atomicOr(&reinterpret_cast<unsigned int*>(ws + w.off_mask)[(size_t)m * w.n + q], 1u << k);
}

}  // namespace

int fn_build_maps(const int32_t* coords, int n, int batch, char* ws, int32_t* status, hipStream_t st)
{
    const FnWs w = fn_ws(n);
    const int g = (n + kB - 1) / kB;
    int* bcnt = reinterpret_cast<int*>(ws + w.off_bcnt);
    const size_t init_vec = (w.zero_end / 16 + kB - 1) / kB;
    hipLaunchKernelGGL(fn_init_kernel, dim3((unsigned)(init_vec < 4096 ? init_vec : 4096)), dim3(kB), 0, st, ws, w, status);
    UMEREG_CHECK_LAUNCH("fn_init_kernel");
    // compaction of ws.flag over *n_ptr rows -> ws.newid, count -> *total
    auto compact = [&](const int32_t* n_ptr, int32_t* total) -> int {
        hipLaunchKernelGGL(fn_compact_kernel<0>, dim3(w.nblk), dim3(kFnScanBlock), 0, st, ws, w, n_ptr);
        UMEREG_CHECK_LAUNCH("fn_compact_kernel");
        hipLaunchKernelGGL(fn_scan_kernel, dim3(1), dim3(1024), 0, st, bcnt, bcnt, (int*)nullptr, n_ptr, kFnScanBlock, total);
        UMEREG_CHECK_LAUNCH("fn_scan_kernel");
        hipLaunchKernelGGL(fn_compact_kernel<1>, dim3(w.nblk), dim3(kFnScanBlock), 0, st, ws, w, n_ptr);
        UMEREG_CHECK_LAUNCH("fn_compact_kernel");
        return UMEREG_OK;
    };
    // level-0 order: stable counting sort by locality cell
    hipLaunchKernelGGL(fn_cell_insert_kernel, dim3(g), dim3(kB), 0, st, coords, batch, ws, w, status);
    UMEREG_CHECK_LAUNCH("fn_cell_insert_kernel");
    hipLaunchKernelGGL(fn_flag_kernel, dim3(g), dim3(kB), 0, st, ws, w, kFnSortTable, status + 1);
    UMEREG_CHECK_LAUNCH("fn_flag_kernel");
    if (int rc = compact(status + 1, status + 6)) return rc;
    hipLaunchKernelGGL(fn_cell_id_kernel, dim3(g), dim3(kB), 0, st, ws, w);
    UMEREG_CHECK_LAUNCH("fn_cell_id_kernel");
    hipLaunchKernelGGL(fn_cell_place_kernel, dim3(g), dim3(kB), 0, st, ws, w, 0);
    UMEREG_CHECK_LAUNCH("fn_cell_place_kernel");
    int* cnt = reinterpret_cast<int*>(ws + w.off_cnt);
    hipLaunchKernelGGL(fn_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, reinterpret_cast<int*>(ws + w.off_start),
                       reinterpret_cast<int*>(ws + w.off_cursor), status + 6, 1, (int32_t*)nullptr);
    UMEREG_CHECK_LAUNCH("fn_scan_kernel");
    hipLaunchKernelGGL(fn_cell_place_kernel, dim3(g), dim3(kB), 0, st, ws, w, 1);
    UMEREG_CHECK_LAUNCH("fn_cell_place_kernel");
    hipLaunchKernelGGL(fn_cell_rank_kernel, dim3(g), dim3(kB), 0, st, ws, w);
    UMEREG_CHECK_LAUNCH("fn_cell_rank_kernel");
    hipLaunchKernelGGL(fn_level0_kernel, dim3(g), dim3(kB), 0, st, coords, batch, ws, w, status);
    UMEREG_CHECK_LAUNCH("fn_level0_kernel");
    // levels 1..4
    for (int l = 0; l + 1 < kFnLevels; ++l) {
        hipLaunchKernelGGL(fn_coarse_insert_kernel, dim3(g), dim3(kB), 0, st, ws, w, l, status);
        UMEREG_CHECK_LAUNCH("fn_coarse_insert_kernel");
        hipLaunchKernelGGL(fn_flag_kernel, dim3(g), dim3(kB), 0, st, ws, w, l + 1, status + 1 + l);
        UMEREG_CHECK_LAUNCH("fn_flag_kernel");
        if (int rc = compact(status + 1 + l, status + 2 + l)) return rc;
        hipLaunchKernelGGL(fn_coarse_scatter_kernel, dim3(g), dim3(kB), 0, st, ws, w, l, status);
        UMEREG_CHECK_LAUNCH("fn_coarse_scatter_kernel");
    }
    // neighbour tables
    FnMapDesc d;
    for (int l = 0; l < kFnLevels; ++l) {
        d.ql[fn_map_self(l)] = l, d.tl[fn_map_self(l)] = l, d.ts[fn_map_self(l)] = fn_tstride(l), d.sign[fn_map_self(l)] = 1;
        if (l + 1 < kFnLevels) {
            // strided: output l+1, gathers level l at + off (ts_in = ts_l); transposed: output l, gathers level l+1 at - off (ts_out = ts_l)
            d.ql[fn_map_down(l)] = l + 1, d.tl[fn_map_down(l)] = l, d.ts[fn_map_down(l)] = fn_tstride(l), d.sign[fn_map_down(l)] = 1;
            d.ql[fn_map_up(l)] = l, d.tl[fn_map_up(l)] = l + 1, d.ts[fn_map_up(l)] = fn_tstride(l), d.sign[fn_map_up(l)] = -1;
        }
    }
    hipLaunchKernelGGL(fn_map_kernel, dim3((unsigned)(((size_t)n * kFnVol + kB - 1) / kB), kFnMaps), dim3(kB), 0, st, ws, w, d, status);
    UMEREG_CHECK_LAUNCH("fn_map_kernel");
    return UMEREG_OK;
}

}  // namespace umereg
