// gt_keypoints.hip -- device-side selection of the ground-truth-driven keypoints of generate_ume_from_keypoints2 (reference
// utils/loc_utils.py:86-188) for gfx950; the entries are declared in umereg_gt_keypoints.h.
//
//   candidates  the flagged source points in DESCENDING index order: compact.h's count / scan / scatter over the reversed row
//   select      the density predicate min(hits, max_nn) >= min_nn, evaluated lazily: one wavefront per candidate over the packed
//               search structure (grid.h), the ball's scan left at the min_nn-th hit (no neighbour list, no top-K, no moments), and
//               candidates handed out by a per-element ticket, in the reference's order (from the end of the truncated list to its
//               head), until num_samples dense ones are published; then the first num_samples dense steps of the tested prefix, in
//               order (compact.h's block rank, one workgroup per element)
//   ball_any    for many tiny (q, p) pairs: how many rows of q have a row of p strictly within the radius; p staged in LDS
#include <limits.h>

#include "ball_search.h"
#include "compact.h"
#include "umereg_gt_keypoints.h"

namespace umereg {

constexpr int kGtBlock = 256;           // rows per workgroup of the candidate compaction
constexpr int kGtPickBlock = 1024;      // positions per trip of the pick kernel's one workgroup
constexpr int kGtTestWaves = 4;         // wavefronts (= workers) per workgroup of the density test
constexpr int kGtMaxTestWg = 512;       // workgroups per batch element of the density test, at most
constexpr int kGtWorkersPerSample = 4;  // workers per requested keypoint: a test is a chain of dependent loads, so what hides its
                                        // latency is candidates in flight; the overshoot is balls that leave at the min_nn-th hit
constexpr int kAnyBlock = 256;          // threads of a ball_any workgroup
constexpr int kAnyTile = 4096;          // rows of p staged in LDS at a time (48 KiB)

struct GtWs {
    size_t off_bcnt, off_ctr, off_dense, total;
    int nblk;
};

inline GtWs gt_ws(int B, int N)
{
    GtWs w;
    w.nblk = (N + kGtBlock - 1) / kGtBlock;
    size_t o = 0;
    w.off_bcnt = o;  o += align_up((size_t)B * w.nblk * 4, 16);
    w.off_ctr = o;   o += align_up((size_t)B * 2 * 4, 16);       // ticket[B], found[B]
    w.off_dense = o; o += (size_t)B * N;                         // dense flag per candidate position
    w.total = align_up(o, 256);
    return w;
}

// ---- candidates ----------------------------------------------------------------------------------------------------------
// row r of the reversed order is point N - 1 - r: ascending rows are descending indices
__device__ __forceinline__ bool gt_flag(const int64_t* __restrict__ overlap_idx, const uint8_t* __restrict__ non_flat, int b, int N, int r)
{
    if (r >= N) return false;
    const size_t at = (size_t)b * N + (N - 1 - r);
    return overlap_idx[at] > -1 && non_flat[at] != 0;
}

__global__ __launch_bounds__(kGtBlock) void gt_cand_count_kernel(const int64_t* __restrict__ overlap_idx, const uint8_t* __restrict__ non_flat,
                                                                 int N, int nblk, int* __restrict__ bcnt)
{
    const int b = blockIdx.y, r = blockIdx.x * kGtBlock + threadIdx.x;
    const BlockRank br = block_rank<kGtBlock>(gt_flag(overlap_idx, non_flat, b, N, r));
    if (threadIdx.x == 0) bcnt[(size_t)b * nblk + blockIdx.x] = br.total;
}

__global__ __launch_bounds__(1024) void gt_cand_scan_kernel(int* bcnt, int nblk, int32_t* __restrict__ lengths)
{
    const int b = blockIdx.x;
    int* mine = bcnt + (size_t)b * nblk;
    const int total = scan_counts<1024>(mine, mine, nullptr, nblk);
    if (threadIdx.x == 0) lengths[b] = total;
}

__global__ __launch_bounds__(kGtBlock) void gt_cand_scatter_kernel(const int64_t* __restrict__ overlap_idx, const uint8_t* __restrict__ non_flat,
                                                                   int N, int nblk, const int* __restrict__ bcnt,
                                                                   const int32_t* __restrict__ lengths, int32_t* __restrict__ cand)
{
    const int b = blockIdx.y, r = blockIdx.x * kGtBlock + threadIdx.x;
    const bool keep = gt_flag(overlap_idx, non_flat, b, N, r);
    const BlockRank br = block_rank<kGtBlock>(keep);
    int32_t* row = cand + (size_t)b * N;
    if (keep) row[bcnt[(size_t)b * nblk + blockIdx.x] + br.before] = N - 1 - r;
    if (r < N && r >= lengths[b]) row[r] = -1;      // (kept rows land below lengths[b]: the two writes never meet)
}

// ---- the density predicate -----------------------------------------------------------------------------------------------
// ball_search_grid's walk (ball_search.h: the same rows, chords, loads and predicate) with a counter in place of the list; the
// walk is left once `need` hits are seen.  Returns a count that is >= need iff the ball holds at least `need` points.
template <bool kFma>
__device__ __forceinline__ int ball_count_grid(const float4* __restrict__ P4s, const int* __restrict__ start, const Grid& g, float qx,
                                               float qy, float qz, float r2, int need, int lane)
{
    const float rq = sqrtf(r2) * 1.0001f + 1e-20f;
    const int y0 = cell_axis(qy - rq, g.miny, g.invy, g.ny), y1 = cell_axis(qy + rq, g.miny, g.invy, g.ny);
    const int z0 = cell_axis(qz - rq, g.minz, g.invz, g.nz), z1 = cell_axis(qz + rq, g.minz, g.invz, g.nz);
    const float csy = 1.0f / g.invy, csz = 1.0f / g.invz;
    const float rq2 = rq * rq;
    int cnt = 0;
    const int ny_r = y1 - y0 + 1, n_rows = ny_r * (z1 - z0 + 1);
    for (int r0 = 0; r0 < n_rows; r0 += kWave) {
        int my_beg = 0, my_end = 0;
        {
            const int r = r0 + lane;
            const int z = z0 + r / ny_r, y = y0 + r % ny_r;
            const float z_a = g.minz + (float)z * csz, z_b = z_a + csz;
            const float dzc = fmaxf(fmaxf(z > 0 ? z_a - qz : 0.f, z < g.nz - 1 ? qz - z_b : 0.f), 0.f) * 0.9999f;
            const float y_a = g.miny + (float)y * csy, y_b = y_a + csy;
            const float dyc = fmaxf(fmaxf(y > 0 ? y_a - qy : 0.f, y < g.ny - 1 ? qy - y_b : 0.f), 0.f) * 0.9999f;
            const float rem = rq2 - dyc * dyc - dzc * dzc;
            if (r < n_rows && rem > 0.f) {
                const float sx = sqrtf(rem) * 1.0001f + 1e-20f;
                const int cbase = (z * g.ny + y) * g.nx;
                my_beg = start[cbase + cell_axis(qx - sx, g.minx, g.invx, g.nx)];
                my_end = start[cbase + cell_axis(qx + sx, g.minx, g.invx, g.nx) + 1];
            }
        }
        const int n_here = min(kWave, n_rows - r0);
        for (int rr = 0; rr < n_here; ++rr) {
            const int beg = __builtin_amdgcn_readlane(my_beg, rr);
            const int end = __builtin_amdgcn_readlane(my_end, rr);
            if (beg >= end) continue;                                     // (wave-uniform)
            for (int base = beg; base < end; base += kWave * 2) {
                float4 pv[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int pos = base + u * kWave + lane;
                    pv[u] = P4s[pos < end ? pos : end - 1];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int pos = base + u * kWave + lane;
                    const float dx = qx - pv[u].x, dy = qy - pv[u].y, dz = qz - pv[u].z;
                    const float d2 = dist2_as_the_reference<kFma>(dx, dy, dz);
                    cnt += (int)__popcll(__ballot((pos < end) && (d2 < r2)));
                }
                if (cnt >= need) return cnt;                              // (wave-uniform)
            }
        }
    }
    return cnt;
}

__device__ __forceinline__ int gt_min_length(const int32_t* __restrict__ lengths, int B)
{
    int L = INT_MAX;
    for (int k = 0; k < B; ++k) L = min(L, (int)lengths[k]);
    return L;
}

// One worker per wavefront.  A worker looks at the element's found-counter BEFORE it takes a ticket, always finishes a ticket it
// took, and bumps the counter only for a ticket it took and found dense.  Tickets are steps of the reference's walk over the truncated candidate
// list -- from its END to its head: the reference sorts the dense POSITIONS in descending order -- so what was tested when
// the kernel ends is the prefix [0, min(ticket, L)); if any worker stopped at the counter, num_samples dense tickets of that prefix
// had been counted before it looked, and otherwise the prefix is the whole list.  Either way the first num_samples dense positions
// of the prefix are those of the list.  Nothing waits: a worker's loop is bounded by the tickets.
template <bool kFma>
__global__ __launch_bounds__(kGtTestWaves* kWave) void gt_density_kernel(const char* __restrict__ packed, size_t packed_stride,
                                                                        const int32_t* __restrict__ cand,
                                                                        const int32_t* __restrict__ lengths, int B, int N, float radius,
                                                                        int max_nn, int min_nn, int num_samples, int* ctr,
                                                                        uint8_t* __restrict__ dense)
{
    const int lane = lane_id();
    const int b = blockIdx.y;
    const int L = uniform_int(gt_min_length(lengths, B));
    const GridWs w = grid_ws(N);
    const char* wb = packed + b * packed_stride;
    const float4* P4o = reinterpret_cast<const float4*>(wb + w.off_p4o);
    const float4* P4s = reinterpret_cast<const float4*>(wb + w.off_p4s);
    const int* start = reinterpret_cast<const int*>(wb + w.off_start);
    const Grid g = load_grid(reinterpret_cast<const unsigned int*>(wb + w.off_bbox), radius, N);
    const float r2 = radius * radius;
    int* ticket = ctr + b;
    int* found = ctr + B + b;
    const bool never = min_nn > max_nn, always = min_nn <= 0;
    // Every lane runs the same statements (no branch on the lane inside the loop, so its control flow stays wave-uniform): the
    // counter is read by all lanes at one address, only lane 0 adds a non-zero amount, and lane 0's return value is the ticket.
    const int one = lane == 0 ? 1 : 0;
    for (;;) {
        const int f = __builtin_amdgcn_readfirstlane(__hip_atomic_load(found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (f >= num_samples) break;
        const int t = __builtin_amdgcn_readfirstlane(atomicAdd(ticket, one));
        if (t >= L) break;
        const int ki = cand[(size_t)b * N + (L - 1 - t)];     // the walk: from the end of the truncated list to its head
        bool is_dense = always && !never;
        if (!never && !always && ki >= 0 && ki < N) {
            const float4 qp = P4o[ki];
            is_dense = ball_count_grid<kFma>(P4s, start, g, qp.x, qp.y, qp.z, r2, min_nn, lane) >= min_nn;
        }
        // (the same byte from every lane.  No fence between the flag and the counter: the flags are read by the NEXT launch only, and
        // the stop rule needs a counted ticket to be TAKEN, not visible -- its worker finishes it before the kernel ends.  An agent-scope
        // fence here writes back and invalidates the L2 per candidate: `select` took 1.5 to 1.7 times as long with it.)
        dense[(size_t)b * N + t] = is_dense ? 1 : 0;
        atomicAdd(found, is_dense ? one : 0);
    }
}

__global__ __launch_bounds__(kGtPickBlock) void gt_pick_kernel(const int32_t* __restrict__ cand, const int32_t* __restrict__ lengths, int B,
                                                               int N, int num_samples, const int* __restrict__ ctr,
                                                               const uint8_t* __restrict__ dense, int64_t* __restrict__ kp_index,
                                                               int32_t* __restrict__ record, int32_t* __restrict__ tested)
{
    const int b = blockIdx.x;
    const int L = gt_min_length(lengths, B);
    const int T = min(ctr[b], L);           // the tested prefix: every position below it carries a flag of this call
    int64_t* out = kp_index + (size_t)b * num_samples;
    int base = 0;
    for (int c0 = 0; c0 < T && base < num_samples; c0 += kGtPickBlock) {        // (uniform: base is the same in every thread)
        const int pos = c0 + (int)threadIdx.x;
        const bool keep = pos < T && dense[(size_t)b * N + pos] != 0;
        const BlockRank br = block_rank<kGtPickBlock>(keep);
        if (keep && base + br.before < num_samples) out[base + br.before] = cand[(size_t)b * N + (L - 1 - pos)];
        base += br.total;
        __syncthreads();                    // block_rank's wave counts are read by every wave before the next trip writes them
    }
    const int n = min(base, num_samples);
    for (int s = n + (int)threadIdx.x; s < num_samples; s += kGtPickBlock) out[s] = -1;
    if (threadIdx.x == 0) {
        record[2 * b] = n;
        record[2 * b + 1] = lengths[b];
        if (tested) tested[b] = T;
    }
}

// ---- ball_any ------------------------------------------------------------------------------------------------------------
// One workgroup per (q, p) pair.  p goes through LDS a tile at a time; a lane owns row c * 256 + tid of q for every c (bit c of
// `mask` = that row has its hit), reads the tile's rows as LDS broadcasts and leaves a row's scan once no lane of the wave needs it.
template <bool kFma>
__global__ __launch_bounds__(kAnyBlock) void gt_ball_any_kernel(const float* __restrict__ q, const float* __restrict__ p, int K, float radius,
                                                                int32_t* __restrict__ hits)
{
    __shared__ float sp[kAnyTile * 3];
    __shared__ int total;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* qb = q + (size_t)b * K * 3;
    const float* pb = p + (size_t)b * K * 3;
    const float r2 = radius * radius;
    const int n_c = (K + kAnyBlock - 1) / kAnyBlock;      // <= 30 for K <= 7680
    unsigned int mask = 0;
    if (tid == 0) total = 0;
    for (int t0 = 0; t0 < K; t0 += kAnyTile) {
        const int nt = min(kAnyTile, K - t0);
        __syncthreads();
        for (int e = tid; e < nt * 3; e += kAnyBlock) sp[e] = pb[(size_t)t0 * 3 + e];
        __syncthreads();
        for (int c = 0; c < n_c; ++c) {
            const int row = c * kAnyBlock + tid;
            const bool open = row < K && !((mask >> c) & 1u);
            if (__ballot(open) == 0ull) continue;           // (wave-uniform)
            const int rr = row < K ? row : K - 1;
            const float qx = qb[(size_t)rr * 3], qy = qb[(size_t)rr * 3 + 1], qz = qb[(size_t)rr * 3 + 2];
            bool hit = false;
            for (int j0 = 0; j0 < nt; j0 += 8) {
                if (__ballot(open && !hit) == 0ull) break;  // wave vote: every row of this wave has its hit
                const int j1 = min(j0 + 8, nt);
                for (int j = j0; j < j1; ++j) {
                    const float dx = qx - sp[3 * j], dy = qy - sp[3 * j + 1], dz = qz - sp[3 * j + 2];
                    hit = hit || (dist2_as_the_reference<kFma>(dx, dy, dz) < r2);
                }
            }
            if (open && hit) mask |= 1u << c;
        }
    }
    const int mine = __popc(mask);
    if (mine) atomicAdd(&total, mine);      // (an integer sum in LDS: the same whatever the order)
    __syncthreads();
    if (tid == 0) hits[b] = total;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_gt_keypoints_workspace_bytes(int B, int N)
{
    if (B < 1 || B > UMEREG_GT_KEYPOINTS_MAX_B || N < 1) return 0;
    return gt_ws(B, N).total;
}

UMEREG_API int umereg_gt_candidates(const int64_t* overlap_idx, const uint8_t* non_flat, int B, int N, int32_t* cand, int32_t* lengths,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(overlap_idx && non_flat && cand && lengths, "gt_candidates: null pointer");
    UMEREG_REQUIRE(B >= 1 && B <= UMEREG_GT_KEYPOINTS_MAX_B && N >= 1, "gt_candidates: B in [1, %d] and N >= 1 expected (got %d, %d)",
                   UMEREG_GT_KEYPOINTS_MAX_B, B, N);
    UMEREG_REQUIRE_WORKSPACE("gt_candidates", workspace, workspace_bytes, umereg_gt_keypoints_workspace_bytes(B, N));
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const GtWs w = gt_ws(B, N);
    int* bcnt = reinterpret_cast<int*>((char*)workspace + w.off_bcnt);
    hipLaunchKernelGGL(gt_cand_count_kernel, dim3(w.nblk, B), dim3(kGtBlock), 0, st, overlap_idx, non_flat, N, w.nblk, bcnt);
    UMEREG_CHECK_LAUNCH("gt_cand_count_kernel");
    hipLaunchKernelGGL(gt_cand_scan_kernel, dim3(B), dim3(1024), 0, st, bcnt, w.nblk, lengths);
    UMEREG_CHECK_LAUNCH("gt_cand_scan_kernel");
    hipLaunchKernelGGL(gt_cand_scatter_kernel, dim3(w.nblk, B), dim3(kGtBlock), 0, st, overlap_idx, non_flat, N, w.nblk, (const int*)bcnt,
                       (const int32_t*)lengths, cand);
    UMEREG_CHECK_LAUNCH("gt_cand_scatter_kernel");
    return UMEREG_OK;
}

UMEREG_API int umereg_gt_select_f32(const void* packed, const int32_t* cand, const int32_t* lengths, int B, int N, float radius, int max_nn,
                                    int min_nn, int num_samples, int flags, int64_t* kp_index, int32_t* record, int32_t* tested,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(packed && cand && lengths && kp_index && record, "gt_select: null pointer");
    UMEREG_REQUIRE(B >= 1 && B <= UMEREG_GT_KEYPOINTS_MAX_B && N >= 1, "gt_select: B in [1, %d] and N >= 1 expected (got %d, %d)",
                   UMEREG_GT_KEYPOINTS_MAX_B, B, N);
    UMEREG_REQUIRE(radius > 0.f, "gt_select: radius must be positive");
    UMEREG_REQUIRE(num_samples >= 1, "gt_select: num_samples must be positive (got %d)", num_samples);
    UMEREG_REQUIRE((flags & ~UMEREG_BALL_FMA) == 0, "gt_select: unknown flags 0x%x", flags);
    UMEREG_REQUIRE(((uintptr_t)packed & 15) == 0, "gt_select: packed structure misaligned");
    UMEREG_REQUIRE_WORKSPACE("gt_select", workspace, workspace_bytes, umereg_gt_keypoints_workspace_bytes(B, N));
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const GtWs w = gt_ws(B, N);
    int* ctr = reinterpret_cast<int*>((char*)workspace + w.off_ctr);
    uint8_t* dense = reinterpret_cast<uint8_t*>((char*)workspace + w.off_dense);
    if (int rc = launch_zero(ctr, (size_t)B * 2 * 4, 1, 0, st)) return rc;
    // workers: kGtWorkersPerSample candidates in flight per requested keypoint, no more than the list can feed
    const int want = (std::min(num_samples, 1 << 20) * kGtWorkersPerSample + kGtTestWaves - 1) / kGtTestWaves;
    const int most = (N + kGtTestWaves - 1) / kGtTestWaves;
    const int n_wg = std::max(1, std::min(std::min(want, most), kGtMaxTestWg));
    const size_t stride = grid_ws(N).total;
    if (flags & UMEREG_BALL_FMA)
        hipLaunchKernelGGL(gt_density_kernel<true>, dim3(n_wg, B), dim3(kGtTestWaves * kWave), 0, st, (const char*)packed, stride, cand, lengths,
                           B, N, radius, max_nn, min_nn, num_samples, ctr, dense);
    else
        hipLaunchKernelGGL(gt_density_kernel<false>, dim3(n_wg, B), dim3(kGtTestWaves * kWave), 0, st, (const char*)packed, stride, cand, lengths,
                           B, N, radius, max_nn, min_nn, num_samples, ctr, dense);
    UMEREG_CHECK_LAUNCH("gt_density_kernel");
    hipLaunchKernelGGL(gt_pick_kernel, dim3(B), dim3(kGtPickBlock), 0, st, cand, lengths, B, N, num_samples, (const int*)ctr,
                       (const uint8_t*)dense, kp_index, record, tested);
    UMEREG_CHECK_LAUNCH("gt_pick_kernel");
    return UMEREG_OK;
}

UMEREG_API int umereg_gt_ball_any_f32(const float* q, const float* p, int Bk, int K, float radius, int flags, int32_t* hits, void* stream)
{
    UMEREG_REQUIRE(q && p && hits, "gt_ball_any: null pointer");
    UMEREG_REQUIRE(Bk >= 1, "gt_ball_any: Bk must be positive (got %d)", Bk);
    UMEREG_REQUIRE(K >= 1 && K <= UMEREG_GT_BALL_ANY_MAX_K, "gt_ball_any: K must be in [1, %d] (got %d)", UMEREG_GT_BALL_ANY_MAX_K, K);
    UMEREG_REQUIRE(radius > 0.f, "gt_ball_any: radius must be positive");
    UMEREG_REQUIRE((flags & ~UMEREG_BALL_FMA) == 0, "gt_ball_any: unknown flags 0x%x", flags);
    if (int rc = check_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (flags & UMEREG_BALL_FMA)
        hipLaunchKernelGGL(gt_ball_any_kernel<true>, dim3(Bk), dim3(kAnyBlock), 0, st, q, p, K, radius, hits);
    else
        hipLaunchKernelGGL(gt_ball_any_kernel<false>, dim3(Bk), dim3(kAnyBlock), 0, st, q, p, K, radius, hits);
    UMEREG_CHECK_LAUNCH("gt_ball_any_kernel");
    return UMEREG_OK;
}
