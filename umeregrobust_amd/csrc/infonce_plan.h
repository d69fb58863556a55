// infonce_plan.h -- the host-checkable arithmetic of infonce.hip: the tile constants of the fused InfoNCE kernels, the sizes they
// accept and the layout of the caller's workspace.  Everything here is a pure function of the sizes (never of the grid or the device),
// is __host__ __device__ and launches nothing, so tests/infonce_plan_host.cpp prints the header's own answers on the CPU and
// tests/test_infonce_cpu.py compares them with the Python restatement (tests/infonce_cases.py) the GPU tests place their edges with.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace umereg {

constexpr int kInfoNceD = 32;               // feature channels: the only width the kernels are built for
constexpr int kInfoNceWaves = 4;            // waves of a workgroup; each takes 32 of the kInfoNceCols columns of a step
constexpr int kInfoNceThreads = 64 * kInfoNceWaves;
constexpr int kInfoNceRows = 32;            // R: rows (samples) a workgroup owns -- one MFMA tile edge
constexpr int kInfoNceCols = 32 * kInfoNceWaves;    // C: samples of the walked side staged in LDS per step
constexpr int kInfoNceLdsStride = 36;       // floats per staged feature row: 32 + 4, so that 16 rows of float4 reads cover all 64 banks
constexpr int kInfoNceMaxS = 8192;          // largest S: the scatter keeps the S row indices of one batch element in LDS
constexpr int kInfoNceScatterRows = 64;     // samples a workgroup of the scatter looks after (16 per wave)

// staged features + one float4 (x, y, z, lse) per staged sample; the combine of the four waves reuses the feature area
constexpr size_t kInfoNceLdsBytes = (size_t)kInfoNceCols * kInfoNceLdsStride * 4 + (size_t)kInfoNceCols * 16;
constexpr size_t kInfoNceScatterLdsBytes = (size_t)kInfoNceMaxS * 4;
constexpr size_t kInfoNceLdsPerCu = 160 * 1024;
static_assert(2 * kInfoNceLdsBytes <= kInfoNceLdsPerCu && 2 * kInfoNceScatterLdsBytes <= kInfoNceLdsPerCu,
              "two workgroups per CU must fit in LDS");
static_assert(((size_t)kInfoNceWaves * 32 * 32 + 2 * 32 + 2 * kInfoNceWaves * 32) * 4 <= (size_t)kInfoNceCols * kInfoNceLdsStride * 4,
              "the combine, its coefficients and the row sums reuse the feature area");

__host__ __device__ inline int infonce_row_blocks(int S) { return (S + kInfoNceRows - 1) / kInfoNceRows; }
__host__ __device__ inline int infonce_col_steps(int S) { return (S + kInfoNceCols - 1) / kInfoNceCols; }

// what the compute entries accept (the grid is B * row_blocks workgroups wide, twice that in the scatter)
__host__ __device__ inline bool infonce_sizes_ok(long long B, long long N, long long M, long long S)
{
    if (B < 1 || N < 1 || M < 1 || S < 1 || S > kInfoNceMaxS) return false;
    if (N > 0x7fffffffLL || M > 0x7fffffffLL) return false;
    return B * infonce_row_blocks((int)S) <= 0x3fffffffLL;
}

struct InfoNceLayout {
    size_t part;    // fp64 [B][row_blocks]: the row sums of each workgroup of the forward
    size_t da;      // f32 [B][S][32]: per-sample gradient of the anchors, before the scatter
    size_t dp;      // f32 [B][S][32]: per-sample gradient of the positives
    size_t nm;      // f32 [B][S]: the negatives' share of each row, sum_t w_st, from the row pass to the column pass
    size_t total;
};

__host__ __device__ inline size_t infonce_align(size_t v) { return (v + 255) / 256 * 256; }

// infonce_sizes_ok(B, 1, 1, S)
__host__ __device__ inline InfoNceLayout infonce_layout(int B, int S)
{
    InfoNceLayout L;
    L.part = 0;
    L.da = infonce_align((size_t)B * infonce_row_blocks(S) * 8);
    L.dp = L.da + infonce_align((size_t)B * S * kInfoNceD * 4);
    L.nm = L.dp + infonce_align((size_t)B * S * kInfoNceD * 4);
    L.total = L.nm + infonce_align((size_t)B * S * 4);
    return L;
}

}  // namespace umereg
