// voxel_centroid_math.h -- the host-checkable arithmetic of voxel_centroid.hip: a point's cell, its integer share of the voxel's sum and
// the centroid that sum stands for.  Everything here is __host__ __device__ and launches nothing, so tests/voxel_centroid_host.cpp
// prints the header's own answers on the CPU and tests/test_voxel_centroid_cpu.py compares them with the numpy mirror
// (tests/voxel_centroid_ref.py) the GPU tests compare the kernels with.
//
// The sum is an INTEGER sum, so any arrival order gives the same bits.  Per axis, for a point p (f32) and an edge v (f32):
//   c = floorf(p / v)                              the cell, voxel_key.h's own quotient (fp32 division, fp32 floor)
//   u = (double)p / (double)v - (double)c          the position inside the cell, nominally in [0, 1).  The fp32 quotient can round UP
//                                                  to an integer the real quotient stays below, so u may be as low as minus half an f32
//                                                  ulp of the quotient (>= -2^-4 at 2^20 cells); it never reaches 1 (an integer below
//                                                  2^24 is an f32: a real quotient >= k cannot round below k).  u is signed.
//   q = llrint(u * 2^32)                           |q| <= 2^32 (the scaling is exact, the rounding is to nearest even)
//   S = sum q (int64), cnt = points in the voxel
//   centroid = (float)(((double)c + (double)S / ((double)cnt * 2^32)) * (double)v)
// The build has -ffp-contract=off: every step is one IEEE operation.  (double)S must be exact: n <= kVoxCentroidMaxPoints = 2^20
// points give |S| <= 2^20 * 2^32 = 2^52 < 2^53.  That is where the cap comes from.
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

namespace umereg {

constexpr int kVoxCentroidMaxPoints = 1 << 20;
constexpr double kVoxCentroidScale = 4294967296.0;      // 2^32

__host__ __device__ __forceinline__ float voxel_cell(float p, float voxel)
{
    return floorf(p / voxel);
}

__host__ __device__ __forceinline__ long long voxel_quantum(float p, float voxel, float cell)
{
    const double u = (double)p / (double)voxel - (double)cell;
    return llrint(u * kVoxCentroidScale);
}

__host__ __device__ __forceinline__ float voxel_centroid(float cell, long long sum, int count, float voxel)
{
    return (float)(((double)cell + (double)sum / ((double)count * kVoxCentroidScale)) * (double)voxel);
}

}  // namespace umereg
