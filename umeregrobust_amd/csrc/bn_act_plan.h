// bn_act_plan.h -- the host-checkable arithmetic of bn_act.hip: how the rows of a [n, C] activation are cut into slabs for the
// per-channel sums of batch norm, and how a flat tensor is cut into chunks for the gradient scale's maximum.  Everything here is a pure
// function of the sizes (never of the grid or the device), is __host__ __device__ and launches nothing, so tests/bn_act_plan_host.cpp
// prints the header's own answers on the CPU and tests/test_bn_act_cpu.py compares them with the Python mirror (tests/bn_act_ref.py)
// the GPU tests choose their shapes with.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace umereg {

constexpr int kBnThreads = 256;     // threads of every workgroup of bn_act.hip; a lane owns 4 adjacent channels
constexpr int kBnMaxC = 256;        // channels: multiples of 32 up to this
constexpr int kBnMinPasses = 4;     // a slab is at least this many workgroup passes long
constexpr int kBnMaxSlabs = 256;    // and there are at most this many slabs: the apply kernels re-add the partials themselves

constexpr int kGsChunk = 8192;      // elements behind one partial of the gradient scale's maximum
constexpr int kGsWidth = 256;       // partials the finishing workgroup reads per pass

__host__ __device__ inline bool bn_channels_ok(int C) { return C >= 32 && C <= kBnMaxC && C % 32 == 0; }

struct BnPlan {
    int unit;       // rows one workgroup pass covers: kBnThreads / (C / 4)
    int slab;       // S: rows per slab, a multiple of `unit`
    int slabs;      // ceil(n / S), at most kBnMaxSlabs
    int width;      // W: runs of consecutive slabs the finishing step adds side by side: kBnThreads / C
};

// n > 0, bn_channels_ok(C)
__host__ __device__ inline BnPlan bn_plan(int n, int C)
{
    BnPlan p;
    p.unit = kBnThreads / (C / 4);
    const long long cover = (long long)p.unit * kBnMaxSlabs;
    long long passes = (n + cover - 1) / cover;
    if (passes < kBnMinPasses) passes = kBnMinPasses;
    p.slab = (int)(passes * p.unit);
    p.slabs = (int)(((long long)n + p.slab - 1) / p.slab);
    p.width = kBnThreads / C;
    return p;
}

// two fp64 sums per channel and slab
__host__ __device__ inline size_t bn_scratch_bytes(int n, int C) { return (size_t)bn_plan(n, C).slabs * 2 * (size_t)C * 8; }

__host__ __device__ inline size_t gs_partials(size_t count) { return (count + kGsChunk - 1) / kGsChunk; }

}  // namespace umereg
