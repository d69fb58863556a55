// voxel_key.h -- the host-checkable arithmetic of voxel.hip: the workspace / table plan, the 63-bit voxel key and its home slot.
// Everything here is __host__ __device__ and launches nothing, so tests/voxel_key_host.cpp prints the header's own answers on the
// CPU and tests/test_voxel_key_cpu.py compares them with the Python mirror (tests/glue_cases.py) the GPU edge tests choose their
// inputs with.
#pragma once
#include <cmath>
#include <cstddef>

#include <hip/hip_runtime.h>

namespace umereg {

constexpr int kVoxBlock = 1024;
constexpr unsigned long long kVoxEmpty = ~0ull;         // (no key: a key has 63 bits)

struct VoxWs {
    size_t off_keys, off_min, off_slot, off_bcnt, total;
    unsigned int cap;     // table capacity (power of two, >= 2 n)
    int n_blocks;
};

__host__ __device__ inline VoxWs vox_ws(int n)
{
    VoxWs w;
    unsigned int cap = 1024u;
    while (cap < 2u * (unsigned int)n) cap <<= 1;
    w.cap = cap;
    w.n_blocks = (n + kVoxBlock - 1) / kVoxBlock;
    size_t o = 0;
    w.off_keys = o; o += (size_t)cap * 8;
    w.off_min = o;  o += (size_t)cap * 4;
    w.off_slot = o; o += ((size_t)n + 3) / 4 * 16;
    w.off_bcnt = o; o += ((size_t)w.n_blocks + 1 + 3) / 4 * 16;
    w.total = (o + 255) / 256 * 256;
    return w;
}

// floor(p / voxel) per axis (fp32 division and floor, as torch.floor(coordinates / quantization_size)), 21 bits per axis
__host__ __device__ __forceinline__ bool voxel_key(const float* __restrict__ p, float voxel, unsigned long long& key)
{
    const float fx = floorf(p[0] / voxel), fy = floorf(p[1] / voxel), fz = floorf(p[2] / voxel);
    const float lim = 1048575.0f;                       // |q| < 2^20
    if (!(fabsf(fx) <= lim && fabsf(fy) <= lim && fabsf(fz) <= lim)) return false;      // (NaN / inf / out of range)
    const unsigned long long qx = (unsigned long long)((long long)fx + 1048576ll);
    const unsigned long long qy = (unsigned long long)((long long)fy + 1048576ll);
    const unsigned long long qz = (unsigned long long)((long long)fz + 1048576ll);
    key = (qx << 42) | (qy << 21) | qz;
    return true;
}

// where a key's linear probe starts in a table of `cap` slots (cap a power of two)
__host__ __device__ __forceinline__ unsigned int voxel_home_slot(unsigned long long key, unsigned int cap)
{
    return (unsigned int)((key * 0x9E3779B97F4A7C15ull) >> 32) & (cap - 1u);
}

}  // namespace umereg
