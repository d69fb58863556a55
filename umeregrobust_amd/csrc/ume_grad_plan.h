// ume_grad_plan.h -- the host-checkable arithmetic of ume_grad.hip's distance backward: the 16-keypoint pad and the rule that cuts
// the column range into splits.  Everything here is __host__ __device__ and launches nothing, so tests/ume_grad_plan_host.cpp prints
// the header's own answers on the CPU and tests/test_ume_grad_plan_cpu.py compares them with the Python mirror
// (tests/ume_grad_cases.py) the GPU edge tests choose their shapes with.
#pragma once
#include <hip/hip_runtime.h>

namespace umereg {

constexpr int kRowTiles = 2;       // 32-row tiles of A (8 keypoints each) a wave keeps
constexpr int kRowKp = 8 * kRowTiles;

__host__ __device__ inline int pad_kp(int n) { return (n + kRowKp - 1) / kRowKp * kRowKp; }

struct BwdPlan {
    int n_rt, n_jt, tiles_per_split, splits, n_work;
};

// rows: keypoints of the side whose gradient is formed; cols: the other side's
__host__ __device__ inline BwdPlan bwd_plan(int rows, int cols)
{
    BwdPlan p;
    p.n_rt = pad_kp(rows) / kRowKp;
    p.n_jt = pad_kp(cols) / 8;
    int splits = (4096 + p.n_rt - 1) / p.n_rt;     // enough waves for 256 CUs x 4 SIMDs several times over
    if (splits > 32) splits = 32;
    if (splits > p.n_jt) splits = p.n_jt;
    p.tiles_per_split = (p.n_jt + splits - 1) / splits;
    p.splits = (p.n_jt + p.tiles_per_split - 1) / p.tiles_per_split;
    p.n_work = p.n_rt * p.splits;
    return p;
}

}  // namespace umereg
