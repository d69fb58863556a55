// sparse_wgrad.h -- what the weight gradient's two precisions share (sparse_wgrad.hip: f32, sparse_wgrad_f16.hip: f16 operands):
// the row segmentation and the channel check.  Host arithmetic only; not part of the C ABI.
#pragma once
#include "sparse.h"
#include "umereg_sparse_conv.h"

namespace umereg {

struct WgPlan {
    int rps, segments;      // rows per segment, segments over [0, n)
    size_t block;           // floats of one [27][cin][cout] block
};

// depends on n, cin, cout only: at most 64 segments and about 64 MB of partial blocks, at least 1024 rows per segment
inline WgPlan wg_plan(int n, int cin, int cout)
{
    WgPlan p;
    p.block = (size_t)kFnVol * cin * cout;
    size_t smax = ((size_t)64 << 20) / (p.block * 4);
    if (smax < 1) smax = 1;
    if (smax > UMEREG_SPARSE_CONV_MAX_SEGMENTS) smax = UMEREG_SPARSE_CONV_MAX_SEGMENTS;
    size_t rps = align_up(((size_t)n + smax - 1) / smax, 64);
    if (rps < 1024) rps = 1024;
    p.rps = (int)rps;
    p.segments = (int)(((size_t)n + rps - 1) / rps);
    return p;
}

inline bool wg_channels_ok(int cin, int cout)
{
    return (cin == 1 || (cin > 0 && cin % 32 == 0 && cin <= UMEREG_SPARSE_CONV_MAX_CH)) && cout > 0 && cout % 32 == 0 &&
           cout <= UMEREG_SPARSE_CONV_MAX_CH;
}

}  // namespace umereg
