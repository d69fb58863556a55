"""Regenerate tests/golden/featnet_state_dict.json: the state-dict names and shapes of the reference's own
`ResUNetSmall2(in_channels=1, out_channels=32)` (models.py:691-698), constructed from the reference tree with
MinkowskiEngine and pytorch3d replaced by placeholder modules.  The placeholders give every
MinkowskiConvolution(Transpose) MinkowskiEngine 0.5.4's parameter shapes -- `kernel` [27, C_in, C_out] for kernel size 3,
[C_in, C_out] for kernel size 1, `bias` [1, C_out] -- and MinkowskiBatchNorm its `.bn` (torch.nn.BatchNorm1d).

    python tools/gen_featnet_state.py /path/to/reference [out.json]
"""
import json
import os
import sys
import types

import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "featnet_state_dict.json")


def _placeholders():
    me = types.ModuleType("MinkowskiEngine")

    class MinkowskiNetwork(nn.Module):
        def __init__(self, D):
            super().__init__()
            self.D = D

    class _Conv(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                     expand_coordinates=False, convolution_mode=None, dimension=None):
            super().__init__()
            volume = kernel_size ** dimension
            shape = (volume, in_channels, out_channels) if volume > 1 else (in_channels, out_channels)
            self.kernel = nn.Parameter(torch.empty(shape))
            self.bias = nn.Parameter(torch.empty(1, out_channels)) if bias else None

    class MinkowskiBatchNorm(nn.Module):
        def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
            super().__init__()
            self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine, track_running_stats=track_running_stats)

    me.MinkowskiNetwork = MinkowskiNetwork
    me.MinkowskiConvolution = type("MinkowskiConvolution", (_Conv,), {})
    me.MinkowskiConvolutionTranspose = type("MinkowskiConvolutionTranspose", (_Conv,), {})
    me.MinkowskiBatchNorm = MinkowskiBatchNorm
    me.MinkowskiInstanceNorm = MinkowskiBatchNorm
    me.utils = types.ModuleType("MinkowskiEngine.utils")
    mef = types.ModuleType("MinkowskiEngine.MinkowskiFunctional")
    me.MinkowskiFunctional = mef
    p3d = types.ModuleType("pytorch3d")
    p3d.structures = types.ModuleType("pytorch3d.structures")
    p3d.structures.Pointclouds = p3d.structures.padded_to_list = None
    p3d.ops = types.ModuleType("pytorch3d.ops")
    p3d.ops.knn_points = p3d.ops.ball_query = p3d.ops.knn_gather = p3d.ops.sample_farthest_points = None
    return {"MinkowskiEngine": me, "MinkowskiEngine.utils": me.utils, "MinkowskiEngine.MinkowskiFunctional": mef,
            "pytorch3d": p3d, "pytorch3d.structures": p3d.structures, "pytorch3d.ops": p3d.ops}


def main(argv):
    ref = os.path.abspath(argv[1])
    out = argv[2] if len(argv) > 2 else DEFAULT_OUT
    sys.dont_write_bytecode = True
    sys.modules.update(_placeholders())
    sys.path.insert(0, ref)
    import models      # the reference's models.py
    net = models.ResUNetSmall2(in_channels=1, out_channels=32)
    state = {k: list(v.shape) for k, v in net.state_dict().items()}
    with open(out, "w") as f:
        json.dump(state, f, indent=0)
        f.write("\n")
    print(f"{out}: {len(state)} entries")


if __name__ == "__main__":
    main(sys.argv)
