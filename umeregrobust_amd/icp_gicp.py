"""The opt-in plane-to-plane (generalized) ICP refinement: the binding table of include/umereg_icp_gicp.h and the rules for epsilon.

    ns, nt = ops.estimate_normals(src), ops.estimate_normals(tgt)            # the source's normals in the SOURCE's own frame
    reg = ops.icp_plane_to_plane(src, tgt, ns, nt, T_init, 0.2, 200)         # registration_generalized_icp(..., epsilon=1e-3)
    job = ops.IcpJob(src, tgt, T_init_dev, 0.2, 200, src_normals=ns, tgt_normals=nt, epsilon=1e-3)   # the same chain without the wait

`evaluate.refine_registration` and `evaluate.evaluate_pairs` take it as `args.icp_estimation = "plane_to_plane"` (Segal et al.'s
name for this form of Generalized ICP) and read `args.icp_gicp_epsilon` (1e-3) through `epsilon_of`; normals come from
`args.icp_normal_knn` / `args.icp_normal_radius` as for point to plane, once for each cloud.

The entries are declared in include/umereg_icp_gicp.h and typed by `_lib.TABLES`; ICP_GICP_SIGNATURES is that table."""
import numbers

from . import _lib

ICP_GICP_SIGNATURES = _lib.TABLES["umereg_icp_gicp.h"]
load_native = _lib.load

ESTIMATION = "plane_to_plane"
MIN_EPSILON, MAX_EPSILON = 1e-4, 1.0        # UMEREG_GICP_MIN_EPSILON / UMEREG_GICP_MAX_EPSILON
DEFAULT_EPSILON = 1e-3                      # open3d's default, as recalled


def check_epsilon(who, epsilon):
    """epsilon as a float in [1e-4, 1] (ValueError otherwise: a bool, a non-number, NaN, anything outside).  Below 1e-4 the f32
    rounding of a unit normal becomes comparable to 2 epsilon, the smallest eigenvalue of the matrix the kernel inverts."""
    if isinstance(epsilon, bool) or not isinstance(epsilon, numbers.Real) or not MIN_EPSILON <= float(epsilon) <= MAX_EPSILON:
        raise ValueError(f"{who}: epsilon must be a number in [{MIN_EPSILON}, {MAX_EPSILON}], got {epsilon!r}")
    return float(epsilon)


def epsilon_of(args):
    """the epsilon a refinement site reads from its `args`: args.icp_gicp_epsilon, default 1e-3"""
    epsilon = getattr(args, "icp_gicp_epsilon", None)
    return check_epsilon("icp", DEFAULT_EPSILON if epsilon is None else epsilon)
