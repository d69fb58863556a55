"""The opt-in point-to-plane refinement: the binding table of csrc/icp_plane_api.h and the names of the two estimations.

    normals = ops.estimate_normals(tgt, knn=30, radius=None)              # open3d: tgt.estimate_normals(KDTreeSearchParamKNN / Hybrid)
    reg = ops.icp_point_to_plane(src, tgt, normals, T_init, 0.2, 200)     # registration_icp(..., TransformationEstimationPointToPlane())
    job = ops.IcpJob(src, tgt, T_init_dev, 0.2, 200, tgt_normals=normals) # the same chain without the wait

`evaluate.refine_registration` and `evaluate.evaluate_pairs` read `args.icp_estimation` ("point_to_point", the default and the
reference's estimator, or "point_to_plane"), `args.icp_normal_knn` (30) and `args.icp_normal_radius` (None).

The entries are declared in csrc/icp_plane_api.h, not under include/, and typed here (ICP_PLANE_SIGNATURES), not in `_lib.TABLES`."""
import ctypes

from . import _lib

c_void_p, c_int, c_float, c_double, c_size_t = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t

# name -> (restype, argtypes); mirrors csrc/icp_plane_api.h one to one
ICP_PLANE_SIGNATURES = {
    "umereg_normals_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_estimate_normals_f32": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_plane_workspace_bytes": (c_size_t, [c_int, c_int]),
    "umereg_icp_point_to_plane_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double, c_double,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_point_to_plane_dev_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double,
                                                  c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_icp_plane_enqueue_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_float, c_int, c_double, c_double,
                                             c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
}

ESTIMATIONS = ("point_to_point", "point_to_plane")
MIN_KNN, MAX_KNN = 3, 64        # UMEREG_NORMALS_MIN_KNN / UMEREG_NORMALS_MAX_KNN
DEFAULT_KNN = 30


def load_native():
    return _lib.load_typed(ICP_PLANE_SIGNATURES)


def check_estimation(who, estimation):
    """None -> "point_to_point"; ValueError for anything but the two names.  Touches no tensor and no library."""
    if estimation is None:
        return ESTIMATIONS[0]
    if estimation not in ESTIMATIONS:
        raise ValueError(f"{who}: icp_estimation must be 'point_to_point' or 'point_to_plane', got {estimation!r}")
    return estimation


def check_knn(who, knn):
    if isinstance(knn, bool) or int(knn) != knn or not MIN_KNN <= int(knn) <= MAX_KNN:
        raise ValueError(f"{who}: knn must be an integer in [{MIN_KNN}, {MAX_KNN}], got {knn!r}")
    return int(knn)


def estimation_of(args, estimation=None):
    """(estimation, knn, radius) a refinement site reads from its `args` (an explicit `estimation` wins)."""
    est = check_estimation("icp", estimation if estimation is not None else getattr(args, "icp_estimation", None))
    knn = getattr(args, "icp_normal_knn", None)
    return est, check_knn("icp", DEFAULT_KNN if knn is None else knn), getattr(args, "icp_normal_radius", None)
