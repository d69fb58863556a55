"""The opt-in point-to-plane refinement: the binding table of include/umereg_icp_plane.h and the names of the two estimations.

    normals = ops.estimate_normals(tgt, knn=30, radius=None)              # open3d: tgt.estimate_normals(KDTreeSearchParamKNN / Hybrid)
    reg = ops.icp_point_to_plane(src, tgt, normals, T_init, 0.2, 200)     # registration_icp(..., TransformationEstimationPointToPlane())
    job = ops.IcpJob(src, tgt, T_init_dev, 0.2, 200, tgt_normals=normals) # the same chain without the wait

`evaluate.refine_registration` and `evaluate.evaluate_pairs` read `args.icp_estimation` ("point_to_point", the default and the
reference's estimator, "point_to_plane", or "plane_to_plane": icp_gicp.py), `args.icp_normal_knn` (30) and `args.icp_normal_radius`
(None)."""
from . import _lib

ICP_PLANE_SIGNATURES = _lib.TABLES["umereg_icp_plane.h"]
load_native = _lib.load

ESTIMATIONS = ("point_to_point", "point_to_plane", "plane_to_plane")     # the last one: icp_gicp.py (Segal's name for that form)
MIN_KNN, MAX_KNN = 3, 64        # UMEREG_NORMALS_MIN_KNN / UMEREG_NORMALS_MAX_KNN
DEFAULT_KNN = 30


def check_estimation(who, estimation):
    """None -> "point_to_point"; ValueError for anything but the three names.  Touches no tensor and no library."""
    if estimation is None:
        return ESTIMATIONS[0]
    if estimation not in ESTIMATIONS:
        raise ValueError(f"{who}: icp_estimation must be one of {', '.join(map(repr, ESTIMATIONS))}, got {estimation!r}")
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
