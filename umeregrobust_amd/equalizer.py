"""The built-in sampling equalizer: a ready-made `completion_fn` for the place where the reference calls NKSR.

    new_pts = equalizer.equalize_cloud(pts)                                        # 125 000 points of uniform density
    new_pts, new_seg = raw_scan.complete_cloud(pts, seg, equalizer.sampling_equalizer)
    SemanticKITTIDataset(..., use_pc_completion=True, completion_fn=equalizer.sampling_equalizer)      # NuscenesDataset alike
    python -m umeregrobust_amd.datasets.sem_preprocessing ... --nksr True --completion umeregrobust_amd.equalizer:sampling_equalizer

The reference's Sampling Equalizer Module (`lidar_point_cloud_completion`, datasets/kitti/kitti_dataset.py:511-542) rebuilds a surface
from the scan with NKSR, a learned kernel field, samples 125 000 points uniformly from it and copies labels back.  NKSR is not rebuilt
here and no similarity to its samples is claimed: this is the library's OWN equalizer, a deterministic surfel resampler that undoes the
1/r^2 density of a spinning lidar -- every point becomes a small tangent patch whose area is the inverse of the local density, samples
are allocated to patches in proportion to area (systematic resampling, in integers), placed on them, and moved once onto the locally fitted
plane (one moving-least-squares step).  The contract is stated in csrc/equalize_api.h and DESIGN.md 4.20; the kernels are
csrc/equalize.hip.  The defaults (16 neighbours, supports capped at 1 m) are choices, not tuned on real scans.  Opt-in: nothing uses
it unless it is passed as the completion.

The entries are declared in csrc/equalize_api.h, a private header: EQUALIZE_SIGNATURES is their table, typed by `load_native`
through `_lib.load_typed`.  Every call is enqueued on the current stream; `equalize_cloud` and `sample` read one word back (the summed
area weights: zero means there is nothing to sample from, a ValueError)."""
import ctypes
import numbers

import torch

from . import _lib

c_void_p, c_int, c_float, c_size_t, c_uint32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_uint32

EQUALIZE_SIGNATURES = {
    "umereg_equalize_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "umereg_equalize_surfels_f32": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_equalize_sample_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_uint32, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_equalize_project_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "umereg_equalize_cloud_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_float, c_int, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_size_t, c_void_p]),
}

NUM_POINTS = 125000                     # the reference's NKSR_NUM_SAMPLED_POINTS
MIN_KNN, MAX_KNN, DEFAULT_KNN = 3, 64, 16            # UMEREG_EQUALIZE_MIN_KNN / _MAX_KNN
MAX_POINTS = 1 << 22                                 # UMEREG_EQUALIZE_MAX_POINTS: n and num_points
MIN_RADIUS, MAX_RADIUS, DEFAULT_RADIUS = 1e-3, 1e3, 1.0


def load_native():
    """the library with the equalizer's entries typed"""
    return _lib.load_typed(EQUALIZE_SIGNATURES)


# ---- argument rules (no tensor and no library touched) ------------------------------------------------------------------------------

def check_knn(who, knn):
    if isinstance(knn, bool) or not isinstance(knn, numbers.Real) or int(knn) != knn or not MIN_KNN <= int(knn) <= MAX_KNN:
        raise ValueError(f"{who}: knn must be an integer in [{MIN_KNN}, {MAX_KNN}], got {knn!r}")
    return int(knn)


def check_count(who, name, value):
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or int(value) != value or not 1 <= int(value) <= MAX_POINTS:
        raise ValueError(f"{who}: {name} must be an integer in [1, 2^22], got {value!r}")
    return int(value)


def check_radius(who, max_radius):
    if isinstance(max_radius, bool) or not isinstance(max_radius, numbers.Real) or not MIN_RADIUS <= float(max_radius) <= MAX_RADIUS:
        raise ValueError(f"{who}: max_radius must be a number in [{MIN_RADIUS}, {MAX_RADIUS}], got {max_radius!r}")
    return float(max_radius)


def check_seed(who, seed):
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= int(seed) < 1 << 32:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^32), got {seed!r}")
    return int(seed)


def _cloud(who, pts, name="pts", least=1):
    if not isinstance(pts, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor, got {type(pts).__name__}")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"{who}: {name} must be [n,3], got {tuple(pts.shape)}")
    check_count(who, f"the number of {name}", pts.shape[0])
    if pts.shape[0] < least:
        raise ValueError(f"{who}: a cloud of {pts.shape[0]} points has no surfel with an area (the summed area weights Qt are 0; "
                         f"{least} points are the least)")
    if pts.device.type != "cuda":
        raise RuntimeError(f"{who}: {name} on the CPU; umeregrobust_amd has no CPU fallback (move the input to the GPU)")
    return pts.to(torch.float32).contiguous()


def _vector(who, t, name, n, dtype, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.shape != (n,) or t.device != dev:
        raise ValueError(f"{who}: {name} must be a {dtype} [{n}] tensor on {dev}")
    return t.contiguous()


def _workspace(dev, n, num_points, knn):
    from . import ops
    return ops._workspace(dev, load_native().umereg_equalize_workspace_bytes(n, num_points, knn), "equalize")


def _total(who, total):
    if int(total.item()) == 0:                    # the one device -> host read
        raise ValueError(f"{who}: the summed area weights Qt are 0: every point is a duplicate of its neighbours, there is no surface to sample")


# ---- the stages ---------------------------------------------------------------------------------------------------------------------

def surfels(pts, knn=DEFAULT_KNN, max_radius=DEFAULT_RADIUS):
    """pts f32 [n,3] -> (normals f32 [n,3], r2 f32 [n], q int32 [n] holding the uint32 area weights)"""
    who = "equalizer.surfels"
    knn, max_radius = check_knn(who, knn), check_radius(who, max_radius)
    p = _cloud(who, pts)
    n, dev = p.shape[0], p.device
    lib = load_native()
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev)
    r2 = torch.empty(n, dtype=torch.float32, device=dev)
    q = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _workspace(dev, n, 1, knn)
    _lib.call(dev, lib.umereg_equalize_surfels_f32, p.data_ptr(), n, knn, max_radius, normals.data_ptr(), r2.data_ptr(), q.data_ptr(),
              ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    return normals, r2, q


def sample(pts, normals, r2, q, num_points=NUM_POINTS, knn=DEFAULT_KNN, seed=0):
    """the surfels of `pts` (made with this `knn`) -> (samples f32 [M,3], src_index int64 [M], rho2 f32 [M]).  One device -> host read."""
    who = "equalizer.sample"
    num_points, knn, seed = check_count(who, "num_points", num_points), check_knn(who, knn), check_seed(who, seed)
    p = _cloud(who, pts, least=3)
    n, dev = p.shape[0], p.device
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or normals.shape != p.shape or normals.device != dev:
        raise ValueError(f"{who}: normals must be a float32 {tuple(p.shape)} tensor on {dev}")
    normals, r2, q = normals.contiguous(), _vector(who, r2, "r2", n, torch.float32, dev), _vector(who, q, "q", n, torch.int32, dev)
    lib = load_native()
    samples = torch.empty(num_points, 3, dtype=torch.float32, device=dev)
    src = torch.empty(num_points, dtype=torch.int64, device=dev)
    rho2 = torch.empty(num_points, dtype=torch.float32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(dev, n, 1, knn)
    _lib.call(dev, lib.umereg_equalize_sample_f32, p.data_ptr(), normals.data_ptr(), r2.data_ptr(), q.data_ptr(), n, num_points, knn, seed,
              samples.data_ptr(), src.data_ptr(), rho2.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    _total(who, total)
    return samples, src, rho2


def project(samples, rho2, pts, return_count=False):
    """one moving-least-squares step of every sample onto the plane of the original points within sqrt(rho2) of it -> f32 [M,3]
    (with return_count: + the neighbours used, int32 [M])"""
    who = "equalizer.project"
    s, p = _cloud(who, samples, "samples"), _cloud(who, pts)
    m, n, dev = s.shape[0], p.shape[0], p.device
    if s.device != dev:
        raise ValueError(f"{who}: samples and pts must be on one device")
    rho2 = _vector(who, rho2, "rho2", m, torch.float32, dev)
    lib = load_native()
    out = torch.empty(m, 3, dtype=torch.float32, device=dev)
    cnt = torch.empty(m, dtype=torch.int32, device=dev) if return_count else None
    ws = _workspace(dev, n, 1, MIN_KNN)
    _lib.call(dev, lib.umereg_equalize_project_f32, s.data_ptr(), rho2.data_ptr(), p.data_ptr(), m, n, out.data_ptr(), _lib.ptr(cnt),
              ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    return (out, cnt) if return_count else out


# ---- the whole call -----------------------------------------------------------------------------------------------------------------

def equalize_cloud(pts, num_points=NUM_POINTS, knn=DEFAULT_KNN, max_radius=DEFAULT_RADIUS, project=True, seed=0, return_index=False):
    """pts f32 [n,3] on the device (sensor at the origin) -> new_pts f32 [num_points,3] of uniform surface density (with return_index:
    + src_index int64 [num_points], the original point each sample was placed around).  The three stages chained on the current stream
    in one native call; equal inputs give equal bits.  One device -> host read (the summed area weights)."""
    who = "equalize_cloud"
    num_points, knn, max_radius, seed = (check_count(who, "num_points", num_points), check_knn(who, knn), check_radius(who, max_radius),
                                         check_seed(who, seed))
    p = _cloud(who, pts, least=3)
    n, dev = p.shape[0], p.device
    lib = load_native()
    out = torch.empty(num_points, 3, dtype=torch.float32, device=dev)
    src = torch.empty(num_points, dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(dev, n, num_points, knn)
    _lib.call(dev, lib.umereg_equalize_cloud_f32, p.data_ptr(), n, num_points, knn, max_radius, 1 if project else 0, seed, out.data_ptr(),
              src.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    _total(who, total)
    return (out, src) if return_index else out


def make_equalizer(**kw):
    """a `completion_fn(pts) -> new_pts` with other parameters than the defaults (those of `equalize_cloud`, checked here)"""
    unknown = set(kw) - {"num_points", "knn", "max_radius", "project", "seed"}
    if unknown:
        raise ValueError(f"make_equalizer: unknown parameters {sorted(unknown)}")
    for name, rule in (("num_points", lambda v: check_count("make_equalizer", "num_points", v)), ("knn", lambda v: check_knn("make_equalizer", v)),
                       ("max_radius", lambda v: check_radius("make_equalizer", v)), ("seed", lambda v: check_seed("make_equalizer", v))):
        if name in kw:
            rule(kw[name])

    def completion_fn(pts):
        return equalize_cloud(pts, **kw)
    return completion_fn


def sampling_equalizer(pts):
    """`completion_fn` with the defaults: 125 000 points, 16 neighbours, supports capped at 1 m, projection on, seed 0"""
    return equalize_cloud(pts)
