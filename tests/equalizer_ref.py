"""Restatement of the sampling equalizer's contract (umeregrobust_amd/csrc/equalize_api.h) in numpy and Python integers, for
tests/test_equalizer_cpu.py and tests/test_equalizer_gpu.py: brute-force f32 distances in the library's operation order, kNN with ties to
the lower index, fp64 covariance and `eigh` normals with the canonical sign, the area weights in numpy float32, Python-int prefix sums
and allocation, the integer mix, placement and projection in fp64.  Beside every result it reports what justifies a gate on it: the
eigen-gap of each neighbourhood a normal came from, and the smallest distance of any d2 to the rho2 cut it was tested against.
csrc/equalize_math.h compiled for the host (tests/equalize_math_host.cpp) is the bit-exact side of the f32 placement."""
import atexit
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MASK32 = 0xFFFFFFFF
M32 = np.uint64(MASK32)
STREAM_STEP = 0x9E3779B9
MAX_POINTS = 1 << 22


# ------------------------------------------------------------------------------------------------ the mix
def lowbias32(x):
    """C. Wellons' lowbias32 on numpy uint32 arrays (or Python ints)"""
    x = np.array(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def xi(seed, j, c):
    """xi_c(j): the top 24 bits of the mix of (seed, j, c) -> uint64 array like j"""
    k = lowbias32((int(seed) + int(c) * STREAM_STEP) & MASK32)
    return lowbias32((np.asarray(j, np.uint64) + k) & M32) >> np.uint64(8)


# ------------------------------------------------------------------------------------------------ surfels
def d2_f32(a, b):
    """the library's predicate distance between rows of a [m,3] and b [n,3] -> f32 [m,n]: ((dx*dx) + (dy*dy)) + (dz*dz), one rounding each"""
    d = a[:, None, :].astype(F32) - b[None, :, :].astype(F32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn(pts, K, chunk=256):
    """the K nearest points of the cloud for each of its points, itself included: (idx int64 [n,K], d2 f32 [n,K]) ascending, ties to
    the lower index.  The key (d2 bits << 32 | index) orders like (d2, index): d2 >= 0."""
    p = np.ascontiguousarray(pts, F32)
    n = p.shape[0]
    idx, d2 = np.empty((n, K), np.int64), np.empty((n, K), F32)
    for a in range(0, n, chunk):
        d = d2_f32(p[a:a + chunk], p)
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
        part = np.partition(key, K - 1, axis=1)[:, :K] if K < n else key
        part = np.sort(part, axis=1)
        idx[a:a + chunk] = (part & M32).astype(np.int64)
        d2[a:a + chunk] = (part >> np.uint64(32)).astype(np.uint32).view(F32)
    return idx, d2


def canonical(v):
    """the sign rule of covariance_normal: the component of largest magnitude positive, ties -> the lowest axis"""
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def normal_of(C):
    """(unit normal f64 [3], gap = (l1 - l0) / l2) of a covariance; a zero covariance -> ((0,0,1), 0)"""
    if not C.any():
        return np.array([0.0, 0.0, 1.0]), 0.0
    w, V = np.linalg.eigh(C)
    return canonical(V[:, 0]), float((w[1] - w[0]) / w[2]) if w[2] > 0 else 0.0


def scale_of(max_radius):
    """(r_max^2 in f32, s = (float)(65536 / r_max^2)) as the host side of the library forms them"""
    r = F32(max_radius)
    return r * r, F32(65536.0 / (float(r) * float(r)))


def surfels(pts, knn_k=16, max_radius=1.0):
    """-> dict(normals f64 [n,3], gap [n], r2 f32 [n], q uint32 [n], K)"""
    p = np.ascontiguousarray(pts, F32)
    n = p.shape[0]
    K = min(int(knn_k), n)
    idx, d2 = knn(p, K)
    p64 = p.astype(np.float64)
    normals, gap = np.tile([0.0, 0.0, 1.0], (n, 1)), np.zeros(n)
    if K >= 3:
        for i in range(n):
            nb = p64[idx[i]]
            d = nb - nb.mean(axis=0)
            normals[i], gap[i] = normal_of(d.T @ d)
    rmax2, s = scale_of(max_radius)
    r2 = np.minimum(d2[:, K - 1], rmax2).astype(F32)
    q = (r2 * s).astype(np.uint32) if K >= 3 else np.zeros(n, np.uint32)
    return dict(normals=normals, gap=gap, r2=r2, q=q, K=K)


# ------------------------------------------------------------------------------------------------ allocation
def allocate(q, M, seed=0):
    """systematic allocation in Python integers -> (src_index int64 [M], Qt).  Qt == 0 raises ValueError."""
    Q, run = [], 0
    for v in np.asarray(q).tolist():
        run += int(v)
        Q.append(run)
    Qt = run
    if Qt == 0:
        raise ValueError("Qt == 0")
    r = (int(xi(seed, np.array([0]), 0)[0]) * Qt) >> 24           # the one offset of the call
    Qa = np.array(Q, np.uint64)
    u = [(j * Qt + r) // M for j in range(M)]
    assert 0 <= r < Qt and all(0 <= v < Qt for v in u)
    src = np.searchsorted(Qa, np.array(u, np.uint64), side="right").astype(np.int64)      # the first i with Q[i] > u
    return src, Qt


# ------------------------------------------------------------------------------------------------ placement
def basis64(n):
    """Duff et al.'s branch-free basis in fp64"""
    sign = math.copysign(1.0, n[2])
    a = -1.0 / (sign + n[2])
    b = n[0] * n[1] * a
    return (np.array([1.0 + sign * n[0] * n[0] * a, sign * b, -sign * n[0]]), np.array([b, sign + n[1] * n[1] * a, -n[1]]))


def patch_c(K):
    return F32(0.5 * math.sqrt(math.pi / K))


def place(pts, normals, r2, src, K, seed=0):
    """fp64 placement of the samples allocated to `src` -> (x f64 [M,3], rho2 f32 [M])"""
    M = len(src)
    a = (xi(seed, np.arange(M), 1).astype(np.float64) - 2.0 ** 23) * 2.0 ** -23
    b = (xi(seed, np.arange(M), 2).astype(np.float64) - 2.0 ** 23) * 2.0 ** -23
    c = float(patch_c(K))
    out = np.empty((M, 3))
    for j, i in enumerate(src):
        t1, t2 = basis64(np.asarray(normals[i], np.float64))
        h = math.sqrt(float(r2[i])) * c
        out[j] = np.asarray(pts[i], np.float64) + h * (a[j] * t1 + b[j] * t2)
    return out, np.asarray(r2, F32)[src]


# ------------------------------------------------------------------------------------------------ projection
def project(samples, rho2, pts, chunk=512):
    """one moving-least-squares step in fp64 -> dict(x f64 [M,3] (before the rounding to f32), count int [M], gap [M] (eigen-gap of the
    fitted covariance; 0 where the sample stayed), margin: the smallest |d2 - rho2| over every (sample, point) pair, in f32 units of rho2)"""
    x32, p32, rho2 = np.ascontiguousarray(samples, F32), np.ascontiguousarray(pts, F32), np.asarray(rho2, F32)
    M = x32.shape[0]
    out, count, gap, margin = x32.astype(np.float64), np.zeros(M, np.int64), np.zeros(M), np.inf
    p64 = p32.astype(np.float64)
    for a in range(0, M, chunk):
        d2 = d2_f32(x32[a:a + chunk], p32)
        near = d2 < rho2[a:a + chunk, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.abs(d2.astype(np.float64) - rho2[a:a + chunk, None].astype(np.float64)) / rho2[a:a + chunk, None].astype(np.float64)
        margin = min(margin, float(np.nanmin(rel))) if rel.size else margin
        for r in range(near.shape[0]):
            j = a + r
            nb = np.flatnonzero(near[r])
            count[j] = len(nb)
            if len(nb) < 3:
                continue
            t = 1.0 - d2[r, nb].astype(np.float64) / float(rho2[j])
            w = t * t
            e = p64[nb] - out[j]
            m = (w[:, None] * e).sum(axis=0) / w.sum()
            f = e - m
            C = (w[:, None] * f).T @ f
            if not C.any():
                continue
            nrm, gap[j] = normal_of(C)
            out[j] = out[j] + (m @ nrm) * nrm
    return dict(x=out, count=count, gap=gap, margin=margin)


def equalize(pts, num_points, knn_k=16, max_radius=1.0, do_project=True, seed=0):
    """the whole call, restated -> dict(x f64 [M,3], src int64 [M], surfels=...)"""
    s = surfels(pts, knn_k, max_radius)
    src, Qt = allocate(s["q"], num_points, seed)
    x, rho2 = place(np.asarray(pts, F32), s["normals"].astype(F32), s["r2"], src, s["K"], seed)
    if do_project:
        x = project(x.astype(F32), rho2, pts)["x"]
    return dict(x=x, src=src, Qt=Qt, surfels=s)


# ------------------------------------------------------------------------------------------------ judging
def angle(a, b):
    """unsigned angle between rows of a and b (atan2 of |cross| and |dot|)"""
    a, b = np.atleast_2d(np.asarray(a, np.float64)), np.atleast_2d(np.asarray(b, np.float64))
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(axis=1)))


GAP_FLOOR = 1e-3            # a normal is judged where (l1 - l0) / l2 >= GAP_FLOOR, and at least 90 % of a case must be


def normal_bound(gap):
    """angle a device normal may differ from `eigh`'s by: both sides work in fp64 on the same f32 points, so the covariances differ by
    ~K u relative (summation order) and the eigenvector by ~ that over the gap: ~1e-14 / gap; 1e-10 / gap leaves four decades (the
    1e-9 at gap 0.1 of tests/icp_plane_ref.py).  The f32 store of a unit vector adds at most sqrt(3) * 2^-25."""
    return 1e-10 / np.maximum(gap, 1e-300) + math.sqrt(3.0) * 2.0 ** -25


# ------------------------------------------------------------------------------------------------ clouds
def plane_cloud(n, rng, size=4.0, noise=0.0):
    p = np.zeros((n, 3))
    p[:, :2] = rng.uniform(-size / 2, size / 2, (n, 2))
    p[:, 2] = rng.normal(0.0, noise, n) if noise else 0.0
    return p.astype(F32)


def sphere_cloud(n, rng, radius=5.0):
    v = rng.normal(size=(n, 3))
    return (radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def corner_cloud(n, rng, size=3.0, shift=(0.0, 0.0, 0.0)):
    """two walls (x = 0 and y = 0) meeting in a corner"""
    uv = rng.uniform(0.0, size, (n, 2))
    wall = rng.randint(0, 2, n)
    p = np.zeros((n, 3))
    p[wall == 0] = np.stack([np.zeros((wall == 0).sum()), uv[wall == 0, 0], uv[wall == 0, 1]], axis=1)
    p[wall == 1] = np.stack([uv[wall == 1, 0], np.zeros((wall == 1).sum()), uv[wall == 1, 1]], axis=1)
    return (p + np.asarray(shift)).astype(F32)


def duplicate_cloud(n, rng, copies=3, places=10):
    """`places` locations hold `copies` identical points each; the rest are distinct"""
    p = plane_cloud(n, rng, size=2.0)
    for k in range(places):
        p[copies * k:copies * (k + 1)] = p[copies * k]
    return p[rng.permutation(n)]


def disc_cloud(n, rng, r_in=3.0, r_out=30.0):
    """a flat disc scanned with density ~ 1 / r^2: r log-uniform in [r_in, r_out]"""
    r = r_in * (r_out / r_in) ** rng.uniform(size=n)
    t = rng.uniform(0.0, 2.0 * np.pi, n)
    return np.stack([r * np.cos(t), r * np.sin(t), np.zeros(n)], axis=1).astype(F32)


def annulus_counts(xy, r_in=3.0, r_out=30.0, rings=10, drop_edges=True):
    """points per ring of `rings` equal-area annuli of [r_in, r_out]; drop_edges: without the innermost and the outermost (edge effects)"""
    r2 = (np.asarray(xy, np.float64)[:, :2] ** 2).sum(axis=1)
    edges = np.linspace(r_in ** 2, r_out ** 2, rings + 1)
    counts = np.histogram(r2, edges)[0]
    return counts[1:-1] if drop_edges else counts


def gpu_cases():
    """(name, pts, M, knn, max_radius): the smallest shapes that can still go wrong.  n in {3, 4, 63, 64, 65, 257, 1 025} and M in
    {1, 63, 64, 65, 1 000, 4 097} all occur."""
    rng = np.random.RandomState(20)
    return [
        ("plane", plane_cloud(1025, rng), 4097, 16, 1.0),
        ("sphere", sphere_cloud(257, rng), 1000, 16, 1.0),
        ("corner", corner_cloud(1025, rng), 1000, 16, 1.0),
        ("far", corner_cloud(257, rng, shift=(900.0, 0.0, 0.0)), 65, 16, 1.0),
        ("duplicates", duplicate_cloud(65, rng), 64, 3, 1.0),
        ("capped", plane_cloud(63, rng, size=8.0), 63, 16, 0.01),
        ("few_weights", plane_cloud(64, rng, size=1.0), 1000, 16, 51.2),          # Qt < M
        ("k_is_n_3", plane_cloud(3, rng, size=1.0), 1, 16, 1.0),                   # K = n < knn
        ("k_is_n_4", sphere_cloud(4, rng, radius=0.5), 63, 16, 1.0),
    ]


# ------------------------------------------------------------------------------------------------ csrc/equalize_math.h on the host
_exe = []


def host_program():
    """path of tests/equalize_math_host.cpp compiled with the compiler that builds the library, or None where there is none"""
    if _exe:
        return _exe[0]
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    exe = None
    if hipcc:
        tmp = tempfile.mkdtemp(prefix="equalize_math_host_")
        atexit.register(shutil.rmtree, tmp, True)
        exe = os.path.join(tmp, "equalize_math_host")
        subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", _build.CSRC,
                               "-I", _build.INCLUDE, os.path.join(REPO, "tests", "equalize_math_host.cpp"), "-o", exe])
    _exe.append(exe)
    return exe


def _fmt(v):
    return str(int(v)) if isinstance(v, (int, np.integer)) else float(v).hex()


def host_run(kind, rows, width, integers=False):
    """one record of `kind` per row through the host program -> [len(rows), width] (float64, or Python ints with integers=True).
    Integers cross in decimal, floats as hexadecimal floats: bit for bit."""
    text = "".join(kind + " " + " ".join(_fmt(v) for v in r) + "\n" for r in rows)
    out = subprocess.run([host_program()], input=text, capture_output=True, check=True, text=True).stdout.split("\n")
    lines = [ln.split() for ln in out if ln]
    assert len(lines) == len(rows) and all(len(ln) == width for ln in lines), (len(lines), len(rows))
    if integers:
        return [[int(v) for v in ln] for ln in lines]
    return np.array([[float.fromhex(v) for v in ln] for ln in lines], np.float64)


def host_place(pts, normals, r2, src, K, seed=0):
    """the f32 placement by the host-compiled header -> (t1, t2, x) f32 [M,3] each"""
    M = len(src)
    x1, x2 = xi(seed, np.arange(M), 1), xi(seed, np.arange(M), 2)
    c = patch_c(K)
    rows = [[*map(float, pts[i]), *map(float, normals[i]), float(r2[i]), float(c), int(x1[j]), int(x2[j])] for j, i in enumerate(src)]
    got = host_run("P", rows, 9)
    return got[:, 0:3].astype(F32), got[:, 3:6].astype(F32), got[:, 6:9].astype(F32)
