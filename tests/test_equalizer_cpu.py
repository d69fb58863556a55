"""CPU: the ground the sampling equalizer stands on -- csrc/equalize_math.h compiled for the host (tests/equalize_math_host.cpp) against
the restatement (tests/equalizer_ref.py) bit for bit, the quality of the integer mix, the allocation's counts, the refusals of the entries
and of the Python surface without a GPU, and what the contract is for: on the restatement, it equalizes a 1/r^2 density and its projection
takes noise off a plane."""
import inspect

import numpy as np
import pytest
import torch

import equalizer_ref as ref

F32 = np.float32


@pytest.fixture(scope="module")
def host():
    if ref.host_program() is None:
        pytest.skip("no hipcc found: csrc/equalize_math.h cannot be compiled here")
    return ref.host_run


# ---- the header on the host against the restatement ---------------------------------------------------------------------------------

def test_host_mix_and_allocation_bit_for_bit(host):
    rng = np.random.RandomState(0)
    rows = [(int(s), int(j), int(c)) for s in (0, 1, 0xFFFFFFFF, 12345) for j in (0, 1, 63, 64, 65535, (1 << 22) - 1) for c in (0, 1, 2)]
    got = host("X", rows, 1, integers=True)
    want = [int(ref.xi(s, np.array([j]), c)[0]) for s, j, c in rows]
    assert [g[0] for g in got] == want and max(want) < 1 << 24 and len(set(want)) == len(want)
    # lowbias32 is the published function: its value at 1 (computed by hand from the five steps) pins the constants
    assert int(ref.lowbias32(0)) == 0 and int(ref.lowbias32(1)) == _lowbias32_plain(1)
    # allocation at the edges of its ranges: Qt < M, Qt up to 2^22 * 65537, j = M - 1
    rows = []
    for Qt, M in ((1, 1), (5, 1000), (130, 1000), (1 << 22, 63), ((1 << 22) * 65537, 1 << 22), (987654321, 4097)):
        for j in sorted({0, min(1, M - 1), M // 2, M - 1}):
            rows.append((j, Qt, M, int(rng.randint(0, 1 << 24))))
            rows.append((j, Qt, M, (1 << 24) - 1))
    got = host("A", rows, 1, integers=True)
    for (j, Qt, M, x0), (u,) in zip(rows, got):
        r = (x0 * Qt) >> 24
        assert u == (j * Qt + r) // M and (j * Qt) // M <= u < Qt and r < Qt
    # the area weight: numpy float32 product, truncated
    r2 = np.concatenate([rng.uniform(0, 1, 200), [0.0, 1.0, 1e-12]]).astype(F32)
    for rmax in (1.0, 0.01, 51.2, 1000.0):
        _, s = ref.scale_of(rmax)
        rr = (r2 * F32(rmax) * F32(rmax)).astype(F32)
        got = host("Q", [(float(v), float(s)) for v in rr], 1, integers=True)
        assert [g[0] for g in got] == (rr * s).astype(np.uint32).tolist()


def _lowbias32_plain(x):
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_host_basis_placement_and_weight(host):
    """basis and placement bit for bit in f32 against numpy float32 arithmetic in the stated order; the basis orthonormal to f32
    rounding; a and b exact; the weight exact in fp64"""
    rng = np.random.RandomState(1)
    m = 400
    nrm = rng.normal(size=(m, 3))
    nrm[:6] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0, -1, -0.0], [0.6, 0.8, 0.0]]
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    pts = (rng.uniform(-50, 50, (m, 3)) + np.where(np.arange(m)[:, None] % 7 == 0, 900.0, 0.0)).astype(F32)
    r2 = rng.uniform(1e-4, 1.0, m).astype(F32)
    K, seed = 16, 7
    src = np.arange(m)
    t1, t2, x = ref.host_place(pts, nrm, r2, src, K, seed)
    # numpy float32, one rounding per operation, the header's parentheses
    one = F32(1.0)
    sign = np.copysign(one, nrm[:, 2])
    a_ = -one / (sign + nrm[:, 2])
    b_ = (nrm[:, 0] * nrm[:, 1]) * a_
    w1 = np.stack([one + ((sign * nrm[:, 0]) * nrm[:, 0]) * a_, sign * b_, -sign * nrm[:, 0]], axis=1)
    w2 = np.stack([b_, sign + (nrm[:, 1] * nrm[:, 1]) * a_, -nrm[:, 1]], axis=1)
    assert w1.dtype == F32 and np.array_equal(t1.view(np.uint32), w1.view(np.uint32)) and np.array_equal(t2.view(np.uint32), w2.view(np.uint32))
    a = ((ref.xi(seed, src, 1).astype(np.int64) - (1 << 23)).astype(F32) * F32(2.0 ** -23))
    b = ((ref.xi(seed, src, 2).astype(np.int64) - (1 << 23)).astype(F32) * F32(2.0 ** -23))
    assert np.array_equal(a.astype(np.float64), (ref.xi(seed, src, 1).astype(np.float64) - 2.0 ** 23) * 2.0 ** -23)      # exact
    h = np.sqrt(r2) * ref.patch_c(K)
    want = pts + h[:, None] * ((a[:, None] * w1) + (b[:, None] * w2))
    assert want.dtype == F32 and np.array_equal(x.view(np.uint32), want.view(np.uint32))
    # orthonormal to f32 rounding, and right-handed: t1 x t2 = n
    t1d, t2d, nd = t1.astype(np.float64), t2.astype(np.float64), nrm.astype(np.float64)
    assert np.abs((t1d * t2d).sum(1)).max() < 4e-7 and np.abs((t1d * nd).sum(1)).max() < 4e-7 and np.abs((t2d * nd).sum(1)).max() < 4e-7
    assert np.abs(np.linalg.norm(t1d, axis=1) - 1).max() < 4e-7 and np.abs(np.cross(t1d, t2d) - nd).max() < 1e-6
    # the fp64 placement of the restatement is the same point to f32 rounding of its terms
    x64, _ = ref.place(pts, nrm, r2, src, K, seed)
    assert np.abs(x.astype(np.float64) - x64).max() <= 4 * float(np.spacing(F32(950.0)))
    # weight and predicate distance
    d2 = rng.uniform(0, 1, 100).astype(F32)
    rho2 = (d2 + rng.uniform(1e-6, 1, 100)).astype(F32)
    got = host("W", list(zip(d2.tolist(), rho2.tolist())), 1)[:, 0]
    t = 1.0 - d2.astype(np.float64) / rho2.astype(np.float64)
    assert np.array_equal(got, t * t)
    d = rng.normal(size=(100, 3)).astype(F32)
    got = host("D", d.tolist(), 1)[:, 0]
    assert np.array_equal(got.astype(F32), (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


# ---- the mix is usable ----------------------------------------------------------------------------------------------------------------

CHI2_255_Q9999 = 347.65      # the 1 - 1e-4 quantile of chi-square with 255 degrees of freedom


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEF])
def test_mix_is_usable(seed):
    """for j < 65 536 each stream's top byte passes a 256-bin chi-square at the 1 - 1e-4 quantile, and xi1 / xi2 are uncorrelated
    within 4 sigma = 4 / sqrt(65 536)"""
    j = np.arange(65536)
    streams = [ref.xi(seed, j, c) for c in range(3)]
    for c, x in enumerate(streams):
        counts = np.bincount((x >> np.uint64(16)).astype(np.int64), minlength=256)
        chi2 = float(((counts - 256.0) ** 2 / 256.0).sum())
        print(f"[mix seed={seed:#x} c={c}] chi2 {chi2:.1f} (255 dof, gate {CHI2_255_Q9999})")
        assert chi2 < CHI2_255_Q9999
    r = float(np.corrcoef(streams[1].astype(np.float64), streams[2].astype(np.float64))[0, 1])
    print(f"[mix seed={seed:#x}] corr(xi1, xi2) {r:+.5f} (4 sigma = {4 / 256.0:.5f})")
    assert abs(r) < 4.0 / 256.0


# ---- allocation -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def disc():
    """the flat disc, 3 m <= r <= 30 m, 20 000 points of density ~ 1/r^2, equalized to 20 000 samples by the restatement (a flat cloud:
    the projection moves nothing off its plane and is left out).  max_radius = 3 m: 20 000 points on 2 800 m^2 are a sixth of a real
    scan's density, the 16th neighbour of a rim point is 1.8 m away, and a cap below that stops the equalization where it bites (with the
    default 1 m: every support beyond r = 16 m, output ratio 2.62) -- the cap is there to bound the patches of stray points, not to be
    the rule."""
    pts = ref.disc_cloud(20000, np.random.RandomState(5))
    return pts, ref.equalize(pts, 20000, max_radius=3.0, do_project=False)


def _shares(disc):
    _, eq = disc
    q = eq["surfels"]["q"].astype(np.int64)
    counts = np.bincount(eq["src"], minlength=len(q))
    return q, counts, 20000 * q.astype(np.float64) / float(eq["Qt"])


def test_allocation_counts(disc):
    """the counts sum to M and a point without area is never chosen"""
    q, counts, _ = _shares(disc)
    assert counts.sum() == 20000 and q.sum() == disc[1]["Qt"] and not counts[q == 0].any()
    src, _ = ref.allocate(np.array([0, 5, 0, 0, 7, 0], np.uint32), 1000, seed=3)
    assert set(src.tolist()) == {1, 4} and abs(int((src == 1).sum()) - 1000 * 5 / 12) < 1


def test_allocation_within_one_of_its_share(disc):
    """|count_i - M q_i / Qt| < 1 for every i.  Derivation: point i owns the integer interval [Q[i-1], Q[i]) of length q_i; u_j is the
    floor of the real comb (j + r / Qt) Qt / M, whose teeth are Qt / M apart, and an integer interval holds floor(x) exactly when it
    holds x: it holds the floor or the ceiling of q_i M / Qt teeth.  Measured on this disc (n = M = 20 000): 0.988."""
    q, counts, share = _shares(disc)
    off = np.abs(counts - share)
    print(f"[allocation] max |count - share| {float(off.max()):.4f}, {int((off >= 1).sum())} of {len(q)} points at or beyond 1")
    assert float(off.max()) < 1.0
    assert ((counts == np.floor(share)) | (counts == np.ceil(share))).all()


# ---- it equalizes ---------------------------------------------------------------------------------------------------------------------

RESTATEMENT_RATIO = 1.054    # max / min count over the 8 inner annuli of the disc's output, measured on the restatement
EQUALIZED_GATE = 1.5 * RESTATEMENT_RATIO


def test_it_equalizes(disc):
    """10 equal-area annuli of the disc: the input's max / min count ratio is above 10; the output's, with the innermost and the outermost
    annulus dropped (edge effects: patches of border points reach over the rim, and nothing beyond it reaches back), is gated at 1.5 x the
    value measured on the restatement, a gate that is never looser than 2.0.  The input has no edge effect and is judged on all ten rings:
    a density of exactly 1 / r^2 puts ln(r_out / r_in) of each ring into it, 23 : 1 between the first and the last ring but only 5.4 : 1
    between the second and the ninth, so "above 10" can only be meant of the ten."""
    pts, eq = disc
    call, cout = ref.annulus_counts(pts, drop_edges=False), ref.annulus_counts(eq["x"])
    cin = call[1:-1]
    rin, rout = call.max() / call.min(), cout.max() / cout.min()
    print(f"[disc] input counts {call.tolist()} ratio {rin:.2f} (inner eight: {cin.max() / cin.min():.2f}); output counts {cout.tolist()} "
          f"ratio {rout:.3f} (gate {EQUALIZED_GATE:.3f})")
    assert EQUALIZED_GATE <= 2.0
    assert rin > 10.0
    assert rout <= EQUALIZED_GATE
    assert np.abs(eq["x"][:, 2]).max() == 0.0          # a flat cloud stays flat: every patch lies in its plane


def test_projection_takes_noise_off_a_plane():
    """a plane with 1 cm Gaussian noise, project=True: the samples' rms distance to the plane is below the input's"""
    pts = ref.plane_cloud(2000, np.random.RandomState(6), size=4.0, noise=0.01)
    eq = ref.equalize(pts, 2000, do_project=True)
    rms_in = float(np.sqrt((pts[:, 2].astype(np.float64) ** 2).mean()))
    rms_out = float(np.sqrt((eq["x"][:, 2] ** 2).mean()))
    print(f"[noisy plane] rms distance to the plane: input {1e3 * rms_in:.2f} mm, samples {1e3 * rms_out:.2f} mm, ratio {rms_out / rms_in:.3f}")
    assert rms_out / rms_in < 1.0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_entries_check_arguments_before_the_device():
    from umeregrobust_amd import _lib, equalizer
    lib = equalizer.load_native()
    assert lib is _lib.load()
    buf = np.zeros(1 << 16, dtype=np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 256
    big = (1 << 22) + 1
    size = lib.umereg_equalize_workspace_bytes
    assert size(0, 10, 16) == 0 and size(10, 0, 16) == 0 and size(10, 10, 2) == 0 and size(10, 10, 65) == 0
    assert size(big, 10, 16) == 0 and size(10, big, 16) == 0 and size(1 << 22, 1 << 22, 64) > 0
    assert size(1000, 125000, 16) > size(1000, 1, 16) > size(1000, 1, 3) > 0
    surf = lambda **kw: lib.umereg_equalize_surfels_f32(*[kw.get(k, d) for k, d in (                                   # noqa: E731
        ("pts", p), ("n", 100), ("knn", 16), ("r", 1.0), ("nrm", p), ("r2", p), ("q", p), ("ws", p), ("nws", 1 << 16), ("st", None))])
    for kw in (dict(pts=None), dict(q=None), dict(n=0), dict(n=big), dict(knn=2), dict(knn=65), dict(r=0.0), dict(r=-1.0),
               dict(r=float("nan")), dict(r=1e4)):
        assert surf(**kw) == -1, kw
    samp = lambda **kw: lib.umereg_equalize_sample_f32(*[kw.get(k, d) for k, d in (                                    # noqa: E731
        ("pts", p), ("nrm", p), ("r2", p), ("q", p), ("n", 100), ("M", 50), ("knn", 16), ("seed", 0), ("x", p), ("src", p), ("rho2", p),
        ("tot", p), ("ws", p), ("nws", 1 << 16), ("st", None))])
    for kw in (dict(q=None), dict(tot=None), dict(M=0), dict(M=big), dict(n=big), dict(knn=1)):
        assert samp(**kw) == -1, kw
    assert samp(n=2) == -1 and b"Qt == 0" in lib.umereg_last_error()           # fewer than three points: no area anywhere
    proj = lambda **kw: lib.umereg_equalize_project_f32(*[kw.get(k, d) for k, d in (                                   # noqa: E731
        ("x", p), ("rho2", p), ("pts", p), ("M", 50), ("n", 100), ("out", p), ("cnt", None), ("ws", p), ("nws", 1 << 16), ("st", None))])
    for kw in (dict(x=None), dict(out=None), dict(M=0), dict(n=0), dict(M=big)):
        assert proj(**kw) == -1, kw
    whole = lambda **kw: lib.umereg_equalize_cloud_f32(*[kw.get(k, d) for k, d in (                                    # noqa: E731
        ("pts", p), ("n", 100), ("M", 50), ("knn", 16), ("r", 1.0), ("project", 1), ("seed", 0), ("out", p), ("src", p), ("tot", p),
        ("ws", p), ("nws", 1 << 16), ("st", None))])
    for kw in (dict(pts=None), dict(src=None), dict(n=2), dict(n=big), dict(M=big), dict(knn=65), dict(r=0.0)):
        assert whole(**kw) == -1, kw
    assert b"equalize_cloud" in lib.umereg_last_error()
    if lib.umereg_device_count(None, 0) == 0:
        assert surf() == -2 and samp() == -2 and proj() == -2 and whole() == -2        # UMEREG_ENODEV


def test_python_surface_without_a_gpu():
    from umeregrobust_amd import equalizer, ops
    pts = torch.zeros(10, 3)
    assert ops.equalize_cloud is equalizer.equalize_cloud
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        equalizer.equalize_cloud(pts)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        equalizer.sampling_equalizer(pts)
    for knn in (2, 65, 3.5, True, "16"):
        with pytest.raises(ValueError, match="knn"):
            equalizer.equalize_cloud(pts, knn=knn)
        with pytest.raises(ValueError, match="knn"):
            equalizer.make_equalizer(knn=knn)
    for m in (0, -1, (1 << 22) + 1, 2.5, True):
        with pytest.raises(ValueError, match="num_points"):
            equalizer.equalize_cloud(pts, num_points=m)
    for r in (0.0, -1.0, float("nan"), 1e4, True, None):
        with pytest.raises(ValueError, match="max_radius"):
            equalizer.equalize_cloud(pts, max_radius=r)
    for s in (-1, 1 << 32, 0.5, True):
        with pytest.raises(ValueError, match="seed"):
            equalizer.equalize_cloud(pts, seed=s)
    with pytest.raises(ValueError, match=r"\[n,3\]"):
        equalizer.equalize_cloud(torch.zeros(10, 4))
    with pytest.raises(ValueError, match="Qt"):
        equalizer.equalize_cloud(torch.zeros(2, 3))
    with pytest.raises(ValueError, match="unknown"):
        equalizer.make_equalizer(radius=2.0)
    sig = inspect.signature(equalizer.equalize_cloud).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("num_points", 125000), ("knn", 16), ("max_radius", 1.0), ("project", True),
                                                           ("seed", 0), ("return_index", False)]
    assert callable(equalizer.make_equalizer(num_points=1000, knn=8, max_radius=0.5, project=False, seed=3))
    # the entries are the module's own table, typed through load_typed; none of them is in the package tables of include/
    from umeregrobust_amd import _lib
    assert len(equalizer.EQUALIZE_SIGNATURES) == 5 and not set(equalizer.EQUALIZE_SIGNATURES) & {n for t in _lib.TABLES.values() for n in t}
    assert any(t is equalizer.EQUALIZE_SIGNATURES for t in _lib._typed) or equalizer.load_native() is _lib.load()


def test_completion_missing_is_still_raised_without_a_function():
    from umeregrobust_amd import raw_scan
    with pytest.raises(NotImplementedError, match="NKSR.*completion_fn.*sampling_equalizer"):
        raw_scan.complete_cloud(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64), None)
    assert isinstance(raw_scan.completion_missing(), NotImplementedError)
