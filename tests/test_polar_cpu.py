"""polar_rotation (umeregrobust_amd/csrc/polar.h) against a true SVD, without a GPU.

Every transform the library returns goes through this routine (rtume_kernel: every hypothesis; icp_step_kernel: every Umeyama update).
oracle/polar_host.cpp compiles the very header the kernels include for the host; the tests below drive it over constructed
A = s U diag(sigma) V^T (U, V random proper rotations, a negative determinant through -s3) and compare with

    R_truth = U diag(1, 1, sign det(U Vh)) Vh        from an SVD of A.

The truth.  numpy's fp64 SVD is itself only good to about `bound` (below), which at s2/s1 <= 1e-6 is not a tenth of a 1e-9 bar.  So
where mpmath is importable the truth is mpmath's SVD of the same fp64 matrix at 50 digits, and it is trusted only where a second
50-digit route that shares no code with it (the symmetric eigen-solve of A^T A -- squaring is harmless at 50 digits -- with u_i = A v_i / s_i)
agrees to a tenth of the case's bar; numpy's fp64 SVD must agree with it too, to a tenth of the bar or to 4 * bound, its own reach.
Without mpmath the truth is numpy's SVD of A, confirmed by the SVDs of A^T and of a cyclically row-permuted A to a tenth of the bar.
A case whose truth is not confirmed is not judged element-wise, and the tests ASSERT that no case with a gap is lost that way.

Judgement (u = 2^-53, gap = s2 + det * s3, bound = u |A|_F / gap: the problem's own first-order sensitivity)
  element-wise  every case with a gap:  max |R - R_truth| <= max(1e-9, 4 * bound).  1e-9 is the bar the ICP holds against its oracle,
              and it is THE bar wherever an fp64 route can reach it: all of s2/s1 >= 1e-6.  Only at s2/s1 = 1e-7 does the problem's
              own bound pass it (1.1e-9 / (1 + det s3/s2), up to 2.2e-9), and there the bar is 4 * bound.  The factor is not taken
              from the routine: a backward-stable 3x3 route perturbs A by about u |A|_F per sweep of orthogonal updates and needs
              3-4 sweeps, so it errs by <= ~4 * bound, while a route that squares the spectrum errs by u (s1/s2)^2 = 1e7 * bound there;
  by value    (every case, with or without a gap) R orthonormal with det R = +1 to 1e-12, and trace(R^T A) within 64 u |A|_F of its
              optimum s1 + s2 + det * s3.  R = U diag(1, 1, det) Vh is the maximiser of trace(R^T A) over rotations
              (R^T A = V D S V^T), so this is the objective in the routine's own orientation; it is indifferent to which optimal
              rotation an ambiguous case (gap == 0) returns and still refuses a wrong one;
  ill-posed   gap == 0, or so small that 4 * bound >= 0.1 says nothing: by value only.
Scaling by a power of two is exact in fp64, so the truth of s * A is the truth of A: the mpmath work is done once per matrix.
"""
import itertools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import polar_cases as pc
from tests.polar_cases import R2 as _R2, R3 as _R3, compose as _compose, ladder_cell, rot as _rot

_U64 = 2.0 ** -53
_BAR = 1e-9
_SLACK = 4.0                       # bar = max(_BAR, _SLACK * bound): see the module docstring
_SCALES = [2.0 ** -60, 2.0 ** -20, 1.0, 2.0 ** 20, 2.0 ** 60]
_N = 50                            # matrices per cell

try:
    import mpmath
except ImportError:                # pragma: no cover
    mpmath = None


def _truth_numpy(A):
    U, S, Vh = np.linalg.svd(A)
    d = np.sign(np.linalg.det(U @ Vh))
    D = np.tile(np.eye(3), (A.shape[0], 1, 1))
    D[:, 2, 2] = d
    return U @ D @ Vh, S, d


def _mp_rotation(U, V):
    """columns u0, u1 of U and v0, v1 of V (mpmath) -> u0 v0^T + u1 v1^T + (u0 x u1)(v0 x v1)^T as fp64"""
    cr = lambda a, b: mpmath.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])  # noqa: E731
    u0, u1, v0, v1 = U[:, 0], U[:, 1], V[:, 0], V[:, 1]
    R = u0 * v0.T + u1 * v1.T + cr(u0, u1) * cr(v0, v1).T
    return np.array(R.tolist(), dtype=np.float64)


def _truths(A):
    """-> (R_truth, [other routes' R]) for each A[i]; see the module docstring"""
    Rn = _truth_numpy(A)[0]
    if mpmath is None:                                                        # pragma: no cover
        cyc = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float64)         # det +1: R(P A) = P R(A)
        Rt = np.swapaxes(_truth_numpy(np.ascontiguousarray(np.swapaxes(A, 1, 2)))[0], 1, 2)
        return Rn, [Rt, cyc.T @ _truth_numpy(cyc @ A)[0]], None
    R1, R2 = np.empty_like(A), np.empty_like(A)
    with mpmath.workdps(50):
        for i, a in enumerate(A):
            M = mpmath.matrix(a.tolist())
            U, _, Vh = mpmath.svd_r(M)
            R1[i] = _mp_rotation(U, Vh.T)
            _, Q = mpmath.eigsy(M.T * M)                                      # eigenvalues ascending
            V = mpmath.matrix(3, 2)
            W = mpmath.matrix(3, 2)
            for k in range(2):
                V[:, k] = Q[:, 2 - k]
                w = M * V[:, k]
                W[:, k] = w / mpmath.norm(w)
            R2[i] = _mp_rotation(W, V)
    return R1, [R2], Rn


def _judge(A, tag, report=None, must_hold_1e9=None, must_be_elementwise=None):
    """Judge polar_rotation on A [n,3,3] at every scale.  -> list of failure strings (empty = pass); fills report[tag] with maxima.
    must_hold_1e9 / must_be_elementwise: optional bool [n]; those cases must end up judged element-wise to the 1e-9 bar / element-wise
    at all (none may drop out through its bound or through the truth's cross-check)."""
    A = np.ascontiguousarray(A, np.float64).reshape(-1, 3, 3)
    n = A.shape[0]
    Rt, S, d = _truth_numpy(A)
    fro = np.sqrt((A * A).sum(axis=(1, 2)))
    gap = S[:, 1] + d * S[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(gap > 0, _U64 * fro / gap, np.inf)
    bar = np.maximum(_BAR, _SLACK * bound)
    elementwise = bar < 0.1                                            # beyond that |dR| <= bar says nothing
    fails = {}                                                         # (tag, kind) -> [first message, how many scales]

    def fail(kind, msg):
        fails.setdefault((tag, kind), [msg, 0])[1] += 1

    # the truth, cross-checked
    idx = np.flatnonzero(elementwise)
    if idx.size:
        R1, others, Rn = _truths(A[idx])
        Rt = Rt.copy()
        Rt[idx] = R1
        dis = np.max([np.abs(Ro - R1).max(axis=(1, 2)) for Ro in others], axis=0)
        trusted = dis <= 0.1 * bar[idx]
        if Rn is not None:
            trusted &= np.abs(Rn - R1).max(axis=(1, 2)) <= np.maximum(0.1 * bar[idx], _SLACK * bound[idx])
        if not trusted.all():
            w = idx[~trusted][np.argmax((dis / bar[idx])[~trusted])]
            fail("truth", f"{tag}: {int((~trusted).sum())} of {idx.size} truths not confirmed by the other routes "
                          f"(worst case {w}: bar {bar[w]:.1e})")
        elementwise[idx[~trusted]] = False
    at_1e9 = elementwise & (bar == _BAR)
    if must_hold_1e9 is not None and (np.asarray(must_hold_1e9) & ~at_1e9).any():
        lost = np.asarray(must_hold_1e9) & ~at_1e9
        fail("lost 1e-9", f"{tag}: {int(lost.sum())} cases that must be held to {_BAR:.0e} are not (bound max {bound[lost].max():.2e})")
    if must_be_elementwise is not None and (np.asarray(must_be_elementwise) & ~elementwise).any():
        lost = np.asarray(must_be_elementwise) & ~elementwise
        fail("lost", f"{tag}: {int(lost.sum())} cases with a gap are not judged element-wise (bound max {bound[lost].max():.2e})")
    opt = S[:, 0] + S[:, 1] + d * S[:, 2]
    rep = dict(n=n, at_1e9=int(at_1e9.sum()), at_4_bounds=int((elementwise & ~at_1e9).sum()), dR_at_1e9=0.0, dR_beyond=0.0,
               dR_over_bound=0.0, value=0.0, ortho=0.0)
    for s in _SCALES:
        R = orc.polar_rotation_host(A * s)
        if not np.isfinite(R).all():
            fail("finite", f"{tag} scale {s:.0e}: non-finite R")
            continue
        ortho = np.maximum(np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max(axis=(1, 2)), np.abs(np.linalg.det(R) - 1.0))
        val = np.abs(np.einsum("nij,nij->n", R, A) - opt) / np.where(fro > 0, fro, 1.0) / _U64
        dR = np.abs(R - Rt).max(axis=(1, 2))
        rep["ortho"] = max(rep["ortho"], float(ortho.max()))
        rep["value"] = max(rep["value"], float(val.max()))
        rep["dR_at_1e9"] = max(rep["dR_at_1e9"], float(dR[at_1e9].max(initial=0.0)))
        rep["dR_beyond"] = max(rep["dR_beyond"], float(dR[elementwise & ~at_1e9].max(initial=0.0)))
        thin = elementwise & (bound > 1e-13)                            # (below that the ratio is rounding of R's entries over ~0)
        rep["dR_over_bound"] = max(rep["dR_over_bound"], float((dR / bound)[thin].max(initial=0.0)))
        if ortho.max() > 1e-12:
            fail("rotation", f"{tag} scale {s:.0e}: R not a rotation to 1e-12 ({ortho.max():.2e}, case {ortho.argmax()})")
        if val.max() > 64.0:
            fail("value", f"{tag} scale {s:.0e}: trace(R^T A) off its optimum by {val.max():.3g} u |A|_F (case {val.argmax()})")
        bad = elementwise & (dR > bar)
        if bad.any():
            w = np.flatnonzero(bad)[np.argmax((dR / bar)[bad])]
            fail("bar", f"{tag} scale {s:.0e}: {int(bad.sum())} of {int(elementwise.sum())} over the bar; worst |dR| {dR[w]:.2e} "
                        f"> {bar[w]:.2e} (bound {bound[w]:.2e}, case {w}); max |dR| {dR[elementwise].max():.2e}")
    if report is not None:
        report[tag] = rep
    return [msg + (f"   [and at {k - 1} more scales]" if k > 1 else "") for msg, k in fails.values()]


@pytest.mark.parametrize("r2", _R2, ids=[f"s2/s1={r:.0e}" for r in _R2])
def test_sigma_ladder(r2):
    """s2/s1 = r2 x s3/s2 in {1, .5, .1, 1e-3, 0} x det +-, 50 matrices a cell, five scales.  Every cell with a gap is judged
    element-wise, and every such cell of s2/s1 >= 1e-6 to 1e-9 -- asserted from the cell's own sigma, so that none can drop out of
    that class; the cells of s2/s1 = 1e-7 (bound 0.55e-9 .. 2.2e-9) to 4 * bound."""
    fails, report = [], {}
    for r3, det in itertools.product(_R3, (1, -1)):
        A = ladder_cell(r2, r3, det)
        gap = r2 * (1.0 + det * r3)
        fro = np.sqrt(1.0 + r2 ** 2 + (r2 * r3) ** 2)
        has_gap = gap > 0
        at_1e9 = has_gap and _SLACK * _U64 * fro * 1.001 / gap <= _BAR
        assert at_1e9 == (has_gap and r2 >= 1e-6), (r2, r3, det)
        fails += _judge(A, f"s3/s2={r3:g} det={det:+d}", report, must_hold_1e9=np.full(A.shape[0], at_1e9),
                        must_be_elementwise=np.full(A.shape[0], has_gap))
    for k, v in report.items():
        print(f"[polar ladder s2/s1={r2:.0e}] {k}: {v}")
    assert not fails, "\n".join(fails)


def test_no_ladder_cell_is_lost():
    """Every cell of the ladder with a gap -- down to s2/s1 = 1e-7, s3 = s2 with det > 0 included -- has a truth that both routes
    confirm to a tenth of its bar, so every such case is judged element-wise."""
    for r2, r3, det in itertools.product(_R2, _R3, (1, -1)):
        if r3 == 1.0 and det == -1:
            continue                                                    # gap = 0: judged by value
        A = ladder_cell(r2, r3, det, n=8)
        Rt, S, d = _truth_numpy(A)
        gap = S[:, 1] + d * S[:, 2]
        bound = _U64 * np.sqrt((A * A).sum(axis=(1, 2))) / gap
        assert (gap > 0).all() and (_SLACK * bound < 0.1).all()
        bar = np.maximum(_BAR, _SLACK * bound)
        R1, others, Rn = _truths(A)
        for Ro in others:
            assert (np.abs(Ro - R1).max(axis=(1, 2)) <= 0.1 * bar).all(), (r2, r3, det)
        if Rn is not None:
            assert (np.abs(Rn - R1).max(axis=(1, 2)) <= np.maximum(0.1 * bar, _SLACK * bound)).all(), (r2, r3, det)


def test_ties():
    rng = np.random.RandomState(101)
    fails, report = [], {}
    for r3, det in itertools.product([0.9, 0.5, 1e-3, 0.0], (1, -1)):                      # s1 = s2 > s3: R is determined, u_i, v_i are not
        A = np.stack([_compose(_rot(rng), [1.0, 1.0, r3], _rot(rng), det) for _ in range(_N)])
        fails += _judge(A, f"s1=s2 s3={r3:g} det={det:+d}", report, must_hold_1e9=np.ones(_N, bool))
    Q = np.stack([_rot(rng) for _ in range(_N)])
    c = rng.uniform(0.5, 2.0, (_N, 1, 1))
    fails += _judge(c * Q, "multiples of a rotation", report, must_hold_1e9=np.ones(_N, bool))
    fails += _judge(Q, "exact rotations", report, must_hold_1e9=np.ones(_N, bool))
    M = np.diag([1.0, 1.0, -1.0])
    fails += _judge(c * (Q @ M @ np.swapaxes(Q[::-1], 1, 2)), "multiples of a reflection (gap = 0: by value)", report)
    fails += _judge(np.stack([np.diag([1.0, 1, -1]), np.diag([-1.0, 1, 1]), np.diag([1.0, -1, 1]), -np.eye(3), -3 * np.eye(3)]),
                    "axis reflections, -I", report)
    for k, v in report.items():
        print(f"[polar ties] {k}: {v}")
    assert not fails, "\n".join(fails)


def test_special_matrices():
    rng = np.random.RandomState(102)
    fails, report = [], {}
    iv = lambda: rng.randint(-9, 10, 3).astype(np.float64)                                # noqa: E731  small integers: exact products
    rank2 = np.stack([np.outer(iv(), iv()) + np.outer(iv(), iv()) for _ in range(_N)])
    rank2 = rank2[np.linalg.matrix_rank(rank2) == 2]
    fails += _judge(rank2, "exact rank 2 (integers)", report)
    rank1 = np.stack([np.outer(iv(), iv()) for _ in range(_N)])
    rank1 = rank1[np.abs(rank1).max(axis=(1, 2)) > 0]
    fails += _judge(rank1, "exact rank 1 (integers: gap = 0, by value)", report)
    e = np.eye(3)
    fails += _judge(np.stack([np.outer(e[i], e[j]) * s for i in range(3) for j in range(3) for s in (1.0, -2.0)]),
                    "rank 1 on the axes", report)
    for k, v in report.items():
        print(f"[polar special] {k}: {v}")
    assert not fails, "\n".join(fails)
    for s in _SCALES + [0.0]:                                                                 # A = 0 -> I, exactly (LAPACK's U = V = I)
        Z = np.zeros((1, 3, 3))
        assert np.array_equal(orc.polar_rotation_host(Z * s)[0], np.eye(3))
    # denormal-sized input: still a rotation (nothing to compare element-wise: the products of the entries underflow)
    R = orc.polar_rotation_host(np.stack([_rot(rng) for _ in range(8)]) * 2.0 ** -1040)
    assert np.isfinite(R).all() and np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 1e-12


def test_diagonal_and_permutation_matrices():
    """Zero off-diagonal products from the start (the rotation's early return) in every eigenvalue order and sign pattern."""
    fails, report = [], {}
    mats = []
    for perm in itertools.permutations(range(3)):
        P = np.eye(3)[list(perm)]
        for sig in ([3.0, 2.0, 1.0], [1.0, 1e-3, 1e-6], [1.0, 1.0, 0.5], [2.0, 1.0, 1.0], [1.0, 0.25, 0.0], [1.0, 1.0, 1.0]):
            for order in itertools.permutations(range(3)):
                for signs in itertools.product((1.0, -1.0), repeat=3):
                    mats.append(P @ np.diag(np.asarray(sig)[list(order)] * signs))
    A = np.stack(mats)
    fails += _judge(A, "signed, permuted diagonals", report)
    for k, v in report.items():
        print(f"[polar diagonal] {k}: {v}")
    assert not fails, "\n".join(fails)


def test_dominant_right_singular_vector_on_each_axis():
    """v1 = +-e_k exactly and nearly, with the other two in either order: every branch of the selection of the two dominant pairs."""
    rng = np.random.RandomState(103)
    fails, report = [], {}
    for perm in itertools.permutations(range(3)):
        P = np.eye(3)[:, list(perm)]
        for sig in ([1.0, 0.3, 0.1], [1.0, 1e-4, 1e-5], [1.0, 0.999, 1e-3]):
            for det in (1, -1):
                mats = []
                for i in range(_N):
                    V = P * rng.choice([-1.0, 1.0], 3)
                    if np.linalg.det(V) < 0:
                        V[:, 2] = -V[:, 2]
                    if i % 2:                                                           # nearly on the axis
                        w = rng.normal(size=3) * 10.0 ** rng.uniform(-12, -3)
                        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
                        V = V @ (np.eye(3) + K + K @ K / 2)
                        V = np.linalg.qr(V)[0] * np.sign(np.diag(np.linalg.qr(V)[1]))
                    mats.append(_compose(_rot(rng), sig, V, det))
                fails += _judge(np.stack(mats), f"v order {perm} sigma {sig} det={det:+d}", report)
    worst = max(report.values(), key=lambda v: v["dR_over_bound"])
    print(f"[polar dominant axis] {len(report)} cells; worst {worst}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ the GPU ladders' inputs (tests/test_polar_gpu.py), checked here
def test_rtume_ladder_inputs_realise_the_spectrum_and_qualify():
    """The constructed UME pairs have the prescribed cross-moment spectrum AFTER their fp32 rounding (s2/s1 to 0.1 %, and s3/s2 to 2 %
    where s3 is above the rounding left by the shift), and every hypothesis of a cell with a gap qualifies for the RTUME bars by the
    problem's bound alone -- so the GPU ladder judges the whole ladder, both families."""
    u64 = 2.0 ** -53
    for family in ("plain", "shift"):
        G, H, cell = pc.rtume_ladder(4097, family)
        T, cf = orc.batch_estimate_transform_ume_f64(G, H)
        tn = np.linalg.norm(T[:, :3, 3], axis=1)
        assert (tn.max() == 0.0) if family == "plain" else (100.0 < tn.max() <= 145.0)
        r2, r3, det = (np.array([pc.CELLS[c][k] for c in cell]) for k in range(3))
        assert np.bincount(cell, minlength=len(pc.CELLS)).min() >= 50
        assert np.abs(cf.s[:, 1] / cf.s[:, 0] / r2 - 1.0).max() <= 1e-3
        big3 = r3 >= 1e-1
        assert np.abs((cf.s[:, 2] / cf.s[:, 1])[big3] / r3[big3] - 1.0).max() <= 2e-2
        qual = (cf.kappa_R_problem <= 1e-8 / u64) & (cf.kappa_t_problem <= 1e-7 / u64 * np.maximum(1.0, tn))
        has_gap = ~((r3 == 1.0) & (det == -1))
        assert qual[has_gap].all(), (family, int((~qual & has_gap).sum()))
        # and what the old gate's extra term would have excused: every rung below s2/s1 ~ 1e-4
        excused = (cf.kappa_R > 1e-8 / u64) & has_gap
        assert excused[(r2 <= 1e-5) & has_gap].all() and not excused[r2 >= 1e-3].any()


def test_icp_thin_cases_are_what_they_claim():
    """identity pairing at full fitness; the covariance's bound puts w = 1 m, 0.1 m and the plane inside the 1e-9 bar's reach"""
    u64 = 2.0 ** -53
    for kind, w, judged in (("segment", 1.0, True), ("segment", 0.1, True), ("segment", 0.02, False), ("segment", 0.005, False),
                            ("planar", 0.0, True), ("collinear", 0.0, False)):
        src, tgt, T0, max_dist = pc.icp_thin_case(kind, w)
        idx, fit, _, q = orc.icp_evaluate(src, tgt, T0, max_dist)
        assert fit == 1.0 and np.unique(idx).size == idx.size
        d = np.linalg.norm(tgt[:, None].astype(np.float64) - tgt[None].astype(np.float64), axis=2) + 1e9 * np.eye(tgt.shape[0])
        assert d.min() >= 10 * np.linalg.norm(q - tgt[idx], axis=1).max()              # the motion is far below the point spacing
        q_ = tgt.astype(np.float64)[idx]
        cov = (q_ - q_.mean(0)).T @ (q - q.mean(0)) / idx.size
        U, S, Vt = np.linalg.svd(cov)
        gap = S[1] + np.sign(np.linalg.det(U @ Vt)) * S[2]
        assert (u64 * np.linalg.norm(cov) / gap <= 1e-11) == judged, (kind, w)
        if kind == "planar":
            assert S[2] <= 1e-15 * S[0] and np.ptp(tgt[:, 2]) == 0 and np.ptp(src[:, 2]) == 0
        if kind == "collinear":
            assert S[1] <= 1e-14 * S[0]
