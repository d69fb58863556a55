"""The oracle's fp64 Householder basis and subspace distance against a 50-digit truth, without a GPU.

oracle.orthobasis_f64 / oracle.ume_cdist_f64 stand in for truth in every GPU test of the bases and of what consumes them, yet they are
a C restatement of the kernel's algorithm in the kernel's precision: an error the two share is invisible there.  Here they are judged
against tests/ortho_cases.truth (mpmath, 50 digits) on every rung of tests/ortho_cases.py, matrices of cond up to 7e13 included, and
held to what numpy's LAPACK achieves on the same input.  tests/test_ortho_gpu.py relies on three things asserted here: that every
rung qualifies for its bar, that the oracle's projector is LAPACK-class on all of them, and that its distance is good to 1e-9 / D.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import ortho_cases as oc

_EPS_LD = float(np.finfo(oc.LD).eps)


@pytest.fixture(scope="module")
def rungs():
    return oc.rungs()


def test_the_truth_is_a_qr_factorisation(rungs):
    """An independent check of the 50-digit Q, which shares no step with how it was computed: Q^T Q = I, R = Q^T A is upper triangular
    and Q R = A, each to the working precision of np.longdouble and relative to the column's norm (the graded columns reach 2^-36).
    For a full-rank A these three fix Q up to the signs of its columns; the signs are judged against numpy below."""
    tol = 256 * _EPS_LD
    for name, mats in rungs.items():
        for i, a in enumerate(mats):
            t = oc.truth(a)
            A = a.astype(oc.LD)
            cn = np.maximum(np.sqrt((A * A).sum(axis=0)), np.finfo(np.float64).tiny)
            R = t.Q.T @ A
            assert oc.err_orth(t.Q) <= tol, (name, i)
            assert (np.abs(np.tril(R, -1)) / cn).max() <= tol, (name, i)
            assert (np.abs(t.Q @ R - A) / cn).max() <= tol, (name, i)


def test_every_rung_is_judged(rungs):
    """max(e_round, e_lapack) <= 1e-6 on every rung: none drops out of the GPU tests' bars, cond 7e13 included"""
    for name, mats in rungs.items():
        y = oc.rung_yardsticks(mats)
        cond = [np.linalg.cond(a.astype(np.float64)) for a in mats]
        print(f"[ortho yardsticks] {name:12s} cond {min(cond):.1e} .. {max(cond):.1e}: e_round {y.e_round:.2e}, e_lapack {y.e_lapack:.2e}, "
              f"|Q32^T Q32 - I| {y.orth_round:.2e}")
        assert max(y.e_round, y.e_lapack) <= oc.JUDGED_MAX, (name, y)
    assert len(rungs) == len(oc.GENERIC_K) + len(oc.FAR_C) + len(oc.GRADED_EXP) + 1
    assert sum(len(m) for m in rungs.values()) <= 150                      # (the truth costs about 25 ms a matrix)


def test_oracle_projector_is_lapack_class(rungs):
    """orc.orthobasis_f64 is within 4 x the rung's e_lapack of the 50-digit projector, on every rung"""
    for name, mats in rungs.items():
        y = oc.rung_yardsticks(mats)
        Q = orc.orthobasis_f64(mats)
        e = max(oc.err_P(Q[i], oc.truth(mats[i])) for i in range(len(mats)))
        print(f"[ortho oracle] {name:12s} oracle {e:.2e}, e_lapack {y.e_lapack:.2e}")
        assert e <= oc.SLACK * y.e_lapack, (name, e, y.e_lapack)


@pytest.mark.parametrize("ci", range(len(oc.FAR_C)))
def test_oracle_distance_on_far_balls(ci):
    """orc.ume_cdist_f64 on 8 x 8 pairs of a far rung (its six matrices and two perturbed copies, each against each) is within
    1e-9 / D of D = sqrt(4 - tr(P1 P2)) from the 50-digit bases, wherever D > 0.05."""
    mats = np.concatenate([oc.far(ci), oc.far_perturbed(ci, 2)])
    assert mats.shape[0] == 8
    Q = np.stack([oc.truth(a).Q for a in mats])
    C = np.einsum("ika,jkb->ijab", Q, Q)
    D = np.sqrt(np.maximum(4 - (C * C).sum(axis=(2, 3)), 0)).astype(np.float64)
    D64 = orc.ume_cdist_f64(mats, mats)
    far = D > 0.05
    assert far.sum() >= 50 and not far[np.arange(8), np.arange(8)].any(), far.sum()
    e = np.abs(D64 - D)[far] * D[far]
    print(f"[ortho oracle] far |c| = {oc.FAR_C[ci]:.0e}: {int(far.sum())} pairs, D {D[far].min():.3f} .. {D[far].max():.3f}, "
          f"max |D64 - D| D {e.max():.2e}, max |D64 - D| at D <= 0.05 {np.abs(D64 - D)[~far].max():.2e}")
    assert e.max() <= 1e-9


def test_oracle_q_is_lapacks_on_the_conventions():
    """The conventions family: the oracle's Q equals numpy.linalg.qr's column for column, signs included (-0.0 on the diagonal counts
    as negative in both); both are within 4 x numpy's own distance from the 50-digit Q; and every column that the tau = 0 convention
    leaves as e_k is e_k exactly."""
    cases = oc.conventions()
    mats = np.stack(list(cases.values()))
    Q = orc.orthobasis_f64(mats)
    Qn = np.stack([oc.lapack_q(a) for a in mats])
    Qt = np.stack([oc.truth(a).Q for a in mats])
    e_np = np.abs(Qn - Qt).max(axis=(1, 2)).astype(np.float64)
    e_or = np.abs(Q - Qt).max(axis=(1, 2)).astype(np.float64)
    print(f"[ortho oracle] conventions: max |Q_numpy - Q50| {e_np.max():.2e}, max |Q_oracle - Q50| {e_or.max():.2e}")
    eye = np.eye(32)[:, :4]
    n_exact = 0
    for i, name in enumerate(cases):
        assert e_or[i] <= oc.SLACK * e_np.max(), (name, e_or[i], e_np.max())
        assert np.abs(Q[i] - Qn[i]).max() <= (1 + oc.SLACK) * e_np.max(), (name, np.abs(Q[i] - Qn[i]).max())
        assert (np.sign((Q[i] * Qn[i]).sum(axis=0)) > 0).all(), name                     # (said once more, in the plainest way)
        for k in range(4):
            if np.array_equal(Qt[i][:, k], eye[:, k].astype(oc.LD)):
                assert np.array_equal(Q[i][:, k], eye[:, k]) and np.array_equal(Qn[i][:, k], eye[:, k]), (name, k)
                n_exact += 1
    assert np.array_equal(Q[list(cases).index("zero")], eye) and np.array_equal(Q[list(cases).index("top4_triu")], eye)
    # the zero matrix and top4_triu: four columns each; one non-zero column j leaves e_k for k < j: 0 + 1 + 2 + 3
    assert n_exact == 14, n_exact
    # the sign convention is exercised: -0.0 on the diagonal flips column 0 against the same matrix with +0.0
    a = cases["negzero_diag"].copy()
    a[0, 0] = 0.0
    assert (orc.orthobasis_f64(a[None])[0][:, 0] * Q[list(cases).index("negzero_diag")][:, 0]).sum() < -0.99
