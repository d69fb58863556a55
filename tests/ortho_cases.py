"""32x4 matrices for the Householder bases (csrc/householder.h) and the singular values (svdvals_kernel), with a 50-digit truth and
the two yardsticks every bar on them is derived from.  Shared by tests/test_ortho_cpu.py (no GPU: the oracle against the truth, and
that every rung qualifies) and tests/test_ortho_gpu.py (the kernels).  Test infrastructure only, host only.

Families (fp32, seeded, 6 matrices a rung; the fp32 entries are taken as exact)
  generic_k      U diag(logspace(0, -k, 4)) V^T * 37, k = 0, 3, 6, 8
  far_c          UME-shaped [m, m o (c + d)]: m > 0 with sum 1, d ~ 2 N(0, 1), a ball centre of length |c| = 0, 1e2 .. 1e7
                 (cond 5e3 .. 7e13: column grading, which Householder QR does not suffer from)
  graded_j       a well-conditioned B (half of them with correlated columns, B + 3 B[:, :1]) times exact power-of-two column scales
  conventions    the zero matrix, one non-zero column, all tails zero, a zero middle column, -0.0, entries at 1e+-18
  NONFINITE      one NaN, one inf: no truth exists; they are only ever batch neighbours (slot independence)

Truth   Householder QR with LAPACK's dgeqr2 / dorg2r conventions (beta = -sign(alpha) |x|, -0.0 counting as negative as Fortran's SIGN
        has it; tau = 0 and H = I when the tail is exactly zero) in mpmath at 50 digits, held as np.longdouble (64-bit mantissa where
        the platform has one: the truth is then good to 1e-19, and errors of 1e-16 are measured to three digits).
Error   err_P(Q) = max |Q Q^T - P_truth|, the projector: what every consumer of the bases uses.
Yardsticks, per matrix, and per rung their maximum
  e_round    err_P of the truth's Q rounded to fp32: what storing a perfect basis in fp32 costs
  e_lapack   err_P of numpy.linalg.qr in fp64 on the same input
A rung is JUDGED when max(e_round, e_lapack) <= 1e-6 (JUDGED_MAX); the bar on a kernel that stores fp32 is SLACK = 4 times that
maximum: one factor 2 for another summation order flipping fp32 roundings, one factor 2 of margin.
"""
from collections import OrderedDict, namedtuple

import mpmath
import numpy as np

LD = np.longdouble
JUDGED_MAX = 1e-6
SLACK = 4.0
N_PER_RUNG = 6
GENERIC_K = [0, 3, 6, 8]
FAR_C = [0.0, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7]
GRADED_EXP = [[0, -12, -24, -36], [-36, -24, -12, 0], [0, -30, -1, -31]]

Truth = namedtuple("Truth", "Q P tau0")          # Q longdouble [32,4], P longdouble [32,32], tau0 bool [4] (H_k = I)


# ------------------------------------------------------------------------------------------------ families
def _orth(rng, rows, cols):
    q, r = np.linalg.qr(rng.standard_normal((rows, cols)))
    return q * np.sign(np.diag(r))


def generic(k):
    rng = np.random.RandomState([31, 0, k])
    return np.stack([(_orth(rng, 32, 4) * np.logspace(0, -k, 4)) @ _orth(rng, 4, 4).T * 37.0
                     for _ in range(N_PER_RUNG)]).astype(np.float32)


def far_one(rng, cnorm):
    """one UME-shaped matrix [m, m o (c + d)] and the parts it was made of (fp64)"""
    m = rng.uniform(0.2, 1.0, 32)
    m /= m.sum()
    c = rng.standard_normal(3)
    c *= cnorm / np.linalg.norm(c)
    d = 2.0 * rng.standard_normal((32, 3))
    return m, c, d


def _far_matrix(m, c, d):
    return np.concatenate([m[:, None], m[:, None] * (c + d)], axis=1).astype(np.float32)


def far(ci, n=N_PER_RUNG):
    rng = np.random.RandomState([31, 1, ci])
    return np.stack([_far_matrix(*far_one(rng, FAR_C[ci])) for _ in range(n)])


def far_perturbed(ci, n, rel=0.05, seed=0):
    """the first n matrices of far(ci, n) with d perturbed by rel * 2 N(0, 1): the same ball seen with a little noise"""
    rng = np.random.RandomState([31, 1, ci])
    rng2 = np.random.RandomState([31, 4, ci, seed])
    out = []
    for _ in range(n):
        m, c, d = far_one(rng, FAR_C[ci])
        out.append(_far_matrix(m, c, d + rel * 2.0 * rng2.standard_normal((32, 3))))
    return np.stack(out)


def graded_bases():
    """the well-conditioned B: fp32 [6,32,4]; odd ones have correlated columns"""
    rng = np.random.RandomState([31, 2])
    B = rng.standard_normal((N_PER_RUNG, 32, 4))
    B[1::2] += 3.0 * B[1::2, :, :1]
    return B.astype(np.float32)


def graded(j):
    return (graded_bases() * np.exp2(np.array(GRADED_EXP[j], np.float64)).astype(np.float32)).astype(np.float32)


def conventions():
    """-> OrderedDict name -> fp32 [32,4]"""
    rng = np.random.RandomState([31, 3])
    out = OrderedDict()
    out["zero"] = np.zeros((32, 4), np.float32)
    for j in range(4):
        a = np.zeros((32, 4), np.float32)
        a[:, j] = rng.standard_normal(32)
        out[f"one_column_{j}"] = a
    a = np.zeros((32, 4), np.float32)
    a[:4] = rng.standard_normal((4, 4))
    out["top4_dense"] = a                                    # tails of columns 0..2 non-zero, column 3's exactly zero (either sign of a33)
    b = a.copy()
    b[3, 3] = -abs(b[3, 3])
    out["top4_dense_neg"] = b
    a = np.zeros((32, 4), np.float32)
    a[:4] = np.triu(rng.standard_normal((4, 4)))
    a[np.arange(4), np.arange(4)] = [-1.5, 2.0, -0.25, -3.0]
    out["top4_triu"] = a                                     # every tail exactly zero: Q = I[:, :4], negative diagonal or not
    for j in (1, 2):
        a = rng.standard_normal((32, 4)).astype(np.float32)
        a[:, j] = 0.0
        out[f"zero_column_{j}"] = a
    a = rng.standard_normal((32, 4)).astype(np.float32)
    a[0, 0] = -0.0                                           # alpha = -0.0 with a tail: LAPACK's SIGN takes it as negative
    out["negzero_diag"] = a
    a = rng.standard_normal((32, 4)).astype(np.float32)
    a[rng.rand(32, 4) < 0.3] = -0.0
    a[:, 3] = -0.0                                           # and a whole column of -0.0: tau = 0
    a[1, 1] = 1.0
    out["negzero_scattered"] = a
    out["big_1e18"] = (rng.standard_normal((32, 4)) * 1e18).astype(np.float32)
    out["small_1e-18"] = (rng.standard_normal((32, 4)) * 1e-18).astype(np.float32)
    out["mixed_1e+-18"] = (rng.standard_normal((32, 4)) * np.array([1e18, 1e-18, 1.0, 1e18])).astype(np.float32)
    return out


def nonfinite():
    rng = np.random.RandomState([31, 5])
    a = rng.standard_normal((2, 32, 4)).astype(np.float32)
    a[0, 17, 2] = np.nan
    a[1, 5, 1] = np.inf
    return a


def rungs():
    """-> OrderedDict rung -> fp32 [n,32,4]: every rung that has a truth, in a fixed order"""
    out = OrderedDict()
    for k in GENERIC_K:
        out[f"generic_{k}"] = generic(k)
    for ci in range(len(FAR_C)):
        out[f"far_{FAR_C[ci]:.0e}"] = far(ci)
    for j in range(len(GRADED_EXP)):
        out[f"graded_{j}"] = graded(j)
    out["conventions"] = np.stack(list(conventions().values()))
    return out


# ------------------------------------------------------------------------------------------------ truth
_TRUTH = {}
_SIGMA = {}


def _ld(x):
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def _mp_householder(A32):
    """LAPACK-convention Householder Q of one fp32 [32,4] in mpmath (call under workdps) -> (Q as [32][4] mpf, tau0 [4])"""
    rows = A32.shape[0]
    a = [[mpmath.mpf(float(A32[r, c])) for c in range(4)] for r in range(rows)]
    tau = [mpmath.mpf(0)] * 4
    touched = False                                          # has a reflection with tau != 0 been applied yet
    for k in range(4):
        alpha = a[k][k]
        xn2 = mpmath.fsum(a[r][k] * a[r][k] for r in range(k + 1, rows))
        if xn2 == 0:
            continue
        nrm = mpmath.sqrt(alpha * alpha + xn2)
        neg = alpha < 0 or (alpha == 0 and not touched and bool(np.signbit(A32[k, k])))
        beta = nrm if neg else -nrm
        tau[k] = (beta - alpha) / beta
        sc = 1 / (alpha - beta)
        for r in range(k + 1, rows):
            a[r][k] *= sc
        a[k][k] = beta
        touched = True
        for c in range(k + 1, 4):
            w = (a[k][c] + mpmath.fsum(a[r][k] * a[r][c] for r in range(k + 1, rows))) * tau[k]
            a[k][c] -= w
            for r in range(k + 1, rows):
                a[r][c] -= w * a[r][k]
    q = [[mpmath.mpf(1 if r == c else 0) for c in range(4)] for r in range(rows)]
    for k in range(3, -1, -1):
        if tau[k] == 0:
            continue
        for c in range(4):
            w = (q[k][c] + mpmath.fsum(a[r][k] * q[r][c] for r in range(k + 1, rows))) * tau[k]
            q[k][c] -= w
            for r in range(k + 1, rows):
                q[r][c] -= w * a[r][k]
    return q, [t == 0 for t in tau]


def truth(A32):
    """50-digit Q and projector of one fp32 [32,4], cached per process"""
    A32 = np.ascontiguousarray(A32, np.float32)
    assert A32.shape == (32, 4) and np.isfinite(A32).all()
    key = A32.tobytes()
    if key not in _TRUTH:
        with mpmath.workdps(50):
            q, tau0 = _mp_householder(A32)
            Q = np.array([[_ld(x) for x in row] for row in q], dtype=LD)
        _TRUTH[key] = Truth(Q, Q @ Q.T, np.array(tau0))
    return _TRUTH[key]


def sigma_truth(A32):
    """singular values of one fp32 [32,4] by mpmath.svd_r at 50 digits, descending, as fp64 (good to 1e-16 relative each)"""
    A32 = np.ascontiguousarray(A32, np.float32)
    key = A32.tobytes()
    if key not in _SIGMA:
        with mpmath.workdps(50):
            S = mpmath.svd_r(mpmath.matrix(A32.astype(np.float64).tolist()), compute_uv=False)
            _SIGMA[key] = np.array(sorted((float(s) for s in S), reverse=True))
    return _SIGMA[key]


# ------------------------------------------------------------------------------------------------ errors and yardsticks
def err_P(Q, t):
    """max |Q Q^T - P_truth| of one basis [32,4] (any float type) against its Truth"""
    Q = np.asarray(Q).astype(LD)
    return float(np.abs(Q @ Q.T - t.P).max())


def err_orth(Q):
    Q = np.asarray(Q).astype(LD)
    return float(np.abs(Q.T @ Q - np.eye(4, dtype=LD)).max())


def lapack_q(A32):
    """numpy.linalg.qr's reduced Q of the fp32 matrix in fp64"""
    return np.linalg.qr(np.asarray(A32, np.float32).astype(np.float64), mode="reduced")[0]


Yard = namedtuple("Yard", "e_round e_lapack orth_round")


def yardsticks(A32):
    """per-matrix yardsticks of one fp32 [32,4]: (e_round, e_lapack, |Q32^T Q32 - I| of the fp32-rounded truth)"""
    t = truth(A32)
    q32 = t.Q.astype(np.float32)
    return Yard(err_P(q32, t), err_P(lapack_q(A32), t), err_orth(q32))


def rung_yardsticks(mats):
    """the maxima over a rung"""
    y = np.array([yardsticks(a) for a in mats])
    return Yard(*y.max(axis=0))


def bar(y):
    return SLACK * max(y.e_round, y.e_lapack)


# ------------------------------------------------------------------------------------------------ consumers
def consumer_sets():
    """What consumes the bases, on the far rungs: sources = every far matrix (42, rung by rung); targets = a perturbed copy of each in
    the same order (target i is source i seen again), then 25 decoys (other balls at the same centres): 67 = 64 + 3 targets."""
    nr = len(FAR_C)
    src = np.concatenate([far(ci) for ci in range(nr)])
    tgt = np.concatenate([far_perturbed(ci, N_PER_RUNG) for ci in range(nr)] +
                         [far_perturbed(ci, 4, rel=1.0, seed=1) for ci in range(nr)])[:67]
    return src, tgt
