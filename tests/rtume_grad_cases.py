"""Inputs, fp64 truths, yardsticks and gates of tests/test_rtume_grad_edges_gpu.py, all of it checkable without a GPU
(tests/test_rtume_grad_cases_cpu.py): pairs on a ladder of gaps s2 + d s3 down to 1e-6 s1 with d = -1, pairs that are exact in fp32
on either side of the cut UMEREG_RTUME_BWD_MIN_GAP, exactly repeated singular values, one group of near-singular pairs among benign
ones, a pair without a path through R, masses small enough for the reference's two 1e-16 terms to weigh, and the 3 x 3 classes the
host build of csrc/polar_grad.h (tests/polar_grad_host.cpp) is judged on.

Truth: `cube_loss_ref.solve_grads_closed_form` in fp64 on the fp32 inputs with the header's cut; yardstick: the same closed form in
fp32 on the CPU (no 1 / (s_i^2 - s_j^2): it is as regular on repeated values as the kernel's formula).  Gate: per hypothesis,
`ume_grad_cases.row_gate`, with the sharp bar of `sharp_bar()`.  Nothing here touches the GPU library; `host_program()` takes the
compiler's path from `umeregrobust_amd._build`, as tests/test_ume_grad_plan_cpu.py does.

Small masses: the case exists (`small_mass_case`): at a scale of 2^-23 sum mg^2 is about 4e-16, both closed forms stay finite, and a
restatement with one 1e-16 in the left denominator is more than 100 sharp bars from the truth."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import torch

import cube_loss_ref as cref
from ume_grad_cases import row_gate as _row_gate
from ume_grad_cases import row_rel, row_stats          # noqa: F401  (re-exported: the gate's parts)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "umereg_rtume_grad.h")
TAG = "rtume ladder"


def header_min_gap():
    """UMEREG_RTUME_BWD_MIN_GAP as the header states it"""
    return float(re.search(r"#define UMEREG_RTUME_BWD_MIN_GAP (\S+)\n", open(HEADER).read()).group(1))


MIN_GAP = header_min_gap()


def say(line):
    print(f"[{TAG}] {line}")


def row_gate(got, truth, yard, name, groups=None, bar=None):
    """ume_grad_cases.row_gate under this module's tag"""
    return _row_gate(got, truth, yard, name, groups=groups, bar=bar, log=print, tag=TAG)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- truth and yardstick ------------------------------------------------------------------------------------------------------

def truth_and_yard(G, H, dT, min_gap=MIN_GAP):
    """((dG, dH) fp64, (dG, dH) fp32) of the closed form on the fp32 inputs"""
    assert G.dtype == H.dtype == dT.dtype == torch.float32
    return cref.solve_grads_closed_form(G.double(), H.double(), dT.double(), min_gap=min_gap), cref.solve_grads_closed_form(G, H, dT, min_gap=min_gap)


def signed_spectrum(G, H):
    """(s1, s2, d s3) [n, 3] and d [n] of the fp32 inputs' cross moments, in fp64"""
    S, d = cref.spectrum(G.double(), H.double())
    return S * torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1), d


def gap_ratio(G, H):
    """(s2 + d s3) / s1 per pair, fp64"""
    sp, _ = signed_spectrum(G, H)
    return (sp[:, 1] + sp[:, 2]) / sp[:, 0]


# ---- the gap ladder -----------------------------------------------------------------------------------------------------------

GAP_RUNGS = [1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6]
GAP_RUNGS_REQUIRED = GAP_RUNGS[:-1]         # the truth must resolve these (tests/test_rtume_grad_cases_cpu.py holds it to that)
N_RUNG = 17                                 # two full workgroups of 8 and a lone hypothesis in a half-filled wavefront


def _rotations(g, n):
    q = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64)).Q
    return q * torch.sign(torch.det(q))[:, None, None]          # (3 x 3: the sign of -q's determinant is the opposite one)


def _frames_off_the_mass(g, m):
    """q [n, 32, 3] with orthonormal columns, each orthogonal to m [n, 32]"""
    x = torch.cat([m[:, :, None], torch.randn(m.shape[0], 32, 3, generator=g, dtype=torch.float64)], dim=2)
    return torch.linalg.qr(x).Q[:, :, 1:]


@functools.lru_cache(maxsize=None)
def gap_rung(gap, n=N_RUNG):
    """(G, H, dT) fp32: G[:, 0] = m positive of unit norm, G[:, 1:] = q R1 + m (x) c, H[:, 0] = m times positive noise,
    H[:, 1:] = q diag(1, 0.5, -(0.5 - gap)) R2 + H[:, 0] (x) c'; q orthonormal and orthogonal to m.  The cross moment is
    R1^T diag(1, 0.5, -(0.5 - gap)) R2: d = -1 and (s2 + d s3) / s1 = gap, up to the fp32 rounding of the inputs."""
    g = gen(4000 + int(round(-np.log10(gap) * 10)) + 100 * n)
    m = torch.rand(n, 32, generator=g, dtype=torch.float64) + 0.1
    m = m / m.norm(dim=1, keepdim=True)
    q = _frames_off_the_mass(g, m)
    R1, R2 = _rotations(g, n), _rotations(g, n)
    c, c2 = torch.randn(n, 1, 3, generator=g, dtype=torch.float64), torch.randn(n, 1, 3, generator=g, dtype=torch.float64)
    mh = m * (0.5 + torch.rand(n, 32, generator=g, dtype=torch.float64))
    sv = torch.tensor([1.0, 0.5, -(0.5 - gap)], dtype=torch.float64)
    G, H = torch.zeros(n, 32, 4, dtype=torch.float64), torch.zeros(n, 32, 4, dtype=torch.float64)
    G[:, :, 0], H[:, :, 0] = m, mh
    G[:, :, 1:] = q @ R1 + m[:, :, None] * c
    H[:, :, 1:] = (q * sv) @ R2 + mh[:, :, None] * c2
    dT = torch.randn(n, 4, 4, generator=g, dtype=torch.float64)
    return G.float(), H.float(), dT.float()


@functools.lru_cache(maxsize=None)
def sharp_bar():
    """4 x the fp32 closed form's largest row-relative error on the 1e-1 rung, per side (dG, dH).  The kernel forms A, the frames and
    the signed values in fp64 from the fp32 inputs, so nothing in it should grow with 1 / gap beyond what the truth itself carries."""
    G, H, dT = gap_rung(GAP_RUNGS[0])
    truth, yard = truth_and_yard(G, H, dT)
    return tuple(4 * float(row_rel(y, t).max()) for y, t in zip(yard, truth))


# ---- pairs that are exact in fp32 ---------------------------------------------------------------------------------------------

HADAMARD_COLUMNS = (3, 5, 30)       # three columns of the 32 x 32 Sylvester matrix other than the all-ones column 0
CONST_G = (0.5, -0.25, 1.0)
CONST_H = (-0.5, 1.0, 0.25)


def hadamard_columns():
    """[32, 3] of +-1 (fp64): orthogonal to each other and to the all-ones column, squared norm 32"""
    i = np.arange(32)
    cols = [[(-1.0) ** bin(int(r) & c).count("1") for r in i] for c in HADAMARD_COLUMNS]
    return torch.tensor(cols, dtype=torch.float64).T.contiguous()


def hadamard_pair(g_diag, h_diag, shift=1):
    """(G, H) fp64 [32, 4]: masses 1 / 32, G[:, 1:] = q g_diag / 4 + const, H[:, 1:] = (q h_diag / 8 with its columns rolled by
    `shift`) + const.  q^T q = 32 I, so the cross moment is diag(g_diag h_diag) times a cyclic permutation (det +1): its signed
    values are the products g_diag h_diag."""
    q = hadamard_columns()
    G, H = torch.zeros(32, 4, dtype=torch.float64), torch.zeros(32, 4, dtype=torch.float64)
    G[:, 0] = H[:, 0] = 1.0 / 32
    G[:, 1:] = q * torch.tensor(g_diag, dtype=torch.float64) / 4 + torch.tensor(CONST_G, dtype=torch.float64)
    H[:, 1:] = torch.roll(q * torch.tensor(h_diag, dtype=torch.float64) / 8, shift, dims=1) + torch.tensor(CONST_H, dtype=torch.float64)
    return G, H


def cut_pair(s1, s2, e):
    """(G, H) fp64, exact in fp32: signed values (s1, s2, -s2 (1 - 2^-2e)), so d = -1 and s2 + d s3 = s2 2^-2e"""
    return hadamard_pair((1.0, 1.0, 1.0 - 2.0 ** -e), (s1, s2, -s2 * (1.0 + 2.0 ** -e)))


# (s1, s2, e, kept): (s2 + d s3) / s1 = 7.45e-9, 1.19e-8 (kept only by a cut RELATIVE to s1), 1.49e-8 (and s1 = s2), 2.98e-8, 1.86e-9
CUT_PAIRS = [(1.0, 0.5, 13, False), (0.625, 0.5, 13, True), (0.5, 0.5, 13, True), (1.0, 0.5, 12, True), (1.0, 0.5, 14, False)]
REPEATED = [(1.0, 1.0, 0.25), (1.0, 0.5, 0.5), (1.0, 1.0, 1.0), (1.0, 1.0, -0.25)]
GAP_ZERO = (1.0, 0.5, -0.5)


def cut_ratio(s1, s2, e):
    return s2 * 2.0 ** (-2 * e) / s1


def _stack32(pairs):
    G = torch.stack([p[0] for p in pairs])
    H = torch.stack([p[1] for p in pairs])
    assert torch.equal(G.float().double(), G) and torch.equal(H.float().double(), H), "the pairs must be exact in fp32"
    return G.float(), H.float()


def cut_pairs():
    """(G, H) fp32 [5, 32, 4], exactly the fp64 construction"""
    return _stack32([cut_pair(s1, s2, e) for s1, s2, e, _ in CUT_PAIRS])


def repeated_pairs():
    """(G, H) fp32 [4, 32, 4]: the signed values of REPEATED, exactly"""
    return _stack32([hadamard_pair((1.0, 1.0, 1.0), sv) for sv in REPEATED])


def gap_zero_pair():
    """(G, H) fp32 [1, 32, 4]: signed values (1, 0.5, -0.5), s2 + d s3 = 0 exactly"""
    return _stack32([hadamard_pair((1.0, 1.0, 1.0), GAP_ZERO)])


def interleave(special, n_total, where, seed):
    """(G, H, dT, where) fp32: benign `ume_pairs` with the given pairs at the positions `where`"""
    Gs, Hs = special
    G, H, dT = cref.ume_pairs(n_total, seed)
    G, H = G.clone(), H.clone()
    G[where], H[where] = Gs, Hs
    return G, H, dT


CUT_WHERE = [0, 3, 6, 9, 15]        # even and odd slots, the first, and the last of a workgroup: each next to a benign pair
CUT_TOTAL = 18
GAP_ZERO_WHERE = 11


@functools.lru_cache(maxsize=None)
def cut_case(with_gap_zero=False):
    """18 hypotheses: the five exact cut pairs at CUT_WHERE (and the exact-gap-0 pair at GAP_ZERO_WHERE) among benign pairs"""
    G, H, dT = interleave(cut_pairs(), CUT_TOTAL, CUT_WHERE, 5001)
    if with_gap_zero:
        z = gap_zero_pair()
        G[GAP_ZERO_WHERE], H[GAP_ZERO_WHERE] = z[0][0], z[1][0]
    return G, H, dT


REPEATED_WHERE = [0, 3, 4, 7]


@functools.lru_cache(maxsize=None)
def repeated_case():
    """8 hypotheses: the four exact repeated-value pairs, each in a wavefront with a benign pair"""
    return interleave(repeated_pairs(), 8, REPEATED_WHERE, 5002)


# ---- mixed, no path through R, small masses -----------------------------------------------------------------------------------

MIXED_ILL = [5, 17, 40, 63]
MIXED_GAP = 1e-4


@functools.lru_cache(maxsize=None)
def mixed_case():
    """(G, H, dT, ill): 64 hypotheses, four pairs of the 1e-4 rung at MIXED_ILL among benign `ume_pairs`"""
    Gr, Hr, dTr = gap_rung(MIXED_GAP, len(MIXED_ILL))
    G, H, dT = interleave((Gr, Hr), 64, MIXED_ILL, 5003)
    ill = torch.zeros(64, dtype=torch.bool)
    ill[MIXED_ILL] = True
    return G, H, dT, ill


@functools.lru_cache(maxsize=None)
def zero_pair():
    """(G, H, dT) fp32 [1, ...]: every coordinate zero, positive masses: A = 0, no path through R"""
    g = gen(5004)
    G, H = torch.zeros(1, 32, 4), torch.zeros(1, 32, 4)
    G[0, :, 0], H[0, :, 0] = torch.rand(32, generator=g) + 0.1, torch.rand(32, generator=g) + 0.1
    return G, H, torch.randn(1, 4, 4, generator=g)


def poisoned_pair(value):
    """(G, H) fp32 [1, 32, 4]: a benign pair with one coordinate of G replaced by `value` (NaN or Inf)"""
    G, H, _ = cref.ume_pairs(1, 5005)
    G = G.clone()
    G[0, 7, 2] = value
    return G, H


def parts_one_epsilon(G, H):
    """`cube_loss_ref._parts` with ONE 1e-16 in the left denominator where the reference has two"""
    mg, mh, g, h, mg_square, mg_mh, wlc, wrc, left, right = cref._parts(G, H)
    mg_square = mg_square - 1e-16
    wlc = torch.sum(g * mg, dim=1, keepdim=True) / (mg_square + 1e-16)
    return mg, mh, g, h, mg_square, mg_mh, wlc, wrc, g - wlc * mg, right


SMALL_MASS_SHIFT = 23       # masses times 2^-23: sum mg^2 about 4e-16


@functools.lru_cache(maxsize=None)
def small_mass_case():
    """(G, H, dT) fp32: 17 benign pairs with both mass columns scaled by 2^-SMALL_MASS_SHIFT (exact)"""
    G, H, dT = cref.ume_pairs(17, 5006)
    G, H = G.clone(), H.clone()
    G[:, :, 0] *= 2.0 ** -SMALL_MASS_SHIFT
    H[:, :, 0] *= 2.0 ** -SMALL_MASS_SHIFT
    return G, H, dT


# ---- the 3 x 3 level: csrc/polar_grad.h on the host ---------------------------------------------------------------------------

def polar_closed_form(A, gR, min_gap):
    """(R, s' [n, 3], gA) in fp64 through torch.linalg.svd: the rotation's part of `cube_loss_ref.solve_grads_closed_form`"""
    U, S, Vh = torch.linalg.svd(A)
    d = torch.sign(torch.det(U @ Vh))
    sgn = torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1)
    Vp = Vh.transpose(1, 2) * sgn[:, None, :]
    sp = S * sgn
    C = U.transpose(1, 2) @ gR @ Vp
    gap = sp[:, :, None] + sp[:, None, :]
    ok = (gap > min_gap * S[:, :1, None]) & ~torch.eye(3, dtype=torch.bool)
    Y = torch.where(ok, (C - C.transpose(1, 2)) / torch.where(ok, gap, torch.ones_like(gap)), torch.zeros_like(C))
    return U @ Vp.transpose(1, 2), sp, U @ Y @ Vp.transpose(1, 2)


N_FRAMES = 64


def framed(signed, seed, scale=1.0):
    """(A, gR) fp64 [64, 3, 3]: A = U diag(signed) V^T with random rotations U, V; signed [3] or [64, 3]"""
    g = gen(seed)
    U, V = _rotations(g, N_FRAMES), _rotations(g, N_FRAMES)
    s = torch.as_tensor(signed, dtype=torch.float64).expand(N_FRAMES, 3)
    A = (U * s[:, None, :]) @ V.transpose(1, 2) * scale
    return A, torch.randn(N_FRAMES, 3, 3, generator=g, dtype=torch.float64)


def _benign_values(seed):
    """signed values [64, 3]: s1 in [0.8, 1.2], s2 in [0.4, 0.7], s3 in [0.05, 0.3] with either sign: s2 + d s3 >= 0.1"""
    g = gen(seed)
    r = torch.rand(N_FRAMES, 4, generator=g, dtype=torch.float64)
    sign = torch.where(r[:, 3] < 0.5, -1.0, 1.0).double()
    return torch.stack([0.8 + 0.4 * r[:, 0], 0.4 + 0.3 * r[:, 1], (0.05 + 0.25 * r[:, 2]) * sign], dim=1)


def _near_rank_one(seed):
    g = gen(seed)
    t = 10.0 ** (-3.0 - 6.0 * torch.rand(N_FRAMES, generator=g, dtype=torch.float64))       # 1e-3 ... 1e-9
    sign = torch.where(torch.rand(N_FRAMES, generator=g) < 0.5, -1.0, 1.0).double()
    return torch.stack([torch.ones_like(t), t, 0.5 * t * sign], dim=1)


def host_classes():
    """{name: (A, gR, regular)}: the 3 x 3 classes; regular: no small gap, the two fp64 evaluations must agree to 1e-12"""
    out = {"benign": framed(_benign_values(6000), 6001) + (True,)}
    for k, sv in enumerate(REPEATED):
        out[f"repeated {sv}"] = framed(sv, 6010 + k) + (True,)
    out["s3 = 0"] = framed((1.0, 0.5, 0.0), 6020) + (True,)
    out["s3 = +1e-9"] = framed((1.0, 0.5, 1e-9), 6021) + (True,)
    out["s3 = -1e-9"] = framed((1.0, 0.5, -1e-9), 6022) + (True,)
    out["A x 1e-30"] = framed(_benign_values(6030), 6031, 1e-30) + (True,)
    out["A x 1e+30"] = framed(_benign_values(6032), 6033, 1e30) + (True,)
    out["near rank 1"] = framed(_near_rank_one(6040), 6041) + (False,)
    for k, gap in enumerate(GAP_RUNGS):
        out[f"gap {gap:.0e}"] = framed((1.0, 0.5, -(0.5 - gap)), 6050 + k) + (False,)
    out["gap 2e-8 (kept)"] = framed((1.0, 0.5, -(0.5 - 2e-8)), 6060) + (False,)
    out["gap 5e-9 (dropped)"] = framed((1.0, 0.5, -(0.5 - 5e-9)), 6061) + (False,)
    return out


def mat_rel(x, truth):
    """|x_i - truth_i|_F / |truth_i|_F per 3 x 3 matrix"""
    return row_rel(x, truth)


@functools.lru_cache(maxsize=None)
def host_program():
    """path of tests/polar_grad_host.cpp compiled with the compiler that builds the library, or None where there is none"""
    from umeregrobust_amd import _build
    hipcc = _build.HIPCC if os.path.exists(_build.HIPCC) else shutil.which("hipcc")
    if not hipcc:
        return None
    tmp = tempfile.mkdtemp(prefix="polar_grad_host_")
    atexit.register(shutil.rmtree, tmp, True)
    exe = os.path.join(tmp, "polar_grad_host")
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", _build.CSRC,
                           os.path.join(REPO, "tests", "polar_grad_host.cpp"), "-o", exe])
    return exe


def host_polar(A, gR, min_gap, exe=None):
    """(has_frames bool [n], s [n, 3], gA [n, 3, 3], R [n, 3, 3], U, V) of polar_frames / polar_rotation_grad / polar_rotation on the
    host; every number crosses as a hexadecimal float, bit for bit.  min_gap: a float or one per matrix."""
    exe = exe or host_program()
    n = A.shape[0]
    mg = np.broadcast_to(np.asarray(min_gap, np.float64), (n,))
    rows = np.concatenate([A.reshape(n, 9).numpy(), gR.reshape(n, 9).numpy(), mg[:, None]], axis=1)
    text = "".join(" ".join(float(v).hex() for v in r) + "\n" for r in rows)
    out = subprocess.run([exe], input=text, capture_output=True, check=True, text=True).stdout.split("\n")
    vals = np.array([[float.fromhex(v) for v in ln.split()] for ln in out if ln], np.float64)
    assert vals.shape == (n, 1 + 3 + 9 + 9 + 9 + 9), vals.shape
    t = torch.from_numpy(vals)
    return (t[:, 0] != 0, t[:, 1:4], t[:, 4:13].reshape(n, 3, 3), t[:, 13:22].reshape(n, 3, 3), t[:, 22:31].reshape(n, 3, 3),
            t[:, 31:40].reshape(n, 3, 3))


@functools.lru_cache(maxsize=None)
def truth_resolution():
    """{gap: the largest relative difference of gA between the host build of polar_grad.h and the closed form through torch's SVD,
    both fp64, over 64 random frame pairs}: the truth's own uncertainty on that rung.  None where no compiler is found."""
    if host_program() is None:
        return None
    classes = host_classes()
    out = {}
    for gap in GAP_RUNGS:
        A, gR, _ = classes[f"gap {gap:.0e}"]
        _, _, gA, *_ = host_polar(A, gR, MIN_GAP)
        out[gap] = float(mat_rel(gA, polar_closed_form(A, gR, MIN_GAP)[2]).max())
    return out


def eligible(gap):
    """whether the sharp bar may judge this rung: the truth's uncertainty there is at most a tenth of the bar.  The rungs of
    GAP_RUNGS_REQUIRED are held to that by the CPU tests; the last one is eligible only where it is measured to be."""
    res = truth_resolution()
    if res is None:
        return gap in GAP_RUNGS_REQUIRED
    return res[gap] <= min(sharp_bar()) / 10
