"""Torch restatement of the RTUME solve (reference utils/loc_utils.py:292-350, the transform only) and of
`CubeRegistrationLoss` (reference loss.py:121-190).  Runs in the dtype of its inputs (fp64: the truth of the gradient tests; fp32: the
yardstick of their gates); gradients come from autograd through `torch.linalg.svd`.  `solve_grads_closed_form` is the chain
written out by hand with the derivative of the rotation itself, for a check against that autograd.  Nothing here is shared with
the library.  (The reference's own class cannot run in fp64: its `torch.eye` calls carry no dtype.)"""
import torch

CUBE = [[-1, 1, 1], [1, 1, 1], [-1, -1, 1], [1, -1, 1], [-1, 1, -1], [1, 1, -1], [-1, -1, -1], [1, -1, -1]]


def _parts(G, H):
    mg, mh = G[:, :, 0:1], H[:, :, 0:1]
    g, h = G[:, :, 1:], H[:, :, 1:]
    mg_square = torch.sum(mg ** 2, dim=1, keepdim=True) + 1e-16
    mg_mh = torch.sum(mg * mh, dim=1, keepdim=True)
    wlc = torch.sum(g * mg, dim=1, keepdim=True) / (mg_square + 1e-16)         # [n, 1, 3]
    wrc = torch.sum(h * mg, dim=1, keepdim=True) / (mg_mh + 1e-16)
    left, right = g - wlc * mg, h - wrc * mh
    return mg, mh, g, h, mg_square, mg_mh, wlc, wrc, left, right


def solve(G, H):
    """G (source), H (target) [n, 32, 4] -> T [n, 4, 4]: T[:3,:3] = R^T, T[:3,3] = b2"""
    n = G.shape[0]
    *_, wlc, wrc, left, right = _parts(G, H)
    A = left.transpose(1, 2) @ right
    U, S, Vh = torch.linalg.svd(A)
    d = torch.sign(torch.det(U @ Vh)).detach()
    Q = torch.diag_embed(torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1))
    R = U @ Q @ Vh
    b2 = wrc - wlc @ R                                                         # [n, 1, 3]
    top = torch.cat([R.transpose(1, 2), b2.transpose(1, 2)], dim=2)            # [n, 3, 4]
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=G.dtype).expand(n, 1, 4)
    return torch.cat([top, bottom], dim=1)


def spectrum(G, H):
    """(s [n, 3] descending, d [n] = sign det(U Vh)) of the solve's 3x3 cross moment"""
    *_, left, right = _parts(G, H)
    U, S, Vh = torch.linalg.svd(left.transpose(1, 2) @ right)
    return S, torch.sign(torch.det(U @ Vh))


def solve_grads(G, H, dT):
    """(T, dG, dH) of <solve(G, H), dT> by autograd"""
    a, b = G.detach().clone().requires_grad_(), H.detach().clone().requires_grad_()
    T = solve(a, b)
    (T * dT).sum().backward()
    return T.detach(), a.grad, b.grad


def solve_grads_closed_form(G, H, dT, min_gap=0.0, parts=None):
    """(dG, dH) of <solve(G, H), dT>: product and quotient rules by hand, and for the rotation R = U V'^T (V' = V diag(1, 1, d),
    s' = (s1, s2, d s3)):  C = U^T gR V',  Y_ij = (C_ij - C_ji) / (s'_i + s'_j),  gA = U Y V'^T; pairs with
    s'_i + s'_j <= min_gap * s1 get Y_ij = 0.  `parts`: a stand-in for `_parts` (a test of the tests: a deliberately wrong
    restatement must be told from this one)."""
    mg, mh, g, h, mg_square, mg_mh, wlc, wrc, left, right = (parts or _parts)(G, H)
    A = left.transpose(1, 2) @ right
    U, S, Vh = torch.linalg.svd(A)
    d = torch.sign(torch.det(U @ Vh))
    sgn = torch.stack([torch.ones_like(d), torch.ones_like(d), d], dim=-1)     # [n, 3]
    Vp = Vh.transpose(1, 2) * sgn[:, None, :]
    sp = S * sgn
    R = U @ Vp.transpose(1, 2)
    db2 = dT[:, :3, 3][:, None, :]                                             # [n, 1, 3]
    gR = dT[:, :3, :3].transpose(1, 2) - wlc.transpose(1, 2) @ db2
    g_wrc = db2.clone()
    g_wlc = -(db2 @ R.transpose(1, 2))
    C = U.transpose(1, 2) @ gR @ Vp
    gap = sp[:, :, None] + sp[:, None, :]
    ok = (gap > min_gap * S[:, :1, None]) & ~torch.eye(3, dtype=torch.bool)
    Y = torch.where(ok, (C - C.transpose(1, 2)) / torch.where(ok, gap, torch.ones_like(gap)), torch.zeros_like(C))
    gA = U @ Y @ Vp.transpose(1, 2)
    g_left, g_right = right @ gA.transpose(1, 2), left @ gA                    # [n, 32, 3]
    g_wlc = g_wlc - (g_left * mg).sum(dim=1, keepdim=True)
    g_wrc = g_wrc - (g_right * mh).sum(dim=1, keepdim=True)
    g_mg = -(g_left * wlc).sum(dim=2, keepdim=True)
    g_mh = -(g_right * wrc).sum(dim=2, keepdim=True)
    g_gmg, g_hmg = g_wlc / (mg_square + 1e-16), g_wrc / (mg_mh + 1e-16)
    g_sq = -(g_gmg * wlc).sum(dim=2, keepdim=True)
    g_mm = -(g_hmg * wrc).sum(dim=2, keepdim=True)
    g_g = g_left + g_gmg * mg
    g_h = g_right + g_hmg * mg
    g_mg = g_mg + (g_gmg * g).sum(dim=2, keepdim=True) + (g_hmg * h).sum(dim=2, keepdim=True) + 2 * g_sq * mg + g_mm * mh
    g_mh = g_mh + g_mm * mg
    return torch.cat([g_mg, g_g], dim=2), torch.cat([g_mh, g_h], dim=2)


def rre_deg(R, R_hat):
    """utils/eval_utils.py:60-76"""
    tr = torch.einsum("bii->b", R_hat @ R.transpose(1, 2)).clamp(-1, 3)
    return torch.acos((tr - 1) / 2) * (180 / 3.141592653589793)


def cube_loss(src_ume, tgt_ume, gt_tform, ratio, valid, cube_scale=1.0, thr=0.75):
    """loss.py:137-190 -> (loss, rre [bs, n], rte [bs, n]); src_ume, tgt_ume [bs, n, 32, 4], gt_tform [B, 4, 4], valid bool [B]"""
    dt = src_ume.dtype
    gt = gt_tform[valid].to(dt)
    bs, n = src_ume.shape[:2]
    cube = torch.tensor(CUBE, dtype=dt) * cube_scale
    T = solve(src_ume.reshape(bs * n, 32, 4), tgt_ume.reshape(bs * n, 32, 4)).view(bs, n, 4, 4)
    R, t = T[..., :3, :3], T[..., :3, 3]
    R_gt, t_gt = gt[:, :3, :3], gt[:, :3, 3]
    est = cube[None, None].expand(bs, n, -1, -1) @ R.transpose(-1, -2) + t.unsqueeze(-2)
    want = (cube @ R_gt.transpose(-1, -2) + t_gt[:, None])[:, None].expand(-1, n, -1, -1)
    per_kp = (want - est).norm(dim=-1).mean(dim=-1)
    cond = ratio >= thr
    if cond.sum() == 0:
        cond = ratio >= ratio.median(dim=-1, keepdim=True)[0]
    loss = per_kp[cond].mean()
    with torch.no_grad():
        rre = rre_deg(R.reshape(bs * n, 3, 3), R_gt[:, None].expand(-1, n, -1, -1).reshape(bs * n, 3, 3)).view(bs, n)
        rte = (t - t_gt[:, None]).norm(dim=-1)
    return loss, rre, rte


def loss_and_grads(src_ume, tgt_ume, gt_tform, ratio, valid, cube_scale=1.0, thr=0.75):
    """(loss, rre, rte, d loss / d src_ume, d loss / d tgt_ume)"""
    a, b = src_ume.detach().clone().requires_grad_(), tgt_ume.detach().clone().requires_grad_()
    loss, rre, rte = cube_loss(a, b, gt_tform, ratio, valid, cube_scale, thr)
    loss.backward()
    return loss.detach(), rre, rte, a.grad, b.grad


def ume_pairs(n, seed, thin=False, K=200, angle=0.7):
    """n UME-like pairs as fp32 tensors: G the normalised moment matrix of a neighbourhood of K points with positive features, H that
    of the neighbourhood rotated by `angle` rad about a random axis, shifted, with noise on points and features; `thin`: the
    neighbourhood's third axis scaled by 0.005 (one lidar ring).  -> (G, H [n, 32, 4], dT [n, 4, 4] random)"""
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(n, K, 3, generator=g, dtype=torch.float64) * 2.0
    if thin:
        pts[..., 2] *= 0.005
    feat = torch.rand(n, K, 32, generator=g, dtype=torch.float64) + 0.05
    ax = torch.randn(n, 3, generator=g, dtype=torch.float64)
    ax = ax / ax.norm(dim=-1, keepdim=True)
    Kx = torch.zeros(n, 3, 3, dtype=torch.float64)
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0], Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    rot = torch.eye(3, dtype=torch.float64) + float(torch.sin(torch.tensor(angle))) * Kx + (1 - float(torch.cos(torch.tensor(angle)))) * Kx @ Kx
    shift = torch.randn(n, 1, 3, generator=g, dtype=torch.float64)
    tpts = pts @ rot.transpose(1, 2) + shift + 0.02 * torch.randn(n, K, 3, generator=g, dtype=torch.float64)
    tfeat = feat + 0.02 * torch.randn(n, K, 32, generator=g, dtype=torch.float64)

    def moment(p, f):
        Fr = torch.einsum("nkc,nke->nce", f, torch.cat([torch.ones_like(p[..., :1]), p], dim=-1))
        return Fr / (Fr[..., 0].sum(dim=-1)[:, None, None] + 1e-6)

    dT = torch.randn(n, 4, 4, generator=g, dtype=torch.float64)
    return moment(pts, feat).float(), moment(tpts, tfeat).float(), dT.float()


def conditioning(G, H):
    """(max s1 / (s2 + d s3), max s1 / s3, number of pairs with d = -1) of the pairs' cross moments, in fp64: how far the case
    stands from the rotation's singularity"""
    S, d = spectrum(G.double(), H.double())
    return float((S[:, 0] / (S[:, 1] + d * S[:, 2])).max()), float((S[:, 0] / S[:, 2]).max()), int((d < 0).sum())
