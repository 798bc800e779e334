"""Staged reference of the camera-matrix gradient of csrc/pair.hip (nerf_pair_backward_cam), in the style of
tests/pair_ssim_ref.py, and the checks of one input set (PairCamRef), shared by the GPU module and by the
CPU module's torch emulation.

The reference is helpers.pair_loss_ref (pair_ssim_ref.pair_ssim_loss_ref for the with_ssim term) with the
camera matrix expanded to a per-point leaf [P][4][4], used through a batched torch.linalg.inv in both
unprojections and directly in the projection h3 = K[:3] [q, 1]; nn, valid and bad are given.  Then
gK = sum_p grad_p is what autograd gives a single K used in all those places, and cond16 = sum_p |grad_p|
is the condition sum of that sum: the bar of every entry is PAIR_T_G13 cond16 + F32_MARGIN E_f32, the
bar g13 has, E_f32 the error of the same reference run in f32.  A clamped point (bad) has the constant
q = (nl, nl, nl), which gives R, t and the depths nothing, but its projection still depends on K."""
import torch

from tests import helpers as H
from tests import pair_ssim_ref as S

K_MODES = ("per_point", "shared", "fixed")


def _staged(inp, nn, valid, bad, go_pc, go_rgbs, detach, dtype, ssim, k_mode="per_point"):
    """The staged pair terms at dtype with K as a per-point leaf [P][4][4] ("per_point"), one shared leaf
    [4][4] ("shared") or a constant ("fixed": pc1, pc2 and h3 keep their gradients instead, for the
    emulation) -> dict(total, K leaf, and the intermediates)."""
    from oracle import nerf_oracle as orc
    c = H._pair_cast(inp, dtype)
    h, w, P = c["h"], c["w"], c["h"] * c["w"]
    assert k_mode in K_MODES
    if k_mode == "per_point":
        leaf = Kp = c["K"].expand(P, 4, 4).clone().requires_grad_(True)
    elif k_mode == "shared":
        leaf = c["K"].clone().requires_grad_(True)
        Kp = leaf.expand(P, 4, 4)
    else:
        leaf, Kp = None, c["K"].expand(P, 4, 4)
    Kinv = torch.linalg.inv(Kp)
    pix = H._pair_pixels(h, w, dtype)
    hom = [torch.stack([pix[:, 0] * d, pix[:, 1] * d, d, torch.ones_like(d)], 1) for d in (c["d1"], c["d2"])]
    b4 = [torch.einsum("pij,pj->pi", Kinv, v) for v in hom]           # inv(K) v, all four rows
    pc1, pc2 = b4[0][:, :3], b4[1][:, :3]
    if k_mode == "fixed":
        pc1, pc2 = pc1.detach().requires_grad_(True), pc2.detach().requires_grad_(True)
    R, t = c["Rt"][:3, :3], c["Rt"][:3, 3]
    s1 = 1.0 if c["s1"] is None else c["s1"]
    X = (pc1 / s1) @ R.t() + t
    Y = pc2 / s1
    a, b = nn[0].long(), nn[1].long()
    pc = torch.linalg.norm(X - Y[a], dim=1).mean() + torch.linalg.norm(Y - X[b], dim=1).mean()
    total = torch.zeros((), dtype=dtype)
    if go_pc is not None:
        total = total + go_pc * pc
    out = dict(leaf=leaf, Kinv=Kinv.detach(), b4=[v.detach() for v in b4], pc1=pc1, pc2=pc2, h3=None, q=None, P=P)
    if c["img1"] is not None:
        pr = pc1.detach() if detach else pc1
        q = pr @ R.t() + t
        q = torch.where(bad[:, None], torch.full_like(q, c["nl"]), q)
        h3 = torch.einsum("pij,pj->pi", Kp[:, :3, :3], q) + Kp[:, :3, 3]
        if k_mode == "fixed":           # a zero leaf added to h3 collects gh whatever h3 depends on
            e3 = torch.zeros(P, 3, dtype=dtype, requires_grad=True)
            h3 = h3 + e3
        p_re = h3[:, :2] / h3[:, 2:]
        rgb1 = orc.grid_values(c["img1"][None], pix[None])
        rgb2 = orc.grid_values(c["img2"][None], p_re[None])
        rgb_s = orc.rgb_s_loss_ref(rgb1.view(1, h, w, 3), rgb2.view(1, h, w, 3), valid.view(1, h, w, 1),
                                   **(dict(with_ssim=True) if ssim else {}))
        if go_rgbs is not None:
            total = total + go_rgbs * rgb_s
        out.update(h3=e3 if k_mode == "fixed" else h3, q=q.detach())
    out["total"] = total
    return out


def pair_cam_loss_ref(inp, nn, valid, bad, go_pc=1.0, go_rgbs=None, detach=False, dtype=torch.float64, ssim=False):
    """-> dict(gK [16] = sum_p grad_p, cond16 [16] = sum_p |grad_p|) of the per-point K leaf.  A total without
    grad (no live point and go_pc absent) gives zeros."""
    st = _staged(inp, nn, valid, bad, go_pc, go_rgbs, detach, dtype, ssim, "per_point")
    if st["total"].requires_grad:
        st["total"].backward()
    g = torch.zeros_like(st["leaf"]) if st["leaf"].grad is None else st["leaf"].grad
    g = g.reshape(st["P"], 16)
    return dict(gK=g.sum(0), cond16=g.abs().sum(0))


def shared_leaf_gK(inp, nn, valid, bad, go_pc, go_rgbs, detach, ssim=False):
    """fp64 autograd of one K leaf [4][4] shared by every use -> [16]."""
    st = _staged(inp, nn, valid, bad, go_pc, go_rgbs, detach, torch.float64, ssim, "shared")
    if not st["total"].requires_grad:
        return torch.zeros(16, dtype=torch.float64)
    st["total"].backward()
    return st["leaf"].grad.reshape(16)


class PairCamRef(H.PairRef):
    """PairRef with the camera gradient: refs_cam are pair_cam_loss_ref's at f64 and f32, the bar PairRef.bar
    per row of K at T = PAIR_T_G13 cond16; an entry with cond16 == 0 must be exactly 0."""

    def refs_cam(self, nn, combo, detach, ssim):
        nn = nn.detach().cpu().view(2, self.P).long()
        key = ("cam", combo, bool(detach), bool(ssim), hash(nn.numpy().tobytes()))
        if key not in self._refs:
            go_pc, go_rgbs = H.PAIR_COMBOS[combo]
            self._refs[key] = tuple(pair_cam_loss_ref(self.inp, nn, self.dec["valid"], self.dec["bad"], go_pc, go_rgbs,
                                                      bool(detach), dt, ssim) for dt in (torch.float64, torch.float32))
        return self._refs[key]

    def check_gK(self, gK16, nn, combo, detach, ssim, where=""):
        r64, r32 = self.refs_cam(nn, combo, detach, ssim)
        where = f"{where} cam{' ssim' if ssim else ''} {combo} detach={int(detach)}"
        got = gK16.detach().cpu().reshape(16)
        for r in range(4):
            sl = slice(4 * r, 4 * r + 4)
            self.bar(f"gK[{r}]", got[sl], r64["gK"][sl], r32["gK"][sl], H.PAIR_T_G13 * r64["cond16"][sl], where)
        zero = r64["cond16"] == 0
        assert bool((got[zero] == 0).all()), f"{where}: gK entries {zero.nonzero().flatten().tolist()} have no term: " \
                                             f"{got[zero].tolist()}"
        return r64


# ---- a torch-f32 emulation of the kernel's per-point accumulation (CPU module) -----------------------------
CAM_WRONG = ("no_inverse", "diagonal_only", "detach_ignored", "no_pc2")


def emulate_cam(inp, nn, valid, bad, combo, detach, ssim=False, wrong=None):
    """What k_pair_bwd_points<., CAM> adds up, in torch f32: with g the gradient arriving at pc1 / pc2 and gh
    the one at h3, per point -a1 b1^T - a2 b2^T (a = inv(K)^T[:, :3] g, b = inv(K) v) plus gh (x) [q, 1] on
    rows 0-2, then the sum over the points.  wrong: one of CAM_WRONG."""
    assert wrong is None or wrong in CAM_WRONG
    go_pc, go_rgbs = H.PAIR_COMBOS[combo]
    det = bool(detach) and wrong != "detach_ignored"
    st = _staged(inp, nn, valid, bad, go_pc, go_rgbs, det, torch.float32, ssim, "fixed")
    P = st["P"]
    if st["total"].requires_grad:
        st["total"].backward()
    z = lambda t: torch.zeros(P, 3) if (t is None or t.grad is None) else t.grad      # noqa: E731
    g1, g2, gh = z(st["pc1"]), z(st["pc2"]), z(st["h3"])
    Kinv = st["Kinv"][0]
    gK = torch.zeros(P, 4, 4)
    if wrong != "no_inverse":
        for g, b in ((g1, st["b4"][0]), (g2, st["b4"][1])):
            if wrong == "no_pc2" and g is g2:
                continue
            a = g @ Kinv[:3, :]                                          # [P][4]: inv(K)^T[:, :3] g
            gK = gK - a[:, :, None] * b[:, None, :]
    if st["q"] is not None:
        q1 = torch.cat([st["q"], torch.ones(P, 1)], 1)
        gK[:, :3, :] = gK[:, :3, :] + gh[:, :, None] * q1[:, None, :]
    if wrong == "diagonal_only":
        gK = gK * torch.eye(4)
    return gK.sum(0).reshape(16)


def emulation_nn(inp):
    """The neighbours of the f32 points (what a correct forward returns)."""
    pts = H.pair_points(inp, torch.float32)
    return torch.stack([H.pair_neighbours(pts["X"], pts["Y"])[1], H.pair_neighbours(pts["Y"], pts["X"])[1]])


def cam_runs(with_img):
    """(combo, detach, ssim) of one input set: the three PAIR_COMBOS x detach x {plain, SSIM}; without images
    there is the chamfer term alone."""
    if not with_img:
        return [("pc", 0, False)]
    return [(c, d, s) for s in (False, True) for c in H.PAIR_COMBOS for d in (0, 1)]


def check_emulation(inp, wrong=None, runs=None):
    ref = PairCamRef(inp)
    nn = emulation_nn(inp)
    for combo, detach, ssim in (cam_runs(inp["img1"] is not None) if runs is None else runs):
        got = emulate_cam(inp, nn, ref.dec["valid"], ref.dec["bad"], combo, detach, ssim, wrong)
        ref.check_gK(got, nn, combo, detach, ssim, "emulation")
    return ref
