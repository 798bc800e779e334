"""Staged reference of the with_ssim reprojection term of csrc/pair.hip (nerf_pair_forward_ssim /
nerf_pair_backward_ssim), in the style of tests/helpers.py::pair_loss_ref, and the checks of one input
set (PairSsimRef), shared by the GPU module and by the CPU module's torch emulation.

The term is oracle/nerf_oracle.py::rgb_s_loss_ref(..., with_ssim=True) on the (1, h, w, 3) samples.  The
SSIM module reads them as NCHW (C = image row, H = image column, W = colour), so the 3 x 3 window of
(row r, column c, colour k) covers columns c-1 .. c+1 of row r and colours k-1 .. k+1, both reflected
without repeating the edge; rows never mix.  `ssim_map_walked` is that rule walked by hand, `ssim_taps`
/ `ssim_moments` the same rule as index tables (what the emulation and its wrong variants use)."""
import torch

from tests import helpers as H

SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2
SSIM_D_MAP = 1e-6          # every map value of a valid output at least this far from 0 and 1
# seeds of the generic sets under with_ssim; a set whose PAIR_SEEDS / default seed breaks a condition of
# PairSsimRef has another one here
PAIR_SSIM_SEEDS = {(2, 2, "narrow"): 2, (2, 3, "narrow"): 2}      # the default seeds leave no corner valid


def ssim_inputs(h, w, camera="diag"):
    return H.pair_generic_inputs(h, w, camera, seed=PAIR_SSIM_SEEDS.get((h, w, camera)))


def narrow_inputs(h, w):
    """2 x 2, 3 x 2, 2 x 3: a near-identity pose (a tenth of the generic rotation and translation), so
    that points of so small a frame stay valid."""
    inp = H.pair_generic_inputs(h, w, "diag", seed=PAIR_SSIM_SEEDS.get((h, w, "narrow"), 31 * h + w))
    inp["Rt"] = H.pair_pose(t=(0.005, -0.002, 0.03), r=(0.005, -0.003, 0.002))
    return inp


def constant_inputs(h=5, w=9):
    """img1 = img2 = 0.5 and a pose that moves every point away from the camera, so that all project
    inside the frame: no window holds a padded sample, sigma = 0 and map = 0 everywhere."""
    inp = H.pair_generic_inputs(h, w, "diag", seed=PAIR_SSIM_SEEDS.get((h, w, "const"), 77))
    inp["Rt"] = H.pair_pose(t=(0.0, 0.0, -0.3), r=(0.005, -0.003, 0.002))
    inp["img1"] = torch.full((3, h, w), 0.5)
    inp["img2"] = torch.full((3, h, w), 0.5)
    return inp


# ---- the window rule ---------------------------------------------------------------------------------
def _reflect(t, n):
    return -t if t < 0 else (2 * (n - 1) - t if t >= n else t)


def ssim_map_walked(x, y):
    """x, y [h][w][3] -> map [h][w][3]: the window rule walked tap by tap (python loops, any dtype)."""
    h, w, _ = x.shape
    out = torch.zeros_like(x)
    for r in range(h):
        for c in range(w):
            for k in range(3):
                taps = [(r, _reflect(c + dc, w), _reflect(k + dk, 3)) for dc in (-1, 0, 1) for dk in (-1, 0, 1)]
                xs = torch.stack([x[t] for t in taps])
                ys = torch.stack([y[t] for t in taps])
                mx, my = xs.sum() / 9, ys.sum() / 9
                sx, sy, sxy = (xs * xs).sum() / 9 - mx * mx, (ys * ys).sum() / 9 - my * my, (xs * ys).sum() / 9 - mx * my
                n = (2 * mx * my + SSIM_C1) * (2 * sxy + SSIM_C2)
                d = (mx * mx + my * my + SSIM_C1) * (sx + sy + SSIM_C2)
                out[r, c, k] = ((1 - n / d) / 2).clamp(0, 1)
    return out


def ssim_taps(h, w, wrong=None):
    """-> (col [P][3] flat index of each column tap, wc [P][3] its weight, ct [3][3] colour taps, wk [3][3]).
    wrong: "flat_index" (the window over i - 1, i, i + 1 of the flat index: crosses row ends),
    "colour_clamped" (colour -1 -> 0, 3 -> 2), "multiplicity_one" (a column the reflection brings in twice
    counted once)."""
    P = h * w
    i = torch.arange(P)
    if wrong == "flat_index":
        col = torch.stack([torch.tensor([_reflect(int(t) + d, P) for t in i]) for d in (-1, 0, 1)], 1)
    else:
        r, c = i // w, i % w
        col = torch.stack([r * w + torch.tensor([_reflect(int(t) + d, w) for t in c]) for d in (-1, 0, 1)], 1)
    wc = torch.ones(P, 3, dtype=torch.float64)
    if wrong == "multiplicity_one":
        wc[:, 2] = (col[:, 2] != col[:, 0]).double()
    if wrong == "colour_clamped":
        ct = torch.tensor([[0, 0, 1], [0, 1, 2], [1, 2, 2]])
    else:
        ct = torch.tensor([[1, 0, 1], [0, 1, 2], [1, 2, 1]])
    return col, wc, ct, torch.ones(3, 3, dtype=torch.float64)


def ssim_moments(x, y, taps):
    """x, y [P][3] -> dict of [P][3] window moments (mean x, y, x^2, y^2, xy) and the quotient's parts."""
    col, wc, ct, wk = taps
    W = (wc[:, :, None, None] * wk[None, None]).to(x.dtype)          # [P][a][k'][b]
    xg, yg = x[col][:, :, ct], y[col][:, :, ct]
    m = lambda v: (W * v).sum((1, 3)) / 9                            # noqa: E731
    mx, my, xx, yy, xy = m(xg), m(yg), m(xg * xg), m(yg * yg), m(xg * yg)
    A1, A2 = 2 * mx * my + SSIM_C1, 2 * (xy - mx * my) + SSIM_C2
    B1, B2 = mx * mx + my * my + SSIM_C1, (xx - mx * mx) + (yy - my * my) + SSIM_C2
    n, d = A1 * A2, B1 * B2
    return dict(mx=mx, my=my, A1=A1, A2=A2, B1=B1, B2=B2, n=n, d=d, raw=(1 - n / d) / 2)


# ---- the staged reference ---------------------------------------------------------------------------
def _oracle_term(rgb1, rgb2, valid):
    from oracle import nerf_oracle as orc
    return orc.rgb_s_loss_ref(rgb1, rgb2, valid, with_ssim=True)


def pair_ssim_loss_ref(inp, nn, valid, bad, go_pc=1.0, go_rgbs=None, detach=False, dtype=torch.float64, term=None,
                       keep=False):
    """helpers.pair_loss_ref with the with_ssim term: same leaves (per-point R, t, s1), nn, valid and bad
    given.  term(rgb1 [1,h,w,3], rgb2, valid [1,h,w,1]) -> scalar: the oracle expression unless the CPU
    module's emulation passes its own.  keep: also return the samples and the fp64-dtype map."""
    from oracle import nerf_oracle as orc
    term = _oracle_term if term is None else term
    c = H._pair_cast(inp, dtype)
    h, w, P = c["h"], c["w"], c["h"] * c["w"]
    leaf = lambda t: t.clone().requires_grad_(True)      # noqa: E731
    d1, d2 = leaf(c["d1"]), leaf(c["d2"])
    Rp, tp = leaf(c["Rt"][:3, :3].expand(P, 3, 3)), leaf(c["Rt"][:3, 3].expand(P, 3))
    sp = leaf((torch.ones(1, dtype=dtype) if c["s1"] is None else c["s1"]).expand(P, 1))
    pix = H._pair_pixels(h, w, dtype)
    Kinv = torch.linalg.inv(c["K"])
    pc1, pc2 = H._pair_unproject(pix, d1, Kinv), H._pair_unproject(pix, d2, Kinv)
    X = torch.einsum("pij,pj->pi", Rp, pc1 / sp) + tp
    Y = pc2 / sp
    a, b = nn[0].long(), nn[1].long()
    pc = torch.linalg.norm(X - Y[a], dim=1).mean() + torch.linalg.norm(Y - X[b], dim=1).mean()
    total = torch.zeros((), dtype=dtype)
    if go_pc is not None:
        total = total + go_pc * pc
    K3 = c["K"][:3]
    pr = pc1.detach() if detach else pc1
    q = torch.einsum("pij,pj->pi", Rp, pr) + tp
    q = torch.where(bad[:, None], torch.full_like(q, c["nl"]), q)
    h3 = q @ K3[:, :3].t() + K3[:, 3]
    p_re = h3[:, :2] / h3[:, 2:]
    rgb1 = orc.grid_values(c["img1"][None], pix[None])
    rgb2 = orc.grid_values(c["img2"][None], p_re[None])
    rgb_s = term(rgb1.view(1, h, w, 3), rgb2.view(1, h, w, 3), valid.view(1, h, w, 1))
    if go_rgbs is not None:
        total = total + go_rgbs * rgb_s
    if total.requires_grad:
        total.backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    gR, gt, gs = z(Rp), z(tp), z(sp)
    g13 = torch.cat([gR.sum(0).reshape(9), gt.sum(0), gs.sum().reshape(1)])
    cond13 = torch.cat([gR.abs().sum(0).reshape(9), gt.abs().sum(0), gs.abs().sum().reshape(1)])
    out = dict(pc=pc.detach(), rgb_s=rgb_s.detach(), g_d1=z(d1), g_d2=z(d2), g13=g13, cond13=cond13)
    if keep:
        out.update(rgb1=rgb1.detach().view(P, 3), rgb2=rgb2.detach().view(P, 3), p=p_re.detach())
    return out


def row_near(mask, h, w):
    """[P] bool: the point or a neighbour within one column of its row is in `mask`."""
    m = mask.view(h, w)
    out = m.clone()
    out[:, 1:] |= m[:, :-1]
    out[:, :-1] |= m[:, 1:]
    return out.reshape(-1)


class PairSsimRef(H.PairRef):
    """PairRef for the with_ssim entries: refs are pair_ssim_loss_ref's, bars and their form PairRef's.
    Conditions asserted on the inputs in fp64 before any comparison: pair_assert_conditions as it is
    (need_sign=False leaves its sign-of-difference condition to the case's own argument); the cell-edge
    and sign distances over every unclamped point whose sample enters a valid point's window; every map
    value of a valid output SSIM_D_MAP away from 0 and 1 (need_map); an invalid point with a non-zero fp64
    g_d1 (need_invalid_grad); at least one valid point (need_valid)."""

    def __init__(self, inp, device=None, generic=True, need_map=True, need_invalid_grad=True, need_sign=True,
                 need_valid=True):
        from oracle import nerf_oracle as orc
        if need_sign:
            super().__init__(inp, device, generic)
        else:
            self.inp, self.P, self.device, self.generic = inp, inp["h"] * inp["w"], device, generic
            self.with_img = True
            self.pts64, self.pts32 = H.pair_points(inp, torch.float64), H.pair_points(inp, torch.float32)
            dec = self.dec = H.pair_decisions(inp)
            assert dec["d_valid"].min().item() >= H.PAIR_D_VALID and dec["d_bad"].min().item() >= H.PAIR_D_BAD
            assert dec["d_cell"] >= H.PAIR_D_CELL, ("bilinear cell edge", dec["d_cell"])
            self.worst, self._refs = {}, {}
        assert self.with_img
        h, w, P = inp["h"], inp["w"], self.P
        valid, bad = self.dec["valid"], self.dec["bad"]
        assert not need_valid or bool(valid.any()), "no valid point"
        nn0 = torch.zeros(2, P, dtype=torch.long)
        r = pair_ssim_loss_ref(inp, nn0, valid, bad, None, 1.0, False, torch.float64, keep=True)
        self.enters = row_near(valid, h, w) & ~bad
        if bool(self.enters.any()):
            wh = torch.tensor([w - 1, h - 1], dtype=torch.float64)
            ij = (r["p"][self.enters] + 1) * 0.5 * wh
            d_cell = ((ij - ij.round()).abs() * 2 / wh).min().item()
            assert d_cell >= H.PAIR_D_CELL, ("bilinear cell edge of a window input", d_cell)
            if need_sign:
                d_sign = (r["rgb1"] - r["rgb2"])[self.enters].abs().min().item()
                assert d_sign >= H.PAIR_D_SIGN, ("sign of img1 - img2 of a window input", d_sign)
        self.map64 = orc.ssim_map(r["rgb1"].view(1, h, w, 3), r["rgb2"].view(1, h, w, 3)).view(P, 3)
        if need_map and bool(valid.any()):
            mv = self.map64[valid]
            assert mv.min().item() >= SSIM_D_MAP and mv.max().item() <= 1 - SSIM_D_MAP, (mv.min().item(), mv.max().item())
        self.n_invalid_grad = int(((r["g_d1"] != 0) & ~valid).sum())
        assert not need_invalid_grad or self.n_invalid_grad > 0, "no invalid point with a gradient"

    def refs(self, nn, combo, detach):
        nn = nn.detach().cpu().view(2, self.P).long()
        key = (combo, bool(detach), hash(nn.numpy().tobytes()))
        if key not in self._refs:
            go_pc, go_rgbs = H.PAIR_COMBOS[combo]
            self._refs[key] = tuple(pair_ssim_loss_ref(self.inp, nn, self.dec["valid"], self.dec["bad"], go_pc, go_rgbs,
                                                       bool(detach), dt) for dt in (torch.float64, torch.float32))
        return self._refs[key]

    def check_grads(self, g, nn, combo, detach, where=""):
        r64, r32 = self.refs(nn, combo, detach)
        where = f"{where} ssim {combo} detach={int(detach)}"
        for name in ("g_d1", "g_d2"):
            self.bar(name, g[name], r64[name], r32[name], H.PAIR_T_ELEM * r64[name].abs().max().item(), where)
        g13 = g["g13"].detach().cpu()
        for name, sl in (("dR", slice(0, 9)), ("dt", slice(9, 12)), ("ds1", slice(12, 13))):
            self.bar(name, g13[sl], r64["g13"][sl], r32["g13"][sl], H.PAIR_T_G13 * r64["cond13"][sl], where)
        if combo == "rgbs":
            g_d1 = g["g_d1"].detach().cpu()
            valid, bad = self.dec["valid"], self.dec["bad"]
            assert bool((g["g_d2"].detach().cpu() == 0).all()), f"{where}: g_d2 from rgb_s alone"
            assert bool((g_d1[bad] == 0).all()), f"{where}: g_d1 of a clamped point"
            alone = ~row_near(valid, self.inp["h"], self.inp["w"])          # invalid, no valid row neighbour
            assert bool((g_d1[alone] == 0).all()), f"{where}: g_d1 of a point in no valid point's window"
            if detach:
                assert bool((g_d1 == 0).all()), f"{where}: g_d1 through a detached scale"
            assert g13[12].item() == 0.0, f"{where}: ds1 from rgb_s alone"
            if not bool(valid.any()):
                assert bool((g13 == 0).all()) and bool((g_d1 == 0).all()), f"{where}: nothing valid"


# ---- a torch emulation of the kernels' algorithm (CPU module) -------------------------------------------
class _EmuTerm(torch.autograd.Function):
    """What k_pair_ssim and ssim_grad_rgb2 do: the f32 samples are kept; windows, quotient and blend in
    fp64 from them; N = 3 n_valid; the backward gathers, per input (i, k), over the outputs of columns
    c-1 .. c+1 of its row and the colours whose window holds k, with the reflection's multiplicity."""

    @staticmethod
    def forward(ctx, rgb1, rgb2, valid, wrong):
        _, h, w, _ = rgb1.shape
        P = h * w
        x, y, v = rgb1.reshape(P, 3).double(), rgb2.reshape(P, 3).double(), valid.reshape(P)
        if wrong == "mask_on_inputs":
            x, y = x * v[:, None], y * v[:, None]
        taps = ssim_taps(h, w, wrong)
        M = ssim_moments(x, y, taps)
        outmask = torch.ones_like(v) if wrong == "mask_on_inputs" else v
        ad = (x - y).abs().clamp(0, 1)
        blend = (0.15 * ad + 0.85 * M["raw"].clamp(0, 1)).float()
        N = 3.0 * float(v.sum())
        ctx.save_for_backward(x, y, v, outmask)
        ctx.taps, ctx.M, ctx.N, ctx.wrong, ctx.shape = taps, M, N, wrong, rgb2.shape
        return (blend[outmask].sum() / N if N > 0 else torch.zeros(())).to(rgb2.dtype)

    @staticmethod
    def backward(ctx, go):
        x, y, v, outmask = ctx.saved_tensors
        (col, wc, ct, wk), M, N, wrong = ctx.taps, ctx.M, ctx.N, ctx.wrong
        P = x.shape[0]
        if N == 0:
            return None, torch.zeros(ctx.shape, dtype=go.dtype), None, None
        i = torch.arange(P)
        cwm = torch.stack([torch.stack([(wk[kp] * (ct[kp] == k)).sum() for k in range(3)]) for kp in range(3)])   # [k'][k]
        passes = ((M["raw"] >= 0) & (M["raw"] <= 1)).double()
        acc = torch.zeros(P, 3, dtype=torch.float64)
        for dj in (-1, 0, 1):
            j = (i + dj).clamp(0, P - 1)
            mult = (wc[j] * (col[j] == i[:, None])).sum(1) * ((i + dj >= 0) & (i + dj < P)) * outmask[j]
            for kp in range(3):
                g = lambda name: M[name][j, kp][:, None]      # noqa: E731
                dn = (2 * g("mx") * g("A2") + g("A1") * 2 * (x - g("mx"))) / 9
                dd = (2 * g("my") * g("B2") + g("B1") * 2 * (y - g("my"))) / 9
                dmap = -(dn * g("d") - g("n") * dd) / (2 * g("d") * g("d")) * passes[j, kp][:, None]
                acc += mult[:, None] * cwm[kp][None] * dmap
        e = x - y
        ab = -torch.sign(e) * (e.abs() <= 1) * (v if wrong != "mask_on_inputs" else outmask)[:, None]
        gy = (go.double() / N) * (0.85 * acc + 0.15 * ab)
        if wrong == "mask_on_inputs":
            gy = gy * v[:, None]
        if wrong == "valid_only":
            gy = gy * v[:, None]
        return None, gy.to(go.dtype).view(ctx.shape), None, None


def emulate_ssim(inp, wrong=None):
    """What a correct kernel family returns under with_ssim (out3 and the gradients of `both` and `rgbs`,
    detach 0 and 1), decisions in f32 on its own points; `wrong` makes it one of the wrong kernels."""
    P = inp["h"] * inp["w"]
    pts = H.pair_points(inp, torch.float32)
    D = lambda Q, R: (Q[:, None, :] - R[None, :, :]).square().sum(-1)      # noqa: E731
    nn = torch.stack([D(pts["X"], pts["Y"]).argmin(1), D(pts["Y"], pts["X"]).argmin(1)])
    dec = H.pair_decisions(inp, torch.float32)
    term = lambda a, b, v: _EmuTerm.apply(a, b, v.bool(), wrong)           # noqa: E731
    fw = pair_ssim_loss_ref(inp, nn, dec["valid"], dec["bad"], 1.0, 1.0, False, torch.float32, term=term)
    out3 = torch.stack([fw["pc"], fw["rgb_s"], 3.0 * dec["valid"].sum()]).float()
    grads = {}
    for combo in ("both", "rgbs"):
        for detach in (0, 1):
            go_pc, go_rgbs = H.PAIR_COMBOS[combo]
            grads[combo, detach] = pair_ssim_loss_ref(inp, nn, dec["valid"], dec["bad"], go_pc, go_rgbs, bool(detach),
                                                      torch.float32, term=term)
    return dict(nn=nn, out3=out3, grads=grads)


def check_emulation(inp, got, **kw):
    ref = PairSsimRef(inp, **kw)
    ref.check_out3(got["out3"], got["nn"])
    for (combo, detach), g in got["grads"].items():
        ref.check_grads(g, got["nn"], combo, detach)
    return ref
