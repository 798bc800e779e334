"""The ray prologue, the loss epilogue, Adam and the weight pack (csrc/rays.hip, csrc/misc.hip)
against fp64 at the shapes where each launch geometry changes (GPU only), through the C ABI.

References and inputs: tests/helpers.py (their own checks: tests/test_prologue_reference_cpu.py).
Bars: the sampler, the forward of the depth affine, the gathers and the pack images are exact; a value
is held to T max|ref| + 4 E_f32 (helpers.f32_bar) with T the fixed tolerance tests/test_gpu_rays.py
already uses (1e-5 for values, 1e-4 for gradients) and E_f32 the plain f32 reference's own distance to
fp64 on the same inputs; a one-workgroup sum to helpers.tree_ceiling times the sum of |term|; Adam to
4 E_f32 + 4 ulp of the largest entry.  Every output is a helpers.Guarded buffer: the sentinels around it
survive every call, and an output the call was told not to write keeps the sentinel everywhere."""
import pytest
import torch

from model import _hip
from model.optim import hyper_block
from oracle import nerf_oracle as orc
from tests import helpers as H
from tests.helpers import Guarded, T_GRAD, T_VALUE

pytestmark = pytest.mark.gpu

INT_FILL = -7


def _report(test, worst):
    for name, (ratio, e32) in worst.items():
        H.report_err(test, name, ratio)
        H.report_err(test, name + ":E_f32", e32)


def _intact(where, **bufs):
    for name, b in bufs.items():
        assert b.intact(), f"{where}: wrote outside {name}"


# ---- the sampler ------------------------------------------------------------------------------------
def _sample(dev, n, R, W, Hh, img, counter=None, with_pix=True, with_rgb=True):
    o = dict(idx=Guarded((R,), dev, torch.int64, INT_FILL), pix=Guarded((R, 2), dev), rgb=Guarded((R, 3), dev),
             status=Guarded((1,), dev, torch.int32, INT_FILL))
    _hip.sample_rays(n, R, H.SAMPLE_SEED, W, Hh, img if with_rgb else None, o["idx"].t, o["pix"].t if with_pix else None,
                     o["rgb"].t if with_rgb else None, o["status"].t, counter)
    torch.cuda.synchronize()
    _intact(f"sample n={n} R={R}", **o)
    return o


def _check_sample(o, ref_idx, rounds, Hh, W, img_c, where, with_pix=True, with_rgb=True):
    n = Hh * W
    assert torch.equal(o["idx"].t.cpu(), ref_idx), f"{where}: idx is not the reference draw"
    assert o["status"].t.item() == rounds, f"{where}: status {o['status'].t.item()} != {rounds} rounds"
    if with_pix:
        assert torch.equal(o["pix"].t.cpu(), orc.arange_pixels(Hh, W)[1][0][ref_idx]), f"{where}: pixels"
        assert torch.equal(o["pix"].t.cpu(), H.pixels_ref(ref_idx, Hh, W)), f"{where}: pixels_ref"
    else:
        assert o["pix"].untouched(), f"{where}: pixels written though NULL"
    if with_rgb:
        assert torch.equal(o["rgb"].t.cpu(), img_c.view(3, n).t()[ref_idx]), f"{where}: rgb gather"
    else:
        assert o["rgb"].untouched(), f"{where}: rgb written though NULL"


@pytest.mark.parametrize("Hh,W,R", H.SAMPLE_CASES)
def test_sampler_draws_the_reference_set(dev, Hh, W, R):
    """idx equals helpers.sample_rays_ref element for element (the header's draw rule: a race in the
    hash set that still yielded distinct values would not), status its round count, the gathers bit
    for bit; three launches on a device counter equal the reference at counters 0, 1, 2."""
    n = Hh * W
    img_c = torch.rand(3, Hh, W, generator=torch.Generator().manual_seed(R))
    img = img_c.to(dev)
    where = f"sample {Hh}x{W} R={R}"
    ref_idx, rounds = H.sample_rays_ref(n, R, H.SAMPLE_SEED)
    _check_sample(_sample(dev, n, R, W, Hh, img), ref_idx, rounds, Hh, W, img_c, where)
    ctr = Guarded((1,), dev, torch.int64, 0)
    for c in range(3):
        ref_c, rounds_c = H.sample_rays_ref(n, R, H.SAMPLE_SEED, counter=c)
        _check_sample(_sample(dev, n, R, W, Hh, img, counter=ctr.t), ref_c, rounds_c, Hh, W, img_c, f"{where} counter {c}")
        assert ctr.t.item() == c + 1 and ctr.intact()
        if R > 3:
            assert not torch.equal(ref_c, ref_idx)


@pytest.mark.parametrize("with_pix,with_rgb", [(True, False), (False, True), (False, False)])
def test_sampler_optional_outputs(dev, with_pix, with_rgb):
    Hh, W, R = 41, 50, 1025
    img_c = torch.rand(3, Hh, W, generator=torch.Generator().manual_seed(3))
    ref_idx, rounds = H.sample_rays_ref(Hh * W, R, H.SAMPLE_SEED)
    o = _sample(dev, Hh * W, R, W, Hh, img_c.to(dev), with_pix=with_pix, with_rgb=with_rgb)
    _check_sample(o, ref_idx, rounds, Hh, W, img_c, f"pix={with_pix} rgb={with_rgb}", with_pix, with_rgb)


# ---- the 4x4 chain --------------------------------------------------------------------------------
def _per_matrix(name, got, r64, r32, t_rel, where, worst):
    """The bar per matrix of the batch (one ill-conditioned matrix does not widen its neighbours' bars)."""
    got = got.detach().cpu()
    for i in range(r64.shape[0]):
        e32 = (r32[i].double() - r64[i]).abs().max().item()
        H.assert_max_bar(name, got[i], r64[i], e32, t_rel, f"{where} [{i}]", worst)


@pytest.mark.parametrize("n", H.MAT4_BATCHES)
def test_mat4_inverse_and_backward(dev, n):
    A = H.mat4_edge_batch(n)[0]
    g = torch.randn(n, 4, 4, generator=torch.Generator().manual_seed(n))
    worst, where = {}, f"mat4_inv n={n}"

    def run(dt):
        a = A.to(dt).clone().requires_grad_(True)
        y = torch.linalg.inv(a)
        y.backward(g.to(dt))
        return y.detach(), a.grad
    (y64, ga64), (y32, ga32) = run(torch.float64), run(torch.float32)
    out, ga = Guarded((n, 4, 4), dev), Guarded((n, 4, 4), dev)
    _hip.mat4_inv(A.to(dev), out.t)
    _hip.mat4_inv_bwd(out.t, g.to(dev), ga.t)
    torch.cuda.synchronize()
    _intact(where, out=out, ga=ga)
    _per_matrix("inv", out.t, y64, y32, T_VALUE, where, worst)
    _per_matrix("inv.g_a", ga.t, ga64, ga32, T_GRAD, where, worst)
    _report("prologue_mat4", worst)


@pytest.mark.parametrize("n", H.MAT4_BATCHES)
def test_mat4_mul_and_backward_forms(dev, n):
    A, B = H.mat4_edge_batch(n)[0], H.mat4_edge_batch(n, seed=50)[0].flip(0).contiguous()
    g = torch.randn(n, 4, 4, generator=torch.Generator().manual_seed(n + 1))
    worst, where = {}, f"mat4_mul n={n}"

    def run(dt):
        a, b = A.to(dt).clone().requires_grad_(True), B.to(dt).clone().requires_grad_(True)
        c = a @ b
        c.backward(g.to(dt))
        return c.detach(), a.grad, b.grad
    r64, r32 = run(torch.float64), run(torch.float32)
    Ad, Bd, gd = A.to(dev), B.to(dev), g.to(dev)
    c = Guarded((n, 4, 4), dev)
    _hip.mat4_mul(Ad, Bd, c.t)
    torch.cuda.synchronize()
    _intact(where, c=c)
    _per_matrix("mul", c.t, r64[0], r32[0], T_VALUE, where, worst)
    for want_a, want_b in ((True, True), (True, False), (False, True)):
        ga, gb = Guarded((n, 4, 4), dev), Guarded((n, 4, 4), dev)
        _hip.mat4_mul_bwd(Ad if want_b else None, Bd if want_a else None, gd, ga.t if want_a else None,
                          gb.t if want_b else None)
        torch.cuda.synchronize()
        _intact(where, ga=ga, gb=gb)
        w = f"{where} g_a={want_a} g_b={want_b}"
        for name, buf, want, k in (("mul.g_a", ga, want_a, 1), ("mul.g_b", gb, want_b, 2)):
            if want:
                _per_matrix(name, buf.t, r64[k], r32[k], T_GRAD, w, worst)
            else:
                assert buf.untouched(), f"{w}: {name} written though NULL"
    _report("prologue_mat4", worst)


@pytest.mark.parametrize("with_init", [True, False])
def test_pose_c2w_over_the_rotation_range(dev, with_init):
    """r from 0 through squares that underflow in f32 to beyond pi, with and without init_c2w, g_r-only
    and g_t-only.  At r = 0 the f32 torch expression is the reference of g_r (fp64 autograd is 0/0
    territory there, as tests/test_gpu_rays.py argues); everywhere g_r is finite."""
    gen = torch.Generator().manual_seed(11)
    init = H.rigid_c2w(5) if with_init else None
    u = torch.tensor(H.POSE_AXIS, dtype=torch.float64)
    worst = {}
    for scale in H.POSE_R_SCALES:
        r = (scale * u).float()
        t, g = torch.randn(3, generator=gen), torch.randn(4, 4, generator=gen)
        r64, e32, r32 = H.pose_c2w_refs(r, t, init, g)
        where = f"pose |r|={scale:g} init={with_init}"
        rd, td, gd = r.to(dev), t.to(dev), g.to(dev)
        init_d = None if init is None else init.contiguous().to(dev)
        out = Guarded((4, 4), dev)
        _hip.pose_c2w(rd, td, init_d, out.t)
        torch.cuda.synchronize()
        _intact(where, c2w=out)
        H.assert_max_bar("c2w", out.t, r64["c2w"], e32["c2w"], T_VALUE, where, worst)
        for want_r, want_t in ((True, True), (True, False), (False, True)):
            gr, gt = Guarded((3,), dev), Guarded((3,), dev)
            _hip.pose_c2w_bwd(rd, init_d, gd, gr.t if want_r else None, gt.t if want_t else None)
            torch.cuda.synchronize()
            _intact(where, g_r=gr, g_t=gt)
            if want_r:
                assert bool(torch.isfinite(gr.t).all()), f"{where}: g_r not finite"
                ref_r = r32["g_r"].double() if scale == 0.0 else r64["g_r"]
                H.assert_max_bar("pose.g_r", gr.t, ref_r, e32["g_r"], T_GRAD, where, worst)
            else:
                assert gr.untouched(), f"{where}: g_r written though NULL"
            if want_t:
                H.assert_max_bar("pose.g_t", gt.t, r64["g_t"], e32["g_t"], T_GRAD, where, worst)
            else:
                assert gt.untouched(), f"{where}: g_t written though NULL"
    _report("prologue_pose", worst)


def test_unproject_backward_each_output_absent(dev):
    b = H.synthetic_rays(R=8, seed=6)
    K, W, S = b["K"][0].contiguous(), b["w2c"][0].contiguous(), b["scale"][0].clone()      # torch.inverse is column-major
    S[:3, :3] *= 1.3
    g = torch.randn(4, 4, generator=torch.Generator().manual_seed(7))
    r64, e32 = H.unproject_refs(K, W, S, g)
    worst, where = {}, "unproject"
    M, invs = Guarded((4, 4), dev), Guarded((3, 4, 4), dev)
    _hip.unproject_matrix(K.to(dev), W.to(dev), S.to(dev), M.t, invs.t)
    torch.cuda.synchronize()
    _intact(where, M=M, inverses=invs)
    H.assert_max_bar("M", M.t, r64["M"], e32["M"], T_VALUE, where, worst)
    M2, invs2 = Guarded((4, 4), dev), Guarded((3, 4, 4), dev)
    _hip.unproject_matrix(K.to(dev), W.to(dev), S.to(dev), M2.t, None)
    torch.cuda.synchronize()
    assert torch.equal(M2.t, M.t) and M2.intact() and invs2.untouched()
    for absent in (None, "g_K", "g_W", "g_S"):
        outs = {k: Guarded((4, 4), dev) for k in ("g_K", "g_W", "g_S")}
        _hip.unproject_matrix_bwd(invs.t, g.to(dev), *[None if k == absent else outs[k].t for k in ("g_K", "g_W", "g_S")])
        torch.cuda.synchronize()
        _intact(where, **outs)
        for k, buf in outs.items():
            if k == absent:
                assert buf.untouched(), f"{where}: {k} written though NULL"
            else:
                H.assert_max_bar("unproject." + k, buf.t, r64[k], e32[k], T_GRAD, f"{where} without {absent}", worst)
    _report("prologue_unproject", worst)


# ---- the depth-prior distortion ---------------------------------------------------------------------
@pytest.mark.parametrize("n", H.AFFINE_N)
def test_depth_affine_at_every_grid_edge(dev, n):
    """One block, the last whole block, one element more, the 64-block cap, the grid stride behind it;
    the forward bit-equal to the f32 torch expression (entries exactly at lo kept, one ulp below it
    clamped), the one-workgroup backward inside its derived ceiling."""
    worst = {}
    for shift_first in (False, True):
        for lo in (float("-inf"), 0.5):
            inp = H.depth_affine_inputs(n, shift_first, lo)
            where = f"affine n={n} shift_first={shift_first} lo={lo}"
            ref = H.depth_affine_ref(inp["d"], inp["s"], inp["t"], shift_first, lo, inp["g"])
            pre = H.affine32(inp["d"], inp["s"], inp["t"], shift_first)
            y_ref = pre.clamp_min(lo) if lo != float("-inf") else pre
            dd, sd, td, gd = (inp[k].to(dev) for k in ("d", "s", "t", "g"))
            y = Guarded((n,), dev)
            _hip.depth_affine(dd, sd, td, shift_first, lo, y.t)
            torch.cuda.synchronize()
            _intact(where, y=y)
            assert torch.equal(y.t.cpu(), y_ref), f"{where}: forward is not the f32 expression"
            if inp["at_lo"]:
                assert bool((pre[inp["at_lo"]] == lo).all()) and bool(ref["keep"][inp["at_lo"]].all())
                assert bool((pre[inp["below"]] < lo).all()) and not bool(ref["keep"][inp["below"]].any())
            ceil = H.tree_ceiling(n, 1024)
            for want_s, want_t in ((True, True), (True, False), (False, True)):
                gs, gt = Guarded((1,), dev), Guarded((1,), dev)
                _hip.depth_affine_bwd(dd, sd, td, shift_first, lo, gd, gs.t if want_s else None, gt.t if want_t else None)
                torch.cuda.synchronize()
                _intact(where, g_scale=gs, g_shift=gt)
                for name, buf, want, k in (("affine.g_scale", gs, want_s, "s"), ("affine.g_shift", gt, want_t, "t")):
                    if want:
                        H.assert_sum_bar(name, buf.t, ref["g_" + k], ref["cond_" + k], ceil, 0.0, where, worst)
                    else:
                        assert buf.untouched(), f"{where}: {name} written though NULL"
    _report("prologue_affine", worst)


# ---- camera rays --------------------------------------------------------------------------------------
CAM_OUT = ("cam", "ray", "view", "ray_norm", "d_src")


def _camera_fwd(dev, inp, depth, flags, R, view=True, mask=True):
    o = dict(cam=Guarded((R, 3), dev), ray=Guarded((R, 3), dev), view=Guarded((R, 3), dev), ray_norm=Guarded((R,), dev),
             d_src=Guarded((R,), dev), mask=Guarded((R,), dev, torch.uint8, 0x5a))
    _hip.camera_rays(inp["M"].to(dev), inp["pix"].to(dev), None if depth is None else depth.to(dev), R, flags, o["cam"].t,
                     o["ray"].t, o["view"].t if view else None, o["ray_norm"].t, o["d_src"].t, o["mask"].t if mask else None)
    torch.cuda.synchronize()
    _intact(f"camera R={R} flags={flags}", **o)
    return o


@pytest.mark.parametrize("R", H.CAMERA_R)
def test_camera_rays_forward(dev, R):
    """All four flag values on a depth with zeros, negatives, one +inf and one NaN: the mask exactly,
    the values where the reference is finite; depth, view, mask each NULL in turn; without a depth
    d_src is exactly 1 under all four flag values."""
    inp = H.camera_inputs(R, nonfinite=True)
    worst = {}
    for flags in range(4):
        where = f"camera R={R} flags={flags}"
        r64, e32, r32 = H.camera_rays_refs(inp["M"], inp["pix"], inp["depth"], flags)
        o = _camera_fwd(dev, inp, inp["depth"], flags, R)
        assert torch.equal(o["mask"].t.cpu().bool(), r32["mask"]), f"{where}: mask"
        assert bool((o["mask"].t.cpu() <= 1).all())
        bad = inp["kinds"]["zero"] + inp["kinds"]["inf"] + inp["kinds"]["nan"]
        assert not bool(r32["mask"][bad].any()) and bool(r32["mask"][inp["kinds"]["neg"]].all())
        for name in CAM_OUT:
            H.assert_max_bar(name, o[name].t, r64[name], e32[name], T_VALUE, where, worst, finite=torch.isfinite(r64[name]))
        if inp["kinds"]["inf"]:
            assert not bool(torch.isfinite(o["d_src"].t[[1, 3]]).any()), f"{where}: d_src of a non-finite depth"
        if flags & 2:
            assert bool((o["view"].t == 1).all()), f"{where}: view with VIEW_ONES"
        else:
            assert torch.equal(o["view"].t, -o["ray"].t), f"{where}: view != -ray"
        # NULL arguments in turn
        r64n, e32n, _ = H.camera_rays_refs(inp["M"], inp["pix"], None, flags)
        on = _camera_fwd(dev, inp, None, flags, R)
        assert bool((on["d_src"].t == 1).all()), f"{where}: d_src != 1 without a depth"
        assert bool((on["mask"].t == 1).all())
        for name in ("cam", "ray", "view", "ray_norm"):
            assert torch.equal(on[name].t, o[name].t), f"{where}: {name} depends on the depth"
        assert bool((r64n["d_src"] == 1).all())
        ov = _camera_fwd(dev, inp, inp["depth"], flags, R, view=False)
        assert ov["view"].untouched() and torch.equal(ov["ray"].t, o["ray"].t)
        om = _camera_fwd(dev, inp, inp["depth"], flags, R, mask=False)
        assert om["mask"].untouched() and torch.equal(om["d_src"].t.nan_to_num(7.0), o["d_src"].t.nan_to_num(7.0))
    _report("prologue_camera", worst)


GRADS = ("g_cam", "g_ray", "g_view", "g_norm", "g_dsrc")


def _camera_bwd(dev, inp, depth, flags, R, grads, want_depth=True):
    gM, gd = Guarded((4, 4), dev), Guarded((R,), dev)
    _hip.camera_rays_bwd(inp["M"].to(dev), inp["pix"].to(dev), None if depth is None else depth.to(dev), R, flags,
                         *[None if grads.get(k) is None else grads[k].to(dev) for k in GRADS], gM.t,
                         gd.t if want_depth else None)
    torch.cuda.synchronize()
    _intact(f"camera_bwd R={R} flags={flags}", gM=gM, g_depth=gd)
    return gM, gd


@pytest.mark.parametrize("R", H.CAMERA_R)
def test_camera_rays_backward(dev, R):
    """gM inside the one-workgroup ceiling of each entry's fp64 per-ray terms (+ 4 E_f32), g_depth per
    element; every upstream gradient absent in turn, g_depth NULL, depth NULL; row 3 of gM and g_depth at
    d = 0 exactly 0.  The depths are finite here (zeros and negatives): a non-finite depth has no
    gradient to compare."""
    inp = H.camera_inputs(R)
    zero = inp["kinds"]["zero"]
    ceil = H.tree_ceiling(R, 1024)
    worst = {}
    for flags in range(4):
        for absent in (None,) + GRADS:
            grads = {k: (None if k == absent else inp[k]) for k in GRADS}
            where = f"camera_bwd R={R} flags={flags} without {absent}"
            r64, e32, _ = H.camera_rays_refs(inp["M"], inp["pix"], inp["depth"], flags, grads)
            gM, gd = _camera_bwd(dev, inp, inp["depth"], flags, R, grads)
            H.assert_sum_bar("gM", gM.t, r64["gM"], r64["condM"], ceil, e32["gM"], where, worst)
            assert bool((gM.t[3] == 0).all()), f"{where}: row 3 of gM"
            H.assert_max_bar("g_depth", gd.t, r64["g_depth"], e32["g_depth"], T_GRAD, where, worst)
            assert bool((gd.t[zero] == 0).all()), f"{where}: g_depth at d = 0"
        grads = {k: inp[k] for k in GRADS}
        where = f"camera_bwd R={R} flags={flags}"
        r64, e32, _ = H.camera_rays_refs(inp["M"], inp["pix"], inp["depth"], flags, grads)
        gM, gd = _camera_bwd(dev, inp, inp["depth"], flags, R, grads, want_depth=False)
        assert gd.untouched(), f"{where}: g_depth written though NULL"
        H.assert_sum_bar("gM", gM.t, r64["gM"], r64["condM"], ceil, e32["gM"], where + " g_depth NULL", worst)
        r64, e32, _ = H.camera_rays_refs(inp["M"], inp["pix"], None, flags, grads)
        gM, gd = _camera_bwd(dev, inp, None, flags, R, grads, want_depth=False)
        assert gd.untouched()
        H.assert_sum_bar("gM", gM.t, r64["gM"], r64["condM"], ceil, e32["gM"], where + " depth NULL", worst)
    _report("prologue_camera_bwd", worst)


# ---- the ray loss -------------------------------------------------------------------------------------
SCALARS = ("total", "l_rgb", "l_depth", "l2_mean")


def _loss_fwd(dev, inp, R, nd, l1, with_depth=True):
    out = {k: Guarded((1,), dev) for k in SCALARS + ("cnt",)}
    dp, dg = (inp["dp"].to(dev), inp["dg"].to(dev)) if with_depth else (None, None)
    mask = None if inp["mask"] is None else inp["mask"].to(dev)
    _hip.ray_loss(inp["rgb"].to(dev), inp["gt"].to(dev), R, dp, dg, mask, nd if with_depth else 0, l1, H.LOSS_W_RGB,
                  H.LOSS_W_DEPTH, [out[k].t for k in SCALARS], out["cnt"].t)
    torch.cuda.synchronize()
    _intact(f"loss R={R}", **out)
    return out


def _loss_bwd(dev, inp, R, nd, l1, go, cnt, want=("g_rgb", "g_dp", "g_dg"), with_depth=True):
    o = dict(g_rgb=Guarded((R, 3), dev), g_dp=Guarded((nd,), dev), g_dg=Guarded((nd,), dev))
    dp, dg = (inp["dp"].to(dev), inp["dg"].to(dev)) if with_depth else (None, None)
    mask = None if inp["mask"] is None else inp["mask"].to(dev)
    gos = [None if go.get(k) is None else torch.tensor([go[k]], device=dev) for k in SCALARS]
    _hip.ray_loss_bwd(inp["rgb"].to(dev), inp["gt"].to(dev), R, dp, dg, mask, nd if with_depth else 0, l1, H.LOSS_W_RGB,
                      H.LOSS_W_DEPTH, gos, cnt, *[o[k].t if k in want else None for k in ("g_rgb", "g_dp", "g_dg")])
    torch.cuda.synchronize()
    _intact(f"loss_bwd R={R}", **o)
    return o


def _check_loss_grads(o, r64, e32, inp, l1, want, where, worst):
    for k in ("g_rgb", "g_dp", "g_dg"):
        if k not in want:
            assert o[k].untouched(), f"{where}: {k} written though NULL"
            continue
        H.assert_max_bar("loss." + k, o[k].t, r64[k], e32.get(k, 0.0), T_VALUE, where, worst)
    if "g_rgb" in want and l1:
        assert bool((o["g_rgb"].t.cpu()[inp["rgb"] == inp["gt"]] == 0).all()), f"{where}: g_rgb where e == 0 under l1"
    for k in ("g_dp", "g_dg"):
        if k in want:
            g = o[k].t.cpu()
            if inp["mask"] is not None:
                assert bool((g[~inp["mask"]] == 0).all()), f"{where}: {k} of a masked ray"
            assert bool((g[inp["dp"] == inp["dg"]] == 0).all()), f"{where}: {k} where dp == dg"


@pytest.mark.parametrize("R,nd", H.LOSS_SHAPES)
def test_ray_loss_values_and_gradients(dev, R, nd):
    """Both losses under the four masks, with and without a depth term: the four scalars inside the
    derived ceiling of their sums, cnt exact, the gradients per element; each upstream scalar absent in
    turn and go_total alone; each gradient output absent in turn."""
    worst = {}
    go_sets = [dict(H.LOSS_GO)] + [{k: (None if k == a else v) for k, v in H.LOSS_GO.items()} for a in SCALARS] + \
        [dict(total=H.LOSS_GO["total"])]
    for l1 in (0, 1):
        for mk in H.LOSS_MASKS:
            inp = H.ray_loss_inputs(R, nd, mk)
            where = f"loss R={R} nd={nd} l1={l1} mask={mk}"
            assert bool((inp["rgb"] == inp["gt"]).any()) and bool((inp["dp"] == inp["dg"]).any())
            r64, _, _ = H.ray_loss_refs(inp, l1, H.LOSS_GO)
            out = _loss_fwd(dev, inp, R, nd, l1)
            bars = H.ray_loss_scalar_bars(r64, R, nd, l1)
            for k in SCALARS:
                H.assert_sum_bar("loss." + k, out[k].t, r64[k], torch.tensor(bars[k], dtype=torch.float64), 1.0, 0.0, where, worst)
            want_cnt = {"none": nd, "all": nd, "one": 1, "zero": 0}[mk]
            assert out["cnt"].t.item() == want_cnt == r64["cnt"], f"{where}: cnt"
            if mk == "zero":
                assert out["l_depth"].t.item() == 0.0, f"{where}: l_depth without a valid ray"
            for go in go_sets:
                r64, e32, _ = H.ray_loss_refs(inp, l1, go)
                o = _loss_bwd(dev, inp, R, nd, l1, go, out["cnt"].t)
                _check_loss_grads(o, r64, e32, inp, l1, ("g_rgb", "g_dp", "g_dg"), f"{where} go={sorted(go)}", worst)
            if mk == "all":
                r64, e32, _ = H.ray_loss_refs(inp, l1, H.LOSS_GO)
                for absent in ("g_rgb", "g_dp", "g_dg"):
                    want = tuple(k for k in ("g_rgb", "g_dp", "g_dg") if k != absent)
                    o = _loss_bwd(dev, inp, R, nd, l1, H.LOSS_GO, out["cnt"].t, want)
                    _check_loss_grads(o, r64, e32, inp, l1, want, f"{where} without {absent}", worst)
        # no depth term at all
        inp = H.ray_loss_inputs(R, nd, "none")
        where = f"loss R={R} l1={l1} no depth"
        r64, e32, _ = H.ray_loss_refs(inp, l1, H.LOSS_GO, with_depth=False)
        out = _loss_fwd(dev, inp, R, nd, l1, with_depth=False)
        bars = H.ray_loss_scalar_bars(r64, R, 0, l1)
        for k in SCALARS:
            H.assert_sum_bar("loss." + k, out[k].t, r64[k], torch.tensor(bars[k], dtype=torch.float64), 1.0, 0.0, where, worst)
        assert out["l_depth"].t.item() == 0.0 and out["cnt"].t.item() == 0.0
        o = _loss_bwd(dev, inp, R, nd, l1, H.LOSS_GO, out["cnt"].t, ("g_rgb",), with_depth=False)
        _check_loss_grads(o, r64, e32, inp, l1, ("g_rgb",), where, worst)
    _report("prologue_loss", worst)


# ---- Adam -----------------------------------------------------------------------------------------------
def _hyper(kind, wd):
    b = hyper_block(H.ADAM_HYPER["lr"], H.ADAM_HYPER["b1"], H.ADAM_HYPER["b2"], H.ADAM_HYPER["eps"], wd)
    f = H.f32r
    hyp = dict(H.ADAM_HYPER, eps=f(H.ADAM_HYPER["eps"]), wd=f(wd))      # eps and the weight decay are f32 slots
    if kind == "no_doubles":        # slot 15 != 1: lr, beta1, beta2 are the f32 slots; slot 6 stays the given 1 - beta2
        b[15] = 0.0
        hyp.update(lr=f(hyp["lr"]), b1=f(hyp["b1"]), b2=f(hyp["b2"]), om2=b[6].item())
    elif kind == "no_om2":          # slot 6 == 0: 1 - beta2 is formed on the device
        b[6] = 0.0
    return b, hyp


@pytest.mark.parametrize("n", H.ADAM_N)
def test_adam_at_every_vector_and_grid_edge(dev, n):
    """No float4 at all, each tail length, a block edge, the 512-block cap, a strided vector, strided
    plus tail; weight decay 0 and 0.01; the default hyper block and its two fallback paths.  Three
    steps: p, m, v against the fp64 update; bit-equal to torch's GPU Adam with the default block; the
    step count, the ticket word after every launch, and the other slots of the block."""
    p0, gs = H.adam_inputs(n)
    assert bool((gs[0] == 0).any()) or n <= 8
    worst = {}
    for wd in (0.0, 0.01):
        for kind in ("default", "no_doubles", "no_om2"):
            block, hyp = _hyper(kind, wd)
            where = f"adam n={n} wd={wd} {kind}"
            hyper = Guarded((16,), dev)
            hyper.t.copy_(block)
            bufs = dict(p=Guarded((n,), dev), m=Guarded((n,), dev), v=Guarded((n,), dev))
            bufs["p"].t.copy_(p0)
            bufs["m"].t.zero_()
            bufs["v"].t.zero_()
            tp = torch.nn.Parameter(p0.clone().to(dev))
            opt = None
            if kind == "default":
                opt = torch.optim.Adam([tp], lr=H.ADAM_HYPER["lr"], betas=(H.ADAM_HYPER["b1"], H.ADAM_HYPER["b2"]),
                                       eps=H.ADAM_HYPER["eps"], weight_decay=wd)
            for s, g in enumerate(gs):
                gd = g.to(dev)
                _hip.adam_step(bufs["p"].t, gd, bufs["m"].t, bufs["v"].t, hyper.t)
                torch.cuda.synchronize()
                hb = hyper.t.cpu()
                assert hb[7:8].view(torch.int32).item() == 0, f"{where}: ticket after launch {s + 1}"
                assert hb[0].item() == s + 1, f"{where}: step after launch {s + 1}"
                if opt is not None:
                    tp.grad = gd.clone()
                    opt.step()
            _intact(where, hyper=hyper, **bufs)
            hb = hyper.t.cpu().view(torch.int32)
            keep = [i for i in range(16) if i not in (0, 7)]
            assert torch.equal(hb[keep], block.view(torch.int32)[keep]), f"{where}: a hyper slot changed"
            r64, e32, _ = H.adam_refs(p0, gs, hyp)
            for name, ref, e in zip(("p", "m", "v"), r64, e32):
                got = bufs[name].t.cpu().double()
                assert bool(torch.isfinite(got).all()), f"{where}: {name} not finite"
                err, bar = (got - ref).abs().max().item(), H.adam_bar(ref, e)
                ratio = err / (e + 4 * H.U24 * ref.abs().max().item())
                prev = worst.get("adam." + name, (0.0, 0.0))
                worst["adam." + name] = (max(prev[0], ratio), max(prev[1], e))
                print(f"{where} {name}: |got-f64| {err:.3e}  E_f32 {e:.3e}  bar {bar:.3e}")
                assert err <= bar, f"{where}: {name}: |got - f64| = {err:.3e} > {bar:.3e}"
            if opt is not None:
                st = opt.state[tp]
                assert torch.equal(bufs["p"].t, tp.detach()), f"{where}: p differs from torch's GPU Adam"
                assert torch.equal(bufs["m"].t, st["exp_avg"]) and torch.equal(bufs["v"].t, st["exp_avg_sq"]), where
    _report("prologue_adam", worst)


# ---- the weight pack ------------------------------------------------------------------------------------
P_ = lambda t: None if t is None else t.data_ptr()      # noqa: E731


class _Desc:
    """One nerf_pack_desc with sentinel-filled guarded destinations and its references."""

    def __init__(self, dev, W, ld_dst, rows_t=0, ld_t=0, rows_s=0, images=False, chain=False, perm_k=0, with_t=True):
        self.W, self.rows, self.cols = W, W.shape[0], W.shape[1]
        self.ld_dst, self.rows_t, self.ld_t, self.perm_k = ld_dst, rows_t, ld_t, perm_k
        self.rows_s = max(rows_s, self.rows)
        self.src = W.to(dev)
        self.n_dst_rows = self.rows_s if images else self.rows
        self.dst = Guarded((self.n_dst_rows, ld_dst), dev)
        self.dst_t = Guarded((rows_t, ld_t), dev) if with_t else None
        img = lambda r, k: Guarded((3, k // 8, r, 8), dev, torch.int16, -1)      # noqa: E731
        self.s = img(self.rows_s, ld_dst) if images else None
        self.ts = img(rows_t, ld_t) if images and with_t else None
        self.cs = img(self.rows_s, ld_dst) if chain else None
        self.cts = img(rows_t, ld_t) if chain and with_t else None
        g = lambda b: None if b is None else b.t      # noqa: E731
        self.desc = _hip.PackDesc(self.src.data_ptr(), self.dst.t.data_ptr(), P_(g(self.dst_t)), self.rows, self.cols, ld_dst,
                                  rows_t, ld_t, P_(g(self.s)), P_(g(self.ts)), rows_s, P_(g(self.cs)), P_(g(self.cts)), perm_k)

    def padded(self):
        Wp = torch.zeros(self.rows_s, self.ld_dst)
        Wp[:self.rows, :self.cols] = self.W
        Wt = torch.zeros(self.rows_t, self.ld_t)
        if self.dst_t is not None:
            Wt[:self.cols, :self.rows] = self.W.t()
        return Wp, Wt

    def check(self, mode, where):
        for name in ("dst", "dst_t", "s", "ts", "cs", "cts"):
            b = getattr(self, name)
            assert b is None or b.intact(), f"{where}: wrote outside {name}"
        Wp, Wt = self.padded()
        dst = self.dst.t.cpu()
        assert torch.equal(dst[:self.rows].view(torch.int32), Wp[:self.rows].view(torch.int32)), f"{where}: dst"
        assert bool((dst[self.rows:] == H.SENT).all()), f"{where}: rows past `rows` of dst lost the sentinel"
        if self.dst_t is not None:
            dt = self.dst_t.t.cpu()
            assert torch.equal(dt[:, :self.rows].view(torch.int32), Wt[:, :self.rows].contiguous().view(torch.int32)), \
                f"{where}: dst_t"
            assert bool((dt[:, self.rows:] == H.SENT).all()), f"{where}: columns r >= rows of dst_t lost the sentinel"
        if mode == 1:
            for name, buf, mat in (("dst_s", self.s, Wp), ("dst_ts", self.ts, Wt)):
                if buf is not None:
                    assert torch.equal(buf.t.cpu(), H.image_ref(mat)), f"{where}: {name} (bf16x3)"
            return
        perm_s = H.chain_perm_index(self.ld_dst, self.perm_k)
        perm_t = H.chain_perm_index(self.ld_t, self.ld_t) if self.cts is not None else None
        for name, buf, mat, perm, compact in (("dst_s", self.s, Wp, None, False), ("dst_ts", self.ts, Wt, None, False),
                                              ("dst_cs", self.cs, Wp, perm_s, True), ("dst_cts", self.cts, Wt, perm_t, True)):
            if buf is None:
                continue
            ref, got = H.pair_image_ref(mat, perm, compact), H.pair_image_read(buf.t, compact)
            for k in ref:
                assert torch.equal(got[k], ref[k]), f"{where}: {name}.{k} (fp16 pair)"


def _field_descs(dev, mode):
    """The descriptors FieldRunner.pack sends at hidden 256 / 128 -- ten weights with all four images
    (mode 2; two in mode 1), ten biases as rows = 1 without dst_t, the 3-row and the 1-row head -- and a
    23rd, 40 x 50 into [64][64] destinations, in the same launch."""
    import model as mdl
    torch.manual_seed(3)
    net = mdl.OfficialStaticNerf(H.make_cfg(hidden=256, S=32))
    layers = net.hip_runner().layers
    descs = []
    for l in layers:
        W = (l.linear.weight.detach() * torch.logspace(-3, 2, l.linear.weight.shape[0]).unsqueeze(1)).contiguous()
        if l.name == "l2":
            W = H.pack_edge_rows(W)
        descs.append((l.name, _Desc(dev, W, l.kp, l.kp, l.out_p, l.out_p, images=True, chain=mode == 2,
                                    perm_k=l.k1 if l.name != "l0" else 0)))
    for l in layers:
        descs.append((l.name + ".bias", _Desc(dev, l.linear.bias.detach().view(1, -1).contiguous(), l.out_p, with_t=False)))
    descs.append(("wc", _Desc(dev, net.fc_rgb.weight.detach().contiguous(), 128, with_t=False)))
    descs.append(("wd", _Desc(dev, net.fc_density.weight.detach().contiguous(), 256, with_t=False)))
    assert len(descs) == 22      # what FieldRunner.pack sends; the 23rd is smaller than its destinations
    W = H.pack_edge_rows(torch.randn(40, 50, generator=torch.Generator().manual_seed(9)))
    descs.append(("padded", _Desc(dev, W, 64, 64, 64, 64, images=True, chain=mode == 2, perm_k=32)))
    assert len(descs) == 23 and sorted({d.ld_dst for _, d in descs[:10]}) == [64, 256, 320]
    return descs


def _pack(descs, mode):
    _hip.gemm_set_precision(mode)
    try:
        _hip.pack_weights([d.desc for _, d in descs])
        torch.cuda.synchronize()
    finally:
        _hip.gemm_set_precision(0)


@pytest.mark.parametrize("mode", [2, 1])
def test_pack_the_fields_descriptors_in_one_launch(dev, mode):
    descs = _field_descs(dev, mode)
    _pack(descs, mode)
    for name, d in descs:
        d.check(mode, f"pack mode {mode} {name}")


@pytest.mark.parametrize("perm_k", [0, 32, 64])
def test_pack_padded_descriptor_keeps_and_zeroes(dev, perm_k):
    """A 64-wide descriptor smaller than its destinations (40 x 50 into [64][64]): the padding the
    header says is kept still holds the sentinel, the images are zero there, and the first perm_k
    columns of dst_cs (every column of dst_cts) are in chain order; a zero row, a row maximum of
    exactly 2^-3, a subnormal row and a row maximum of 3e38."""
    W = H.pack_edge_rows(torch.randn(40, 50, generator=torch.Generator().manual_seed(perm_k)))
    for mode in (2, 1):
        d = _Desc(dev, W, 64, 64, 64, 64, images=True, chain=mode == 2, perm_k=perm_k)
        _pack([("d", d)], mode)
        d.check(mode, f"pack 40x50 mode {mode} perm_k={perm_k}")
        if mode == 2:
            e = H.pair_image_read(d.s.t)["e"]
            assert e[1].item() == 0 and e[2].item() == 17 and e[3].item() == 140 and e[4].item() == 14 - 127
            assert bool((e[40:] == 0).all())
