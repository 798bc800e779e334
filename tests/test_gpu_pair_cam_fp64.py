"""nerf_pair_backward_cam (csrc/pair.hip: the image-pair backward with the camera-matrix gradient of a
learned focal) against fp64 (GPU only), called through the C ABI with sentinel-guarded outputs and, at the
end, through model.pair.pair_losses(camera_grad=True).

The reference is the staged one of tests/pair_cam_ref.py (checked on the CPU by
test_pair_cam_reference_cpu.py): K as a per-point leaf of the staged pair terms, with the kernel's own nn
and the fp64 decisions, whose distance to every threshold PairRef / PairSsimRef assert first.  Per entry of
gK16: |hip - f64| <= PAIR_T_G13 cond16 + 4 E_f32, the bar g13 has, and exactly 0 where cond16 is 0.  g_d1,
g_d2 and g13 must be the bits of nerf_pair_backward / nerf_pair_backward_ssim on the same forward (which
test_gpu_pair_fp64.py and test_gpu_pair_ssim_fp64.py hold to fp64), so they are compared to those."""
import pytest
import torch

from model import _hip
from model.pair import pair_losses
from tests import helpers as H
from tests import pair_cam_ref as C
from tests import pair_ssim_ref as S
from tests import test_gpu_pair_fp64 as plain
from tests import test_gpu_pair_ssim_fp64 as ssimmod
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu

OUT = ("g_d1", "g_d2", "g13")


def _backward_cam(dev, inp, fw, combo, detach, ssim, where=""):
    h, w, P = inp["h"], inp["w"], inp["h"] * inp["w"]
    nb = (P + 255) // 256
    up = fw["up"]
    go_pc, go_rgbs = (None if v is None else torch.tensor([v], device=dev) for v in H.PAIR_COMBOS[combo])
    G = dict(gxy=Guarded((12 * P,), dev), g13=Guarded((13,), dev), gK=Guarded((16,), dev), part=Guarded((29 * nb,), dev),
             g_d1=Guarded((P,), dev), g_d2=Guarded((P,), dev))
    _hip.pair_backward_cam(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], up["img1"], up["img2"],
                           int(detach), fw["G"]["work"].t, fw["G"]["nn"].t, fw["G"]["samp"].t if ssim else None,
                           fw["G"]["out3"].t, go_pc, go_rgbs, G["gxy"].t, G["g_d1"].t, G["g_d2"].t, G["g13"].t, G["gK"].t,
                           G["part"].t)
    torch.cuda.synchronize()
    plain._intact(G, f"{where} cam backward {combo}")
    plain._intact(fw["G"], f"{where} cam backward {combo} (forward buffers)")
    out = {k: G[k].t.cpu() for k in OUT + ("gK", "part")}
    assert not bool((out["gK"] == H.SENT).any()) and not bool((out["part"] == H.SENT).any()), f"{where}: not written"
    return out


def _full_check(dev, inp, where, test):
    """Every run of cam_runs: the existing entry's bits in g_d1, g_d2, g13, gK16 against fp64; the first run
    twice -> (ref, {run: grads})."""
    P = inp["h"] * inp["w"]
    with_img = inp["img1"] is not None
    ref = C.PairCamRef(inp, device=dev if P > 8192 else None)
    fws = {False: plain._forward(dev, inp, where)}
    if with_img:
        S.PairSsimRef(inp, need_invalid_grad=False, need_valid=False)       # the with_ssim conditions of this set
        fws[True] = ssimmod._forward(dev, inp, where)
    grads = {}
    for combo, detach, ssim in C.cam_runs(with_img):
        fw = fws[ssim]
        g = grads[combo, detach, ssim] = _backward_cam(dev, inp, fw, combo, detach, ssim, where)
        old = (ssimmod._backward(dev, inp, fw, combo, detach, where) if ssim
               else plain._backward(dev, inp, fw, combo, detach, where=where))
        plain._same_bits(g, old, OUT, f"{where} {combo} detach={detach} ssim={ssim} (existing entry)")
        ref.check_gK(g["gK"], fw["nn"], combo, detach, ssim, where)
    first = C.cam_runs(with_img)[0]
    plain._same_bits(grads[first], _backward_cam(dev, inp, fws[first[2]], *first, where), OUT + ("gK", "part"), where)
    if with_img:
        last = ("both", 0, True)
        plain._same_bits(grads[last], _backward_cam(dev, inp, fws[True], *last, where), OUT + ("gK", "part"), where)
    ref.report(test)
    return ref, grads


@pytest.mark.parametrize("cam", H.PAIR_CAMERAS)
@pytest.mark.parametrize("h,w", [(2, 2), (2, 128), (2, 129), (19, 27), (47, 155)])
def test_pair_cam_against_fp64(dev, h, w, cam):
    """2 x 2, one full 256-point block, one block plus two points, three blocks with a ragged tail, the
    V_KITTI grid (29 blocks); a diagonal camera, one with a principal point, one with skew."""
    ref, grads = _full_check(dev, H.pair_generic_inputs(h, w, cam), f"{h}x{w}-{cam}", f"pair_cam_{h}x{w}_{cam}")
    gK = grads["both", 0, False]["gK"].view(4, 4)
    assert gK[0, 0].item() != 0 and gK[1, 1].item() != 0
    assert bool((gK[3] == 0).all()), "inv(K) has no translation column: row 3 has no term"


@pytest.mark.parametrize("h,w", [(19, 27), (3, 85)])
def test_pair_cam_full_camera(dev, h, w):
    """Every entry of K[:3] non-zero: inv(K) has a translation column and all 16 entries of gK have terms."""
    ref, grads = _full_check(dev, H.pair_generic_inputs(h, w, "full"), f"{h}x{w}-full", f"pair_cam_{h}x{w}_full")
    assert bool((grads["both", 0, False]["gK"] != 0).all())


def test_pair_cam_large(dev):
    """2 x 8193 = 16386 points, no images: 65 blocks of 29 partials, the reduced fixed-point scale."""
    _full_check(dev, H.pair_large_inputs(), "2x8193", "pair_cam_2x8193")


def test_pair_cam_clamped_points(dev):
    """The first workgroup all clamped and valid: nothing for R, t, s1 and the depths from rgb_s, but the
    projection of (nl, nl, nl) depends on K, so the block's gK partials are not zero."""
    inp, clamped = H.pair_clamped_inputs()
    ref, grads = _full_check(dev, inp, "clamped", "pair_cam_clamped")
    assert bool(ref.dec["bad"][clamped].all()) and bool(ref.dec["valid"][clamped].any())
    g = grads["rgbs", 0, False]
    assert bool((g["g_d1"][clamped] == 0).all()) and bool((g["part"][:13] == 0).all())
    assert g["part"][13:29].abs().max().item() > 0


def test_pair_cam_no_valid_point(dev):
    ref, grads = _full_check(dev, H.pair_no_valid_inputs(), "no-valid", "pair_cam_no_valid")
    assert not bool(ref.dec["valid"].any())
    for detach in (0, 1):
        for ssim in (False, True):
            assert bool((grads["rgbs", detach, ssim]["gK"] == 0).all())


def test_pair_cam_many_to_one(dev):
    """Every X query chooses one Y point: P scattered terms arrive at one pc2."""
    inp, hot = H.pair_many_to_one_inputs(47, 155)
    _full_check(dev, inp, "many-47x155", "pair_cam_many_47x155")


def test_pair_cam_coincident_points(dev):
    """X_i == Y_i on a patch (distance 0: no chamfer gradient from those pairs), no images."""
    _full_check(dev, H.pair_coincident_inputs()[0], "coincident", "pair_cam_coincident")


def test_pair_cam_refusals(dev):
    """A NULL gK16, images that do not go together, w = 1: a negative code with a message, nothing launches."""
    inp = H.pair_generic_inputs(3, 5, "diag")
    up = plain._upload(inp, dev)
    P = 15
    G = dict(work=Guarded((_hip.pair_workspace(P)[1],), dev), nn=Guarded((2 * P,), dev, dtype=torch.int32, fill=-7),
             out3=Guarded((3,), dev), samp=Guarded((6 * P,), dev), gxy=Guarded((12 * P,), dev), g_d1=Guarded((P,), dev),
             g_d2=Guarded((P,), dev), g13=Guarded((13,), dev), gK=Guarded((16,), dev), part=Guarded((29,), dev))
    one = torch.ones(1, device=dev)

    def bwd(h, w, img1, img2, samp, gK):
        _hip.pair_backward_cam(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], img1, img2, 0,
                               G["work"].t, G["nn"].t, samp, G["out3"].t, one, one, G["gxy"].t, G["g_d1"].t, G["g_d2"].t,
                               G["g13"].t, gK, G["part"].t)

    with pytest.raises(RuntimeError, match="gK16"):
        bwd(3, 5, up["img1"], up["img2"], None, None)
    with pytest.raises(RuntimeError, match="needs img1 and img2"):
        bwd(3, 5, None, None, G["samp"].t, G["gK"].t)
    with pytest.raises(RuntimeError, match="go together"):
        bwd(3, 5, up["img1"], None, None, G["gK"].t)
    with pytest.raises(RuntimeError, match="resolution"):
        bwd(15, 1, up["img1"], up["img2"], None, G["gK"].t)
    torch.cuda.synchronize()
    for name, gd in G.items():
        assert gd.untouched(), name


# ---- at the wrapper ----------------------------------------------------------------------------------
def _wrapper_run(dev, inp, weights=(1.0, 0.7), k_grad=True, **kw):
    h, w = inp["h"], inp["w"]
    up = plain._upload(inp, dev)
    d1 = up["d1"].view(1, 1, h, w).clone().requires_grad_(True)
    d2 = up["d2"].view(1, 1, h, w).clone().requires_grad_(True)
    K = up["K"].view(1, 4, 4).clone().requires_grad_(k_grad)
    Rt = up["Rt"].view(1, 4, 4).clone().requires_grad_(True)
    s1 = up["s1"].clone().requires_grad_(True)
    l_pc, l_rgbs = pair_losses(d1, d2, K, Rt, s1, up["img1"][None], up["img2"][None], (h, w), inp["nl"], **kw)
    total = sum(wt * l for wt, l in zip(weights, (l_pc, l_rgbs)) if wt is not None)
    total.backward()
    return dict(l_pc=l_pc.detach().cpu(), l_rgbs=l_rgbs.detach().cpu(), d1=d1.grad.cpu(), d2=d2.grad.cpu(),
                Rt=Rt.grad.cpu(), s1=s1.grad.cpu(), K=None if K.grad is None else K.grad.cpu())


@pytest.mark.parametrize("with_ssim", (False, True))
def test_pair_losses_camera_grad(dev, with_ssim):
    """pair_losses(camera_grad=True) with a [1,4,4] K leaf: backward of each loss alone and of both against
    the staged reference, the gradient in K's shape; a K without requires_grad takes the existing path, bit
    for bit; without camera_grad a K that requires grad is still refused."""
    inp = H.pair_generic_inputs(19, 27, "full")
    ref = C.PairCamRef(inp)
    fw = (ssimmod if with_ssim else plain)._forward(dev, inp, "wrapper")
    kw = dict(with_ssim=with_ssim)
    runs = {}
    for combo, (go_pc, go_rgbs) in H.PAIR_COMBOS.items():
        r = runs[combo] = _wrapper_run(dev, inp, (go_pc, go_rgbs), camera_grad=True, **kw)
        assert tuple(r["K"].shape) == (1, 4, 4)
        ref.check_gK(r["K"], fw["nn"], combo, 0, with_ssim, "wrapper")
        fixed = _wrapper_run(dev, inp, (go_pc, go_rgbs), k_grad=False, camera_grad=True, **kw)
        today = _wrapper_run(dev, inp, (go_pc, go_rgbs), k_grad=False, **kw)
        assert fixed["K"] is None
        for k in ("l_pc", "l_rgbs", "d1", "d2", "Rt", "s1"):
            assert torch.equal(fixed[k], today[k]), f"{combo}: fixed K: {k}"
            assert torch.equal(r[k], today[k]), f"{combo}: learned K: {k}"
    again = _wrapper_run(dev, inp, H.PAIR_COMBOS["both"], camera_grad=True, **kw)
    assert torch.equal(again["K"], runs["both"]["K"])
    det = _wrapper_run(dev, inp, H.PAIR_COMBOS["both"], camera_grad=True, rgbs_detach_scale=True, **kw)
    ref.check_gK(det["K"], fw["nn"], "both", 1, with_ssim, "wrapper")
    with pytest.raises(ValueError, match="learned camera matrix"):
        _wrapper_run(dev, inp, **kw)
    ref.report(f"pair_cam_wrapper{'_ssim' if with_ssim else ''}")
