"""The with_ssim entries of csrc/pair.hip (nerf_pair_forward_ssim / nerf_pair_backward_ssim) against fp64
(GPU only), called through the C ABI with sentinel-guarded outputs and, at the end, through
model.pair.pair_losses(with_ssim=True).

The reference is the staged one of tests/pair_ssim_ref.py (checked on the CPU by
test_pair_ssim_reference_cpu.py): the oracle's rgb_s_loss_ref(..., with_ssim=True) on the (1, h, w, 3)
samples with the kernel's own nn and the fp64 decisions, whose distance to every threshold PairSsimRef
asserts first.  Bars are PairRef's: |hip - f64| <= T + 4 E_f32, E_f32 the error of the same reference run
in f32.  X, Y and nn must be the plain entry's bits (which test_gpu_pair_fp64.py holds to fp64), so they
are compared to those and not to fp64 again."""
import pytest
import torch

from model import _hip
from model.pair import pair_losses
from tests import helpers as H
from tests import pair_ssim_ref as S
from tests import test_gpu_pair_fp64 as plain
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu

COMBOS = (("both", 0), ("both", 1), ("rgbs", 0), ("rgbs", 1))


def _forward(dev, inp, where=""):
    h, w, P = inp["h"], inp["w"], inp["h"] * inp["w"]
    up = plain._upload(inp, dev)
    nc, nfl = _hip.pair_workspace(P)
    G = dict(work=Guarded((nfl,), dev), nn=Guarded((2 * P,), dev, dtype=torch.int32, fill=-7), out3=Guarded((3,), dev),
             samp=Guarded((6 * P,), dev))
    _hip.pair_forward_ssim(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], up["img1"], up["img2"],
                           G["work"].t, G["nn"].t, G["samp"].t, G["out3"].t)
    torch.cuda.synchronize()
    plain._intact(G, f"{where} ssim forward")
    work = G["work"].t.cpu()
    samp = G["samp"].t.cpu()
    assert not bool((samp == H.SENT).any()), f"{where}: samples not written"
    return dict(up=up, G=G, X=work[:3 * P].view(P, 3), Y=work[3 * P:6 * P].view(P, 3), nn=G["nn"].t.cpu().view(2, P),
                out3=G["out3"].t.cpu(), samp=samp)


def _backward(dev, inp, fw, combo, detach, where=""):
    h, w, P = inp["h"], inp["w"], inp["h"] * inp["w"]
    nb = (P + 255) // 256
    up = fw["up"]
    go_pc, go_rgbs = (None if v is None else torch.tensor([v], device=dev) for v in H.PAIR_COMBOS[combo])
    G = dict(gxy=Guarded((12 * P,), dev), g13=Guarded((13,), dev), part=Guarded((13 * nb,), dev), g_d1=Guarded((P,), dev),
             g_d2=Guarded((P,), dev))
    _hip.pair_backward_ssim(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], up["img1"], up["img2"],
                            int(detach), fw["G"]["work"].t, fw["G"]["nn"].t, fw["G"]["samp"].t, fw["G"]["out3"].t, go_pc,
                            go_rgbs, G["gxy"].t, G["g_d1"].t, G["g_d2"].t, G["g13"].t, G["part"].t)
    torch.cuda.synchronize()
    plain._intact(G, f"{where} ssim backward {combo}")
    plain._intact(fw["G"], f"{where} ssim backward {combo} (forward buffers)")
    return {k: G[k].t.cpu() for k in ("g_d1", "g_d2", "g13", "part")}


def _full_check(dev, inp, where, test, **kw):
    """Forward twice, the four backwards, one of them twice, the plain entry's X, Y, nn -> (ref, fw, grads)."""
    ref = S.PairSsimRef(inp, **kw)
    fw = _forward(dev, inp, where)
    plain._same_bits(fw, _forward(dev, inp, where), ("X", "Y", "nn", "out3", "samp"), where)
    plain._same_bits(fw, plain._forward(dev, inp, where), ("X", "Y", "nn"), f"{where} (plain entry)")
    ref.check_out3(fw["out3"], fw["nn"], where)
    grads = {}
    for combo, detach in COMBOS:
        g = grads[combo, detach] = _backward(dev, inp, fw, combo, detach, where)
        ref.check_grads(g, fw["nn"], combo, detach, where)
    plain._same_bits(grads["both", 0], _backward(dev, inp, fw, "both", 0, where), ("g_d1", "g_d2", "g13", "part"), where)
    ref.report(test)
    return ref, fw, grads


@pytest.mark.parametrize("cam", ("diag", "principal"))
@pytest.mark.parametrize("h,w", [(3, 85), (2, 128), (2, 129), (19, 27), (3, 300)])
def test_pair_ssim_against_fp64(dev, h, w, cam):
    """Row ends at flat neighbours inside a wavefront (3 x 85), exactly one workgroup (2 x 128), a workgroup
    edge inside a row (2 x 129, 3 x 300 twice), three workgroups of short rows (19 x 27)."""
    ref, fw, grads = _full_check(dev, S.ssim_inputs(h, w, cam), f"{h}x{w}-{cam}", f"pair_ssim_{h}x{w}_{cam}")
    g_d1 = grads["rgbs", 0]["g_d1"]
    assert int(((g_d1 != 0) & ~ref.dec["valid"]).sum()) > 0, "no invalid point received a gradient"


def test_pair_ssim_vkitti_grid(dev):
    """47 x 155, the cfg3 depth grid, with the skewed camera."""
    _full_check(dev, S.ssim_inputs(47, 155, "skew"), "47x155-skew", "pair_ssim_47x155_skew")


@pytest.mark.parametrize("h,w", [(2, 2), (3, 2), (2, 3)])
def test_pair_ssim_narrow_frames(dev, h, w):
    """w = 2: both neighbours of a column are the other column; w = 3: every window touches both borders.
    A near-identity pose keeps a point valid (asserted)."""
    ref, _, _ = _full_check(dev, S.narrow_inputs(h, w), f"narrow-{h}x{w}", f"pair_ssim_narrow_{h}x{w}",
                            need_invalid_grad=False)
    assert bool(ref.dec["valid"].any())


def test_pair_ssim_clamped_points(dev):
    """Clamped points beside valid ones: their samples enter the neighbours' windows, they get no
    geometry gradient, and the first workgroup (all clamped) adds nothing to dR, dt, ds1."""
    inp, clamped = H.pair_clamped_inputs()
    ref, fw, grads = _full_check(dev, inp, "clamped", "pair_ssim_clamped")
    assert bool(ref.dec["bad"][clamped].all())
    assert fw["out3"][2].item() == 3.0 * int(ref.dec["valid"].sum())
    for detach in (0, 1):
        g = grads["rgbs", detach]
        assert bool((g["g_d1"][clamped] == 0).all()) and bool((g["part"][:13] == 0).all())
        assert g["part"][13:26].abs().max().item() > 0


def test_pair_ssim_no_valid_point(dev):
    inp = H.pair_no_valid_inputs()
    ref, fw, grads = _full_check(dev, inp, "no-valid", "pair_ssim_no_valid", need_valid=False, need_invalid_grad=False)
    assert not bool(ref.dec["valid"].any())
    assert fw["out3"][1].item() == 0.0 and fw["out3"][2].item() == 0.0
    for detach in (0, 1):
        assert all(bool((grads["rgbs", detach][k] == 0).all()) for k in ("g_d1", "g_d2", "g13"))


def test_pair_ssim_constant_images(dev):
    """img1 = img2 = 0.5, every point valid: no window holds a padded sample and the map is 0, at the
    clamp's edge, everywhere.
    The map-distance condition is waived; so is the sign condition, because a point whose difference is
    within rounding of 0 has its bilinear cell inside the constant image, where the sample's derivative
    is exactly 0, so that sign reaches no output."""
    inp = S.constant_inputs()
    ref, fw, grads = _full_check(dev, inp, "constant", "pair_ssim_constant", need_map=False, need_sign=False,
                                 need_invalid_grad=False)
    assert bool(ref.dec["valid"].all())
    assert 0.0 <= fw["out3"][1].item() <= 1e-6
    for g in grads.values():
        assert all(bool(torch.isfinite(g[k]).all()) for k in ("g_d1", "g_d2", "g13"))


def test_pair_ssim_leaves_the_plain_path_alone(dev):
    """nerf_pair_forward / _backward return the same bits before and after the SSIM entries ran on the same
    inputs, and differ from them in rgb_s only."""
    inp = S.ssim_inputs(19, 27, "principal")
    before = plain._forward(dev, inp, "plain before")
    gb = plain._backward(dev, inp, before, "both", 0, where="plain before")
    fw = _forward(dev, inp, "ssim")
    _backward(dev, inp, fw, "both", 0, "ssim")
    after = plain._forward(dev, inp, "plain after")
    ga = plain._backward(dev, inp, after, "both", 0, where="plain after")
    plain._same_bits(before, after, ("X", "Y", "nn", "out3"), "plain path")
    plain._same_bits(gb, ga, ("g_d1", "g_d2", "g13"), "plain path")
    assert torch.equal(fw["out3"][0], before["out3"][0]) and torch.equal(fw["out3"][2], before["out3"][2])
    assert fw["out3"][1].item() != before["out3"][1].item()


def test_pair_ssim_refusals(dev):
    """No sample buffer, no images, w = 1: a negative code with a message, nothing launches."""
    inp = H.pair_generic_inputs(3, 5, "diag")
    up = plain._upload(inp, dev)
    P = 15
    G = dict(work=Guarded((_hip.pair_workspace(P)[1],), dev), nn=Guarded((2 * P,), dev, dtype=torch.int32, fill=-7),
             out3=Guarded((3,), dev), samp=Guarded((6 * P,), dev), gxy=Guarded((12 * P,), dev), g_d1=Guarded((P,), dev),
             g_d2=Guarded((P,), dev), g13=Guarded((13,), dev), part=Guarded((13,), dev))
    one = torch.ones(1, device=dev)

    def fwd(h, w, img1, img2, samp):
        _hip.pair_forward_ssim(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], img1, img2, G["work"].t,
                               G["nn"].t, samp, G["out3"].t)

    def bwd(h, w, img1, img2, samp):
        _hip.pair_backward_ssim(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], img1, img2, 0,
                                G["work"].t, G["nn"].t, samp, G["out3"].t, one, one, G["gxy"].t, G["g_d1"].t, G["g_d2"].t,
                                G["g13"].t, G["part"].t)

    for call in (fwd, bwd):
        with pytest.raises(RuntimeError, match="samples is NULL"):
            call(3, 5, up["img1"], up["img2"], None)
        with pytest.raises(RuntimeError, match="needs img1 and img2"):
            call(3, 5, None, None, G["samp"].t)
        with pytest.raises(RuntimeError, match="go together"):
            call(3, 5, up["img1"], None, G["samp"].t)
        with pytest.raises(RuntimeError, match="resolution"):
            call(15, 1, up["img1"], up["img2"], G["samp"].t)
    torch.cuda.synchronize()
    for name, gd in G.items():
        assert gd.untouched(), name


# ---- at the wrapper ----------------------------------------------------------------------------------
def _wrapper_run(dev, inp, d1_grad=True, with_img=True, **kw):
    h, w = inp["h"], inp["w"]
    up = plain._upload(inp, dev)
    d1 = up["d1"].view(1, 1, h, w).clone().requires_grad_(d1_grad)
    d2 = up["d2"].view(1, 1, h, w).clone().requires_grad_(True)
    Rt = up["Rt"].view(1, 4, 4).clone().requires_grad_(True)
    s1 = up["s1"].clone().requires_grad_(True)
    i1, i2 = (up["img1"][None], up["img2"][None]) if with_img else (None, None)
    l_pc, l_rgbs = pair_losses(d1, d2, up["K"].view(1, 4, 4), Rt, s1, i1, i2, (h, w), inp["nl"], **kw)
    (l_pc + 0.7 * l_rgbs).backward()                    # the weights of H.PAIR_COMBOS["both"]
    return dict(l_pc=l_pc.detach().cpu(), l_rgbs=l_rgbs.detach().cpu(), d1=None if d1.grad is None else d1.grad.cpu(),
                d2=d2.grad.cpu(), Rt=Rt.grad.cpu(), s1=s1.grad.cpu())


def test_pair_losses_with_ssim(dev):
    """pair_losses(with_ssim=True) against the staged reference; d1 without requires_grad; called twice;
    img1 None -> rgb_s 0; with_ssim=False is today's call bit for bit."""
    inp = S.ssim_inputs(19, 27, "principal")
    P = inp["h"] * inp["w"]
    ref = S.PairSsimRef(inp)
    fw = _forward(dev, inp, "wrapper")
    r = _wrapper_run(dev, inp, with_ssim=True)
    assert torch.equal(r["l_pc"], fw["out3"][0]) and torch.equal(r["l_rgbs"], fw["out3"][1])
    ref.check_out3(fw["out3"], fw["nn"], "wrapper")
    g13 = torch.cat([r["Rt"][0, :3, :3].reshape(9), r["Rt"][0, :3, 3], r["s1"].reshape(1)])
    ref.check_grads(dict(g_d1=r["d1"].reshape(P), g_d2=r["d2"].reshape(P), g13=g13), fw["nn"], "both", 0, "wrapper")
    again = _wrapper_run(dev, inp, with_ssim=True)
    for k in r:
        assert torch.equal(r[k], again[k]), f"second call: {k}"
    frozen = _wrapper_run(dev, inp, d1_grad=False, with_ssim=True)
    assert frozen["d1"] is None
    for k in ("l_pc", "l_rgbs", "d2", "Rt", "s1"):
        assert torch.equal(frozen[k], r[k]), f"d1 without grad: {k}"
    no_img = _wrapper_run(dev, inp, with_img=False, with_ssim=True)
    assert no_img["l_rgbs"].item() == 0.0 and torch.equal(no_img["l_pc"], r["l_pc"])
    off, today = _wrapper_run(dev, inp, with_ssim=False), _wrapper_run(dev, inp)
    for k in off:
        assert torch.equal(off[k], today[k]), f"with_ssim=False: {k}"
    assert off["l_rgbs"].item() != r["l_rgbs"].item()
    ref.report("pair_ssim_wrapper")
