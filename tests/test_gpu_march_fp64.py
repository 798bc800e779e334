"""The four per-ray kernels of csrc/march.hip against tests/march_ref.py and fp64 (GPU only).

Bars.  nerf_march_select: state, f_low, f_high bit-equal to the f32 rule (one subtraction or a plain
selection each); d_low / d_high within 4 ulp of the f64 value at their own magnitude.
nerf_march_rays: sample positions within 4 ulp of |cam| + d_far.  nerf_secant_step: d_pred within
4 ulp of d_high against the f64 formula on the kernel's own f32 bracket; the bracket's selections
bit-equal; f_mid = act(raw) - tau within 4 ulp of max(1, sigma) (two library functions of <= 1 ulp
each whose errors reach an occupancy in [0, 1) with factors <= 1, and two roundings).
nerf_phong_shade: the project's render bar (RENDER_RTOL / RENDER_ATOL) against f64."""
import math

import pytest
import torch

from model import _hip
from model.field import F_DIST_ALPHA, F_RELU
from tests import march_ref as MR
from tests.helpers import assert_elementwise

pytestmark = pytest.mark.gpu


def _within_ulps(got, ref64, ulps, at=None, what=""):
    ref64 = ref64.double()
    if ref64.numel() == 0:
        return
    err = (got.double().cpu() - ref64).abs()
    lim = ulps * MR.ulp32(ref64 if at is None else at)
    bad = err > lim
    print(f"{what}: max err / bar = {(err / lim).max().item():.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} beyond {ulps} ulp (worst {(err / lim).max().item():.2f} bars)"


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("R", [1, 65, 384])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 512, 513])
def test_march_select(dev, n, R, tau):
    occ, d_far, names = MR.select_case(n, R, tau)
    d0 = 0.0 if n % 2 == 0 else 0.125
    if tau == 0 and R >= 13 and n >= 5:
        assert len(names) == 13
    state, f_low, f_high, d_low, d_high = (t.cpu() for t in _hip.march_select(occ.to(dev), d_far.to(dev), d0, tau))
    r_state, r_fl, r_fh, _, _ = MR.select_ref(occ, d_far, d0, tau)
    assert torch.equal(state, r_state)
    assert torch.equal(f_low, r_fl) and torch.equal(f_high, r_fh)
    _, _, _, r_dl, r_dh = MR.select_ref(occ, d_far, d0, tau, d_dtype=torch.float64)
    _within_ulps(d_low, r_dl, 4, what="d_low")
    _within_ulps(d_high, r_dh, 4, what="d_high")
    if R >= 65:
        assert {int(s) for s in r_state} == {0, 1, 2}
        for wrong in ("neg_to_pos", "no_product", "no_first"):      # the rows tell the wrong rules apart
            if tau == 0 and n >= 5:
                assert not torch.equal(MR.select_ref(occ, d_far, d0, tau, _wrong=wrong)[0], state), wrong


def _march_ray_set():
    """(cam [R][3], ray [R][3], rad, kind): cam[0] is the sphere's camera for every ray."""
    sets = {}
    cam = torch.tensor([0.15, -0.1, 2.0])
    rays = torch.tensor([[0.0, 0.0, -1.0], [0.05, 0.02, -1.0], [1.0, 0.0, 0.0], [0.3, -0.2, 1.0]])
    sets["outside"] = (cam, rays / rays.norm(dim=-1, keepdim=True), 1.0)         # hit, hit, miss, behind
    sets["inside"] = (torch.tensor([0.2, 0.1, -0.3]), rays / rays.norm(dim=-1, keepdim=True), 1.0)
    sets["tangent_pos"] = (torch.tensor([1.0 - 2.0 ** -20, 0.0, 0.0]), torch.tensor([[0.0, 1.0, 0.0]]), 1.0)
    sets["tangent_neg"] = (torch.tensor([1.0 + 2.0 ** -20, 0.0, 0.0]), torch.tensor([[0.0, 1.0, 0.0]]), 1.0)
    return sets


@pytest.mark.parametrize("n,seg", [(512, 512), (512, 128), (6, 2)])
@pytest.mark.parametrize("kind", ["outside", "inside", "tangent_pos", "tangent_neg"])
def test_march_rays(dev, kind, n, seg):
    cam0, ray, rad = _march_ray_set()[kind]
    R = ray.shape[0]
    cam = cam0.expand(R, 3).contiguous()
    d0 = 0.0 if seg != 2 else 0.25
    ref_far, u = MR.sphere_far(cam0.double(), ray.double(), rad)
    assert (u != 0).all()
    if kind == "outside":
        assert (u > 0).tolist() == [True, True, False, True]      # the last: both roots behind the camera
        assert ref_far[1] > 0 and ref_far[3] == 0
    elif kind == "inside":
        assert (u > 0).all() and (ref_far > 0).all()
    else:                                            # decided on the f64 side, within f32 rounding of 0
        assert abs(u.item()) < 4e-6 and (u.item() > 0) == (kind == "tangent_pos")
    d_far, o_seg, d_seg = _hip.march_rays(cam.to(dev), ray.to(dev), rad, d0, n, seg)
    G = n // seg
    assert o_seg.shape == (R * G, 3) and d_seg.shape == (R * G, 3)
    _within_ulps(d_far, ref_far, 4, what="d_far")
    assert ((ref_far == 0) == (d_far.cpu() == 0)).all()
    scale = (cam.double().norm(dim=-1) + ref_far).view(R, 1, 1).expand(R, n, 3)
    ref = MR.proposal_points(cam.double(), ray.double(), ref_far, d0, n)
    got = MR.segment_points(o_seg.cpu().view(R, G, 3), d_seg.cpu().view(R, G, 3), seg, torch.float64)
    _within_ulps(got, ref, 4, at=scale, what="positions")
    # and as the render kernels form them, in f32 (one multiply, one add more)
    got32 = MR.segment_points(o_seg.cpu().view(R, G, 3), d_seg.cpu().view(R, G, 3), seg, torch.float32)
    _within_ulps(got32, ref, 4, at=scale, what="positions (f32 sampling)")
    # the restatement the CPU tests use is this kernel to rounding
    w_far, w_o, w_d = MR.march_rays_ref(cam, ray, rad, d0, n, seg)
    _within_ulps(o_seg.cpu().view(R, G, 3), w_o.double(), 1, at=scale[:, :G], what="o_seg vs restatement")
    _within_ulps(d_seg.cpu().view(R, G, 3), w_d.double(), 1, at=scale[:, :G], what="d_seg vs restatement")


def _secant_inputs(R, seed=0):
    g = torch.Generator().manual_seed(seed)
    f_low, f_high = -0.02 - 0.45 * torch.rand(R, generator=g), 0.02 + 0.45 * torch.rand(R, generator=g)
    d_low = 0.3 + 3 * torch.rand(R, generator=g)
    d_high = d_low + 0.004 + 0.02 * torch.rand(R, generator=g)
    state = torch.ones(R, dtype=torch.uint8)
    state[3::7] = 0
    state[5::11] = 2
    f_high[2] = f_low[2]                              # a flat bracket: d_pred is not finite
    state[2] = 1
    cam = torch.tensor([0.15, -0.1, 2.0]).expand(R, 3).contiguous()
    ray = torch.randn(R, 3, generator=g)
    ray = ray / ray.norm(dim=-1, keepdim=True)
    raw = 3.0 * torch.randn(R, 4, generator=g)
    raw[::5, 0] = raw[::5, 0].abs() + 25.0            # beyond softplus's threshold of 20
    return f_low, f_high, d_low, d_high, state, cam, ray, raw


@pytest.mark.parametrize("flags", [0, F_RELU, F_DIST_ALPHA, F_RELU | F_DIST_ALPHA])
@pytest.mark.parametrize("R", [1, 257, 600])
def test_secant_step(dev, R, flags):
    tau = 0.5
    f_low, f_high, d_low, d_high, state, cam, ray, raw = _secant_inputs(max(R, 3))
    f_low, f_high, d_low, d_high, state, cam, ray, raw = (t[:R].contiguous() for t in
                                                          (f_low, f_high, d_low, d_high, state, cam, ray, raw))
    G = lambda t: t.clone().to(dev)                                         # noqa: E731
    br = [G(f_low), G(f_high), G(d_low), G(d_high)]
    d_pred, p_mid, d_i = (torch.full(s, 7.0, device=dev) for s in ((R,), (R, 3), (R,)))
    st, cam_d, ray_d = G(state), G(cam), G(ray)
    _hip.secant_step(True, None, flags, tau, st, cam_d, ray_d, br, d_pred, p_mid, d_i)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(br, (f_low, f_high, d_low, d_high)))    # untouched
    dp = d_pred.cpu().clone()
    ref = MR.secant_pred(f_low.double(), f_high.double(), d_low.double(), d_high.double())
    fin = torch.isfinite(ref)
    if R >= 3:
        assert not fin[2] and not math.isfinite(dp[2].item())
    _within_ulps(dp[fin], ref[fin], 4, at=d_high.double()[fin], what="d_pred (first)")

    def check_outputs(dp):
        go = (state == 1) & torch.isfinite(dp)
        want_p = torch.where(go.unsqueeze(-1), cam + dp.unsqueeze(-1) * ray, cam)      # f32, multiply then add
        assert torch.equal(p_mid.cpu(), want_p)
        assert torch.isfinite(p_mid).all()
        want_d = torch.where(state == 1, dp, torch.where(state == 2, 0.0, math.inf))
        assert torch.equal(torch.nan_to_num(d_i.cpu(), nan=-1.0), torch.nan_to_num(want_d, nan=-1.0))

    check_outputs(dp)
    # a step on injected raw head outputs
    occ64 = MR.density_ref(raw[:, 0].double(), bool(flags & F_RELU), bool(flags & F_DIST_ALPHA))
    fm64 = occ64 - tau
    assert (fm64.abs() > 1e-5).all()                  # every side of the threshold is decided
    _hip.secant_step(False, G(raw), flags, tau, st, cam_d, ray_d, br, d_pred, p_mid, d_i)
    low = (fm64 < 0) & fin
    high = ~(fm64 < 0) & fin
    n_fl, n_fh, n_dl, n_dh = (t.cpu() for t in br)
    assert torch.equal(n_dl, torch.where(low, dp, d_low)) and torch.equal(n_dh, torch.where(high, dp, d_high))
    assert torch.equal(n_fl[~low], f_low[~low]) and torch.equal(n_fh[~high], f_high[~high])
    at = occ64.abs().clamp_min(1.0)
    _within_ulps(n_fl[low], fm64[low], 4, at=at[low], what="f_mid (low)")
    _within_ulps(n_fh[high], fm64[high], 4, at=at[high], what="f_mid (high)")
    assert low.any() or R == 1
    dp2 = d_pred.cpu()
    ref2 = MR.secant_pred(n_fl.double(), n_fh.double(), n_dl.double(), n_dh.double())
    _within_ulps(dp2[fin], ref2[fin], 4, at=n_dh.double()[fin], what="d_pred (step)")
    assert not torch.isfinite(dp2[~fin]).any()        # a non-finite d_pred stays
    check_outputs(dp2)


def test_secant_activation_values(dev):
    """softplus below and above its threshold, ReLU at both signs, with and without 1 - exp(-sigma): f_mid
    lands in f_low or f_high."""
    raw0 = torch.tensor([-30.0, -3.0, -0.4328, 0.0, 0.5, 3.0, 19.9, 20.1, 40.0])
    R = raw0.numel()
    raw = torch.zeros(R, 4)
    raw[:, 0] = raw0
    cam, ray = torch.zeros(R, 3), torch.ones(R, 3)
    for flags in (0, F_RELU, F_DIST_ALPHA, F_RELU | F_DIST_ALPHA):
        br = [torch.full((R,), v, device=dev) for v in (-0.25, 0.25, 1.0, 2.0)]
        d_pred, p_mid, d_i = (torch.empty(s, device=dev) for s in ((R,), (R, 3), (R,)))
        st = torch.ones(R, dtype=torch.uint8, device=dev)
        _hip.secant_step(True, None, flags, 0.25, st, cam.to(dev), ray.to(dev), br, d_pred, p_mid, d_i)
        _hip.secant_step(False, raw.to(dev), flags, 0.25, st, cam.to(dev), ray.to(dev), br, d_pred, p_mid, d_i)
        occ = MR.density_ref(raw0.double(), bool(flags & F_RELU), bool(flags & F_DIST_ALPHA))
        fm = occ - 0.25
        got = torch.where(fm < 0, br[0].cpu().double(), br[1].cpu().double())
        _within_ulps(got, fm, 4, at=occ.abs().clamp_min(1.0), what=f"f_mid flags={flags}")


@pytest.mark.parametrize("R", [1, 300])
def test_phong_shade(dev, R):
    g0 = torch.Generator().manual_seed(5)
    cam0 = torch.tensor([0.15, -0.1, 2.0])
    cam = cam0.expand(R, 3).contiguous()
    g = torch.randn(R, 3, generator=g0) * torch.logspace(-3, 3, R).view(R, 1)
    raw = 4.0 * torch.randn(R + 3, 4, generator=g0)             # raw4 has padding rows
    state = torch.ones(R, dtype=torch.uint8)
    d_i = 0.5 + torch.rand(R, generator=g0)
    if R > 1:
        g[0] = 7.0 * cam0                                       # normal = light: the clamp at 1
        g[1] = -3.0 * cam0                                      # facing away: diffuse 0
        g[2] = torch.tensor([-0.1, -0.15, 0.0]) * 1e-3          # orthogonal to the light: diffuse 0 up to rounding
        state[3::7], state[4::9] = 0, 2
        d_i[5], d_i[6] = math.inf, math.nan                     # a bracket whose secant failed: background
        d_i[state == 0], d_i[state == 2] = math.inf, 0.0
    rgb, surf = _hip.phong_shade(g.to(dev), raw.to(dev), state.to(dev), d_i.to(dev), cam.to(dev))
    on = (state == 1) & torch.isfinite(d_i)
    light = cam0.double() / cam0.double().norm()
    normal = g.double() / g.double().norm(dim=-1, keepdim=True)
    shade = (0.3 + 0.7 * (normal @ light).clamp_min(0)).clamp_max(1.0)
    want = torch.where(on.unsqueeze(-1), shade.unsqueeze(-1).expand(R, 3), torch.ones(R, 3, dtype=torch.float64))
    want_s = torch.where(on.unsqueeze(-1), torch.sigmoid(raw[:R, 1:4].double()), torch.zeros(R, 3, dtype=torch.float64))
    assert_elementwise(rgb, want, what="rgb")
    assert_elementwise(surf, want_s, what="rgb_surf")
    assert rgb.max().item() <= 1.0
    if R > 1:
        assert rgb[0, 0].item() > 1 - 1e-6 and abs(rgb[1, 0].item() - 0.3) < 1e-6 and abs(rgb[2, 0].item() - 0.3) < 1e-6
        assert (rgb.cpu()[~on] == 1).all() and (surf.cpu()[~on] == 0).all()


def test_march_entries_check_their_arguments(dev):
    cam = torch.zeros(4, 3, device=dev)
    with pytest.raises(ValueError, match="divide"):
        _hip.march_rays(cam, cam, 1.0, 0.0, 512, 100)
    with pytest.raises(ValueError, match="n >= 2"):
        _hip.march_select(torch.zeros(4, 1, device=dev), torch.zeros(4, device=dev), 0.0, 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.march_rays(torch.zeros(4, 3), torch.zeros(4, 3), 1.0, 0.0, 512, 128)
