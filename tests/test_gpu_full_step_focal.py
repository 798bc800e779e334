"""The config-3 style step with a learned focal length (pose.learn_focal: LearnFocal and its optimizer) on
the MI355X path against orc.compute_loss_full (GPU only): the "small" shape of tests/test_gpu_full_step.py
(48 x 72, 256 rays x 32 samples, D = 64, two cameras in both orders, pose + distortion learning).  On the
oracle side img.camera_mat is the Trainer's torch expression of two leaf coefficients, so the focal
gradient is autograd's through the rays, both point clouds and the projection.

Bars: every loss term 1e-4 and the pose / distortion gradients 1e-4, as in that file.  The focal gradient
is a cancelling sum over rays and points whose fp32 noise nobody had measured, so its bar is 1e-4 plus
four times the fp32 oracle's own relative distance from the same oracle run in fp64 (computed here, on
the CPU).  Also asserted: the step took pair_losses (not the torch expressions), nerf_pair_backward_cam
ran once per backward, and one train_step moves the focal parameters."""
import copy

import pytest
import torch

import model as mdl
from model import _hip
from model.optim import HipAdam
from oracle import nerf_oracle as orc
from tests import test_gpu_full_step as base
from tests.helpers import camera_K, make_cfg, report_err, rigid_c2w

pytestmark = pytest.mark.gpu

H, W, FX, R, S, D, N_CAMS = 48, 72, 60.0, 256, 32, 64, 2
STEPS = ((0, 1), (1, 0))
# (id, with_ssim, fx_only, order)
VARIANTS = [("plain", False, False, 2), ("ssim", True, False, 2), ("fx_only_order1", False, True, 1)]


def oracle_camera(coeffs, fx_only, order):
    """training.py:266-273 on the LearnFocal coefficients (intrinsics.py:59-70)."""
    f = torch.stack([coeffs[0], coeffs[0] if fx_only else coeffs[1]])
    f = f ** 2 if order == 2 else f
    pad, one = torch.zeros(4, dtype=f.dtype), torch.ones(1, dtype=f.dtype)
    return torch.cat([f[0:1], pad, -f[1:2], pad, -one, pad, one]).view(1, 4, 4)


def oracle_step(ref, data, tcfg, rcfg, r0, t0, c2w_gt, scales0, shifts0, coeffs0, fx_only, order, ray_idx, noise, dtype):
    """One compute_loss_full + backward at dtype from the given parameters -> (loss dict, pose, distortion,
    coefficient leaves)."""
    cast = lambda t: t.to(dtype) if (torch.is_tensor(t) and t.is_floating_point()) else t      # noqa: E731
    net = copy.deepcopy(ref).to(dtype)
    net.zero_grad()
    o_pose = {"r": cast(r0).clone().requires_grad_(True), "t": cast(t0).clone().requires_grad_(True),
              "init_c2w": cast(c2w_gt).clone()}
    o_dist = {"scales": cast(scales0).clone().requires_grad_(True), "shifts": cast(shifts0).clone().requires_grad_(True),
              "fix_scaleN": True}
    coeffs = [cast(c).clone().requires_grad_(True) for c in coeffs0]
    d = {k: cast(v) for k, v in data.items()}
    d["img.camera_mat"] = oracle_camera(coeffs, fx_only, order)
    lo = orc.compute_loss_full(net, o_pose, o_dist, d, tcfg, rcfg, epoch=0, scheduling_start=0, ray_idx=ray_idx,
                               noise=cast(noise))
    lo["loss"].backward()
    return lo, o_pose, o_dist, coeffs, net


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_full_step_with_learned_focal_matches_oracle(dev, monkeypatch, variant):
    name, with_ssim, fx_only, order = variant
    cfg = make_cfg(hidden=D, S=S)
    tcfg = dict(cfg["training"])
    tcfg.update(with_ssim=with_ssim, n_training_points=R, annealing_epochs=0, scheduling_start=0)
    cfg["training"] = tcfg
    rcfg = cfg["rendering"]
    imgs, depths = zip(*[base._scene(s, H, W) for s in range(N_CAMS)])
    c2w_gt = torch.stack([rigid_c2w(11, 0.2)] * N_CAMS)
    c2w_gt[1, :3, 3] = c2w_gt[0, :3, 3] + torch.tensor([0.05, 0.0, -0.1])
    K = camera_K(H, W, FX, FX)

    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    ref = orc.OracleNerf(hidden_dim=D, white_background=rcfg["white_background"], dist_alpha=rcfg["dist_alpha"],
                         occ_activation=cfg["model"]["occ_activation"])
    ref.load_state_dict(net.state_dict())
    g = torch.Generator().manual_seed(3)
    r0, t0 = 0.01 * torch.randn(N_CAMS, 3, generator=g), 0.02 * torch.randn(N_CAMS, 3, generator=g)
    scales0, shifts0 = torch.tensor([[0.9], [1.0]]), torch.tensor([[0.02], [-0.03]])

    renderer = mdl.Renderer(net, rcfg, device=dev)
    nn_model = mdl.get_model(renderer, cfg, device=dev)
    pose = mdl.LearnPose(N_CAMS, True, True, cfg, init_c2w=c2w_gt.clone()).to(dev)
    dist = mdl.Learn_Distortion(N_CAMS, True, True, cfg).to(dev)
    k00, k11 = K[0, 0, 0].item(), K[0, 1, 1].item()
    focal = mdl.LearnFocal(True, fx_only, order=order, init_focal=k00 if fx_only else [k00, -k11]).to(dev)
    with torch.no_grad():
        pose.r.copy_(r0); pose.t.copy_(t0)
        dist.global_scales.copy_(scales0); dist.global_shifts.copy_(shifts0)
    tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), tcfg, device=dev,
                     optimizer_pose=torch.optim.Adam(pose.parameters(), lr=5e-4), pose_param_net=pose,
                     optimizer_distortion=torch.optim.Adam(dist.parameters(), lr=5e-4), distortion_net=dist,
                     optimizer_focal=torch.optim.Adam(focal.parameters(), lr=1e-3), focal_net=focal)
    fparams = [focal.fx] if fx_only else [focal.fx, focal.fy]
    coeffs0 = [p.detach().cpu().clone() for p in fparams]

    routed, cam_calls = [], []
    inner = tr._reference_terms

    def spy(*a, **kw):
        out = inner(*a, **kw)
        routed.append(out)
        return out

    tr._reference_terms = spy
    cam = _hip.pair_backward_cam
    monkeypatch.setattr(_hip, "pair_backward_cam", lambda *a: (cam_calls.append(1), cam(*a))[1])

    gdraw = torch.Generator().manual_seed(5)
    keys = ("loss", "loss_rgb", "loss_depth", "loss_pc", "loss_rgb_s", "l2_mean")
    tag = f"full_step_focal_{name}"
    for step, (cam_i, refc) in enumerate(STEPS):
        data = base._data(cam_i, refc, imgs, depths, c2w_gt, K)
        ray_idx = torch.randperm(H * W, generator=gdraw)[:R]
        noise = torch.rand(1, R, S, generator=gdraw)
        args = (ref, data, tcfg, rcfg, r0, t0, c2w_gt, scales0, shifts0, coeffs0, fx_only, order, ray_idx, noise)
        lo, o_pose, o_dist, c32, _ = oracle_step(*args, torch.float32)
        _, _, _, c64, _ = oracle_step(*args, torch.float64)
        for m, o in tr._modules_and_optims():
            o.zero_grad()
        tr.inject = (ray_idx, noise)
        lh = tr.compute_loss(data, it=step, epoch=0, scheduling_start=0)
        lh["loss"].backward()
        assert len(routed) == step + 1 and "pair_losses" in routed[-1], "the step left the pair kernels"
        assert len(cam_calls) == step + 1, f"nerf_pair_backward_cam ran {len(cam_calls)} times after {step + 1} backwards"
        assert float(lo["loss_rgb_s"].detach()) > 0 and float(lo["loss_pc"].detach()) > 0
        for k in keys:
            a, b = float(lh[k].detach()), float(lo[k].detach())
            print(f"step {step} {k}: HIP {a!r} oracle {b!r}")
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, f"step {step} {k}: HIP {a} oracle {b}"
        for nm, a, b in (("pose.r", pose.r.grad, o_pose["r"].grad), ("pose.t", pose.t.grad, o_pose["t"].grad),
                         ("dist.scales", dist.global_scales.grad, o_dist["scales"].grad),
                         ("dist.shifts", dist.global_shifts.grad, o_dist["shifts"].grad)):
            assert report_err(tag, nm, base._rel(a, b)) < 1e-4, (nm, a, b)
        for nm, p, o32, o64 in zip(("focal.fx", "focal.fy"), fparams, c32, c64):
            own = base._rel(o32.grad, o64.grad)              # the fp32 oracle against its fp64 run
            got = base._rel(p.grad, o32.grad)
            report_err(tag, f"{nm} oracle f32 vs f64", own)
            print(f"step {step} {nm}: HIP {p.grad.item()!r} oracle f32 {o32.grad.item()!r} f64 {o64.grad.item()!r}")
            assert o64.grad.abs().item() > 0
            assert report_err(tag, nm, got) <= 1e-4 + 4 * own, (step, nm, p.grad, o32.grad, o64.grad)
    # one whole training step: the focal optimizer moves its parameters
    before = [p.detach().clone() for p in fparams]
    tr.inject = None
    torch.manual_seed(9)
    tr.train_step(base._data(0, 1, imgs, depths, c2w_gt, K), it=2, epoch=0, scheduling_start=0)
    for p, b in zip(fparams, before):
        assert bool(torch.isfinite(p).all()) and bool((p.detach() != b).all()), "the focal parameters did not move"
    assert len(cam_calls) == len(STEPS) + 1
