"""One config-3 style step with training.with_ssim on (GPU only): Trainer.compute_loss + backward against
orc.compute_loss_full with tcfg["with_ssim"] = True, both camera orders, in the default GEMM mode, and
the assertion that the step took the pair kernels (the SSIM entries of csrc/pair.hip), not the torch
expressions.  64 x 96 with pc_ratio 4: a 16 x 24 grid; tests/test_gpu_pair_ssim_fp64.py covers the
production grid against fp64.  Bars: every loss term 1e-4, pose / distortion / NeRF gradients 2e-3."""
import pytest
import torch

import model as mdl
from model.optim import HipAdam
from oracle import nerf_oracle as orc
from tests import test_gpu_full_step as base
from tests.helpers import camera_K, make_cfg, report_err, rigid_c2w

pytestmark = pytest.mark.gpu


def test_full_step_with_ssim_matches_oracle(dev):
    H, W, FX, R, S, D, n_cams = 64, 96, 80.0, 256, 32, 64, 2
    cfg = make_cfg(hidden=D, S=S)
    tcfg = dict(cfg["training"])
    tcfg.update(with_ssim=True, n_training_points=R, annealing_epochs=0, scheduling_start=0)
    cfg["training"] = tcfg
    rcfg = cfg["rendering"]
    assert tcfg["pc_ratio"] == 4 and tcfg["rgb_s_weight"][0] != 0.0
    imgs, depths = zip(*[base._scene(s, H, W) for s in range(n_cams)])
    c2w_gt = torch.stack([rigid_c2w(11, 0.2)] * n_cams)
    c2w_gt[1, :3, 3] = c2w_gt[0, :3, 3] + torch.tensor([0.05, 0.0, -0.1])
    K = camera_K(H, W, FX, FX)

    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    ref = orc.OracleNerf(hidden_dim=D, white_background=rcfg["white_background"], dist_alpha=rcfg["dist_alpha"],
                         occ_activation=cfg["model"]["occ_activation"])
    ref.load_state_dict(net.state_dict())
    g = torch.Generator().manual_seed(3)
    r0, t0 = 0.01 * torch.randn(n_cams, 3, generator=g), 0.02 * torch.randn(n_cams, 3, generator=g)
    scales0, shifts0 = torch.tensor([[0.9], [1.0]]), torch.tensor([[0.02], [-0.03]])

    renderer = mdl.Renderer(net, rcfg, device=dev)
    nn_model = mdl.get_model(renderer, cfg, device=dev)
    pose = mdl.LearnPose(n_cams, True, True, cfg, init_c2w=c2w_gt.clone()).to(dev)
    dist = mdl.Learn_Distortion(n_cams, True, True, cfg).to(dev)
    with torch.no_grad():
        pose.r.copy_(r0); pose.t.copy_(t0)
        dist.global_scales.copy_(scales0); dist.global_shifts.copy_(shifts0)
    tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), tcfg, device=dev,
                     optimizer_pose=torch.optim.Adam(pose.parameters(), lr=5e-4), pose_param_net=pose,
                     optimizer_distortion=torch.optim.Adam(dist.parameters(), lr=5e-4), distortion_net=dist)
    assert tr.loss.cfg["with_ssim"] is True
    routed = []
    inner = tr._reference_terms

    def spy(*a, **kw):
        out = inner(*a, **kw)
        routed.append(out)
        return out

    tr._reference_terms = spy

    gdraw = torch.Generator().manual_seed(5)
    keys = ("loss", "loss_rgb", "loss_depth", "loss_pc", "loss_rgb_s", "l2_mean")
    for step, (cam, refc) in enumerate(((0, 1), (1, 0))):
        data = base._data(cam, refc, imgs, depths, c2w_gt, K)
        ray_idx = torch.randperm(H * W, generator=gdraw)[:R]
        noise = torch.rand(1, R, S, generator=gdraw)
        o_pose = {"r": r0.clone().requires_grad_(True), "t": t0.clone().requires_grad_(True), "init_c2w": c2w_gt.clone()}
        o_dist = {"scales": scales0.clone().requires_grad_(True), "shifts": shifts0.clone().requires_grad_(True),
                  "fix_scaleN": True}
        ref.zero_grad()
        lo = orc.compute_loss_full(ref, o_pose, o_dist, data, tcfg, rcfg, epoch=0, scheduling_start=0, ray_idx=ray_idx,
                                   noise=noise)
        lo["loss"].backward()
        for m, o in tr._modules_and_optims():
            o.zero_grad()
        tr.inject = (ray_idx, noise)
        lh = tr.compute_loss(data, it=step, epoch=0, scheduling_start=0)
        lh["loss"].backward()
        assert len(routed) == step + 1 and "pair_losses" in routed[-1], "the step left the pair kernels"
        assert float(lo["loss_rgb_s"].detach()) > 0
        for k in keys:
            a, b = float(lh[k].detach()), float(lo[k].detach())
            print(f"step {step} {k}: HIP {a!r} oracle {b!r}")
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, f"step {step} {k}: HIP {a} oracle {b}"
        for nm, a, b in (("pose.r", pose.r.grad, o_pose["r"].grad), ("pose.t", pose.t.grad, o_pose["t"].grad),
                         ("dist.scales", dist.global_scales.grad, o_dist["scales"].grad),
                         ("dist.shifts", dist.global_shifts.grad, o_dist["shifts"].grad)):
            assert report_err("full_step_ssim", nm, base._rel(a, b)) < 2e-3, (nm, a, b)
        for (n1, p1), (n2, p2) in zip(net.named_parameters(), ref.named_parameters()):
            assert n1 == n2
            assert report_err("full_step_ssim", n1, base._nrel(p1.grad, p2.grad)) < 2e-3, (step, n1)
