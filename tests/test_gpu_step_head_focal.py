"""The Trainer with a learned focal length (LearnFocal + its Adam) under the step head (NERF_STEP_HEAD=1)
against the separate launches (NERF_STEP_HEAD=0), by the method of tests/test_gpu_step_head_train.py: three
training steps on the two-view 16 x 24 scene, R = 128, S = 16, D = 256, f16x3, pose + distortion + focal
learning with the image-pair terms on (a 4 x 6 pair grid, the cameras alternating), identical seeds --
every tensor of the loss dict and every parameter, focal included, bit for bit (GPU only).  The camera
matrix requires grad here, so its gradient comes from _StepHead.backward (or nerf_unproject_matrix_bwd)
on the ray side and from nerf_pair_backward_cam on the pair side."""
import pytest
import torch

from model import _hip
from tests import test_gpu_step_head_train as base

pytestmark = pytest.mark.gpu

HH, WW, R, S = base.HH, base.WW, base.R, base.S


def _build(dev):
    import model as mdl
    from model.optim import HipAdam
    from model.synthetic import make_cfg, vkitti_pair_scene
    cfg = make_cfg(hidden=256, S=S)
    t = cfg["training"]
    t["n_training_points"] = R
    datas, c2w = vkitti_pair_scene(dev, HH, WW, 14.0)
    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    nn_model = mdl.get_model(mdl.Renderer(net, cfg["rendering"], device=dev), cfg, device=dev)
    pose = mdl.LearnPose(2, True, True, cfg, init_c2w=c2w.clone().to(dev)).to(dev)
    dn = mdl.Learn_Distortion(2, True, True, cfg).to(dev)
    K = datas[0]["img.camera_mat"]
    focal = mdl.LearnFocal(True, False, order=2, init_focal=[K[0, 0, 0].item(), -K[0, 1, 1].item()]).to(dev)
    tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), t, device=dev,
                     pose_param_net=pose, optimizer_pose=torch.optim.Adam(pose.parameters(), lr=5e-3),
                     distortion_net=dn, optimizer_distortion=torch.optim.Adam(dn.parameters(), lr=5e-3),
                     focal_net=focal, optimizer_focal=torch.optim.Adam(focal.parameters(), lr=5e-3))
    return tr, datas


def _run(dev, knob, monkeypatch, steps=3):
    monkeypatch.setenv("NERF_STEP_HEAD", knob)
    tr, datas = _build(dev)
    torch.manual_seed(7)
    seen = []
    for i in range(steps):
        ld = tr.train_step(datas[i % 2], it=i, epoch=0, scheduling_start=0)
        seen.append({k: v.detach().cpu().clone() for k, v in ld.items() if isinstance(v, torch.Tensor)})
    mods = [tr.model, tr.pose_param_net, tr.distortion_net, tr.focal_net]
    params = [p.detach().cpu().clone() for m in mods for p in m.parameters()]
    torch.cuda.synchronize()
    return seen, params, tr


@pytest.fixture(autouse=True)
def _f16x3():
    old = _hip.gemm_get_precision()
    _hip.gemm_set_precision(2)
    yield
    _hip.gemm_set_precision(old)


def test_three_steps_with_a_learned_focal_bit_equal(dev, monkeypatch):
    calls = {"head": 0, "cam": 0}
    head, cam = _hip.step_head, _hip.pair_backward_cam
    monkeypatch.setattr(_hip, "step_head", lambda *a: (calls.__setitem__("head", calls["head"] + 1), head(*a))[1])
    monkeypatch.setattr(_hip, "pair_backward_cam", lambda *a: (calls.__setitem__("cam", calls["cam"] + 1), cam(*a))[1])
    fused = _run(dev, "1", monkeypatch)
    assert calls == {"head": 3, "cam": 3}, f"the step head or the camera backward did not run every step: {calls}"
    plain = _run(dev, "0", monkeypatch)
    assert calls == {"head": 3, "cam": 6}, f"NERF_STEP_HEAD=0 took the step head: {calls}"
    base._assert_same(fused, plain, "learned focal")
    tr = fused[2]
    f0 = [tr.focal_net.fx.detach().cpu(), tr.focal_net.fy.detach().cpu()]
    _, datas = _build(dev)
    K = datas[0]["img.camera_mat"]
    init = torch.tensor([K[0, 0, 0].item(), -K[0, 1, 1].item()]).sqrt()
    assert all(bool(torch.isfinite(f)) for f in f0) and f0[0].item() != init[0].item() and f0[1].item() != init[1].item()
    assert "focalx" in fused[0][0] and "focaly" in fused[0][0]
