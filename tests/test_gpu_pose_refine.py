"""Test-time pose refinement on a frozen field (GPU only): the frozen-field chain kernels
against the training chain kernels they are instantiated from (bit for bit), the native
ray-gradient backward against nerf_field_backward, Renderer.nope_nerf(field_grad=False) and
Trainer_pose against the oracle, and the size of the frozen path's saved state."""
import os

import pytest
import torch
from torch.nn import functional as F

import model as mdl
from model import _hip
from model.common import arange_pixels
from oracle import nerf_oracle as orc
from tests.helpers import assert_elementwise, camera_K, make_cfg, rigid_c2w, synthetic_rays
from tests.helpers import chain_bwd_args as _chain_bwd_args, chain_descs as _chain_descs, chain_kernel_state as _kernel_state

pytestmark = pytest.mark.gpu

R0, S0, NP = 12, 32, 384        # kernel level: three 128-row blocks
SENTINEL = -12345.5


@pytest.fixture
def h16(dev):
    old = _hip.gemm_get_precision()
    _hip.gemm_set_precision(2)
    yield
    _hip.gemm_set_precision(old)


def _nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------ kernel level
def test_chain_frozen_bit_identical_to_chain_train(dev, h16):
    """The same arithmetic without the saves: every ReLU word and raw4 equal nerf_mlp_chain_train's
    bit for bit, and the buffers the training chain wrote (out, cmax) stay untouched."""
    k = _kernel_state(dev)
    runner = k["runner"]
    guards = [t for t in k["outs"] + k["cmaxes"] if t is not None]
    for t in guards:                      # where out / cmax were: kept out of the frozen call
        t.fill_(SENTINEL)
    masks2 = k["new_masks"]()
    raw4_2 = torch.full((NP, 4), SENTINEL, device=dev)
    none = [None] * 10
    _hip.mlp_chain_frozen(k["enc_p"], k["enc_d"], k["rp"], k["rd"], NP, _chain_descs(runner, none, masks2, none),
                          *k["heads"], raw4_2)
    torch.cuda.synchronize()
    assert torch.equal(raw4_2, k["raw4"])
    for l, a, b in zip(runner.layers, masks2, k["masks"]):
        if a is not None:
            assert torch.equal(a, b), l.name
            assert bool((a != 0).any()), l.name
    for t in guards:
        assert bool((t == SENTINEL).all())
    # the host check: a descriptor with an output is refused before any launch
    with pytest.raises(RuntimeError, match="out and cmax"):
        _hip.mlp_chain_frozen(k["enc_p"], k["enc_d"], k["rp"], k["rd"], NP,
                              _chain_descs(runner, [guards[0]] + [None] * 9, masks2, none), *k["heads"], raw4_2)


def test_chain_bwd_rays_bit_identical_to_chain_bwd(dev, h16):
    """D_0, D_5, D_9 and their row maxima equal nerf_mlp_chain_bwd's from the same graw4 and
    ReLU words; nothing else is written."""
    k = _kernel_state(dev)
    g = torch.Generator().manual_seed(9)
    graw4 = torch.randn(NP, 4, generator=g).to(dev)
    e = lambda *s: torch.full(s, SENTINEL, device=dev, dtype=torch.float32)      # noqa: E731
    w = lambda i: 128 if i == 0 else 256                                          # noqa: E731
    dy = [e(NP, w(i)) for i in range(10)]
    cm = [e(NP // 128, w(i)) for i in range(10)]
    rm = [e(NP) for _ in range(10)]
    _hip.mlp_chain_bwd(_chain_bwd_args(k, graw4, dy, cm, rm, e(512)))
    keep = (0, 5, 9)
    dy2 = [e(NP, w(i)) if i in keep else None for i in range(10)]
    rm2 = [e(NP) if i in keep else None for i in range(10)]
    _hip.mlp_chain_bwd_rays(_chain_bwd_args(k, graw4, dy2, [None] * 10, rm2, None))
    torch.cuda.synchronize()
    for i in keep:
        print(f"D_{i}: {int((dy2[i] != dy[i]).sum())} of {dy[i].numel()} elements differ, max |diff| "
              f"{float((dy2[i] - dy[i]).abs().max()):.3e} at max |D| {float(dy[i].abs().max()):.3e}; row maxima: "
              f"{int((rm2[i] != rm[i]).sum())} differ")
    for i in keep:
        assert torch.isfinite(dy[i]).all() and bool((dy[i] != 0).any())
        assert torch.equal(dy2[i], dy[i]), f"D_{i}"
        assert torch.equal(rm2[i], rm[i]), f"rmax {i}"
    with pytest.raises(RuntimeError, match="D_1"):
        _hip.mlp_chain_bwd_rays(_chain_bwd_args(k, graw4, [dy[i] if i in (0, 1, 5, 9) else None for i in range(10)],
                                                [None] * 10, rm2, None))


def test_field_backward_rays_bit_identical_to_field_backward(dev, h16):
    """The ray gradients of nerf_field_backward (ray_grad = 1, bwd_chain = 1) from a
    nerf_mlp_chain_train state, and of nerf_field_backward_rays from its z / raw4 / ReLU-word
    subset: the same launches on the same operands."""
    torch.manual_seed(7)
    net = mdl.OfficialStaticNerf(make_cfg(hidden=256, S=S0)).to(dev)
    runner = net.hip_runner()
    g = torch.Generator().manual_seed(8)
    o = ((torch.rand(R0, 3, generator=g) - 0.5) * 4).to(dev)
    d = F.normalize(torch.rand(R0, 3, generator=g) - 0.5, dim=-1).to(dev)
    g_rgb, g_dist = torch.randn(R0, 3, generator=g).to(dev), torch.randn(R0, generator=g).to(dev)
    old = {n: os.environ.get(n) for n in ("NERF_HEADS_SIDE", "NERF_BWD_CHAIN", "NERF_CHAIN")}
    os.environ.update({"NERF_HEADS_SIDE": "1", "NERF_BWD_CHAIN": "1", "NERF_CHAIN": "1"})   # the native schedule at this size
    try:
        _, _, _, _, st = runner.forward(o, d, (-d).contiguous(), None, 0.01, 10.0, S0, 0, keep=True)
        assert st["Np"] == NP and runner.native_backward(NP)
        grads = {id(p): torch.empty_like(p) for p in runner.param_list()}
        want = runner._backward_native(st, g_rgb, g_dist, True, None, lambda p: grads[id(p)])
        sub = {n: st[n] for n in ("R", "S", "Np", "flags", "z", "raw4", "masks", "pts_o", "pts_d", "view")}
        sub["frozen"] = True
        got = runner.backward_rays(sub, g_rgb, g_dist)
        torch.cuda.synchronize()
    finally:
        for n, v in old.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
    for name, a, b in zip(("g_pts_o", "g_pts_d", "g_view"), got, want):
        assert torch.isfinite(b).all() and bool((b != 0).any()), name
        assert torch.equal(a, b), name


# ------------------------------------------------------------------ end to end
def _pair(D, S, seed=0, gain=1.0):
    cfg = make_cfg(hidden=D, S=S)
    torch.manual_seed(seed)
    net = mdl.OfficialStaticNerf(cfg)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.mul_(gain)
    ref = orc.OracleNerf(hidden_dim=D)
    ref.load_state_dict(net.state_dict())
    return cfg, net, ref


@pytest.mark.parametrize("D", [64, 256])
def test_frozen_render_matches_oracle_and_leaves_the_field_without_grads(dev, D):
    """Renderer.nope_nerf(eval_=True, add_noise=False, field_grad=False) with grad enabled: the
    render and the gradient at world_mat as the oracle's autograd; no field parameter gets a
    .grad (D = 256: the frozen chain; D = 64: the per-layer schedule without weight gradients)."""
    R, S = 96, 32
    cfg, net, ref = _pair(D, S)
    rnd = mdl.Renderer(net.to(dev), cfg["rendering"], device=dev)
    b = synthetic_rays(R=R, S=S, H=40, W=50, seed=1)
    w2c = b["w2c"].to(dev).requires_grad_(True)
    out = rnd.nope_nerf(b["pixels"].to(dev), b["depth"].to(dev), b["K"].to(dev), w2c, b["scale"].to(dev),
                        eval_=True, add_noise=False, field_grad=False)
    (out["rgb"].square().sum() + out["depth_pred"].sum()).backward()
    w2c_o = b["w2c"].clone().requires_grad_(True)
    o = orc.render_nope_nerf(ref, b["pixels"], b["depth"], b["K"], w2c_o, b["scale"], cfg["rendering"], eval_=True)
    (o["rgb"].square().sum() + o["depth_pred"].sum()).backward()
    assert_elementwise(out["rgb"], o["rgb"], what="rgb")
    assert_elementwise(out["depth_pred"], o["depth_pred"], what="depth_pred")
    err = _nrel(w2c.grad, w2c_o.grad)
    print(f"D={D}: world_mat gradient nrel {err:.3e}")
    assert err < 2e-3
    for n, p in net.named_parameters():
        assert p.grad is None, n


H, W, FX, NPTS, CAM = 40, 50, 30.0, 96, 1
# field / pose seed of the scene below and the gain on the field's weight matrices: the default
# initialisation renders a nearly flat image (std 0.01: a pose error of 0.02 costs an MSE of 7e-9,
# the size of f32 rendering noise), at gain 2 the image has std 0.056 and the oracle's 30-step
# refinement lowers its loss threefold (test_short_refinement_lowers_the_loss)
SEED, GAIN = 3, 2.0


def _scene(D=256, S=32, seed=SEED):
    """Two cameras looking at a seeded random field; the images are the field's own renders at the
    true poses (the oracle's, on the CPU), so a perturbed pose has something to refine against."""
    cfg, net, ref = _pair(D, S, seed, GAIN)
    c2w = torch.stack([rigid_c2w(seed, 0.2), rigid_c2w(seed, 0.2)])
    c2w[1, :3, 3] += torch.tensor([0.05, 0.0, -0.1])
    K = camera_K(H, W, FX, FX)
    pix = arange_pixels((H, W), 1)[1]
    g = torch.Generator().manual_seed(seed)
    depth = 1.0 + 7.0 * torch.rand(1, H, W, generator=g)
    with torch.no_grad():
        rgb = orc.render_nope_nerf(ref, pix, depth.view(1, -1, 1), K, torch.inverse(c2w[CAM]).unsqueeze(0),
                                   torch.eye(4).unsqueeze(0), cfg["rendering"], eval_=True)["rgb"]
    img = rgb[0].t().reshape(1, 3, H, W).contiguous()
    data = {"img": img, "img.idx": torch.tensor([CAM]), "img.depth": depth, "img.camera_mat": K,
            "img.scale_mat": torch.eye(4).unsqueeze(0)}
    ray_idx = torch.randperm(H * W, generator=g)[:NPTS]
    return cfg, net, ref, c2w, data, pix, ray_idx


def _oracle_loss(ref, cfg, r, t, c2w, data, pix, ray_idx):
    """learn_pose_forward -> render_nope_nerf(eval_=True) -> F.mse_loss."""
    world_mat = torch.inverse(orc.learn_pose_forward(r, t, c2w, CAM)).unsqueeze(0)
    depth = data["img.depth"].reshape(-1)[ray_idx].view(1, -1, 1)
    out = orc.render_nope_nerf(ref, pix[:, ray_idx], depth, data["img.camera_mat"], world_mat, data["img.scale_mat"],
                               cfg["rendering"], eval_=True)
    return F.mse_loss(out["rgb"], data["img"].view(1, 3, H * W).permute(0, 2, 1)[:, ray_idx])


def _trainer(dev, cfg, net, c2w, r0, t0, lr):
    renderer = mdl.Renderer(net, cfg["rendering"], device=dev)
    nn_model = mdl.get_model(renderer, cfg, device=dev)
    pose = mdl.LearnPose(2, True, True, cfg, init_c2w=c2w.clone()).to(dev)
    with torch.no_grad():
        pose.r.copy_(r0)
        pose.t.copy_(t0)
    opt = torch.optim.Adam(pose.parameters(), lr=lr)
    tr = mdl.Trainer_pose(nn_model, {"n_points": NPTS, "type": "nope_nerf"}, dev, opt, pose, None)
    return tr, pose


def test_trainer_pose_step_matches_oracle(dev):
    cfg, net, ref, c2w, data, pix, ray_idx = _scene()
    g = torch.Generator().manual_seed(5)
    r0, t0 = 0.01 * torch.randn(2, 3, generator=g), 0.02 * torch.randn(2, 3, generator=g)
    tr, pose = _trainer(dev, cfg, net, c2w, r0, t0, 1e-3)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    tr.inject = ray_idx
    loss = tr.train_step(data)["loss"]
    ro, to = r0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
    lo = _oracle_loss(ref, cfg, ro, to, c2w, data, pix, ray_idx)
    lo.backward()
    assert_elementwise(loss, lo, what="loss")
    for name, a, b in (("r", pose.r.grad, ro.grad), ("t", pose.t.grad, to.grad)):
        err = _nrel(a[CAM], b[CAM])
        print(f"pose.{name} gradient nrel {err:.3e}")
        assert err < 2e-3, name
        assert float(a[1 - CAM].abs().max()) == 0.0 and float(b[1 - CAM].abs().max()) == 0.0, name
    # only the pose moved: the field is bit for bit what it was, and took no gradient
    for n, p in net.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
        assert p.grad is None, n
    assert not net.training and pose.training
    assert not torch.equal(pose.r.detach().cpu(), r0) and not torch.equal(pose.t.detach().cpu(), t0)


def _refine_losses(step_fn, n=30):
    return [float(step_fn()) for _ in range(n)]


def test_short_refinement_lowers_the_loss(dev):
    """Camera CAM's translation off by 0.02, 30 Adam steps at lr 1e-3 on a fixed ray set: the
    loss at step 30 is below the loss at step 1.  With SEED = 3 the oracle, stepped the same way
    on the CPU (oracle_refine_losses below), goes from 2.41e-4 to 7.2e-5."""
    cfg, net, ref, c2w, data, pix, ray_idx = _scene()
    t0 = torch.zeros(2, 3)
    t0[CAM] = torch.tensor([0.02, 0.0, 0.0])
    tr, pose = _trainer(dev, cfg, net, c2w, torch.zeros(2, 3), t0, 1e-3)
    tr.inject = ray_idx
    losses = _refine_losses(lambda: tr.train_step(data)["loss"].detach())
    print(f"refinement loss: step 1 {losses[0]:.4e}, step 30 {losses[-1]:.4e}")
    assert losses[-1] < losses[0], losses


def oracle_refine_losses(seed=SEED, n=30):
    """The refinement of test_short_refinement_lowers_the_loss on the oracle alone (CPU)."""
    cfg, net, ref, c2w, data, pix, ray_idx = _scene(seed=seed)
    t0 = torch.zeros(2, 3)
    t0[CAM] = torch.tensor([0.02, 0.0, 0.0])
    r, t = torch.zeros(2, 3, requires_grad=True), t0.clone().requires_grad_(True)
    opt = torch.optim.Adam([r, t], lr=1e-3)

    def step():
        opt.zero_grad()
        lo = _oracle_loss(ref, cfg, r, t, c2w, data, pix, ray_idx)
        lo.backward()
        opt.step()
        return lo.detach()
    return _refine_losses(step, n)


def test_frozen_state_holds_no_activation(dev, h16):
    """The frozen path's saved state at D = 256: raw4, z, the ReLU words and the ray inputs --
    at most Np x 4 x (4 + 1 + 9 x 8) bytes plus the rays, which no [Np, 256] tensor fits in."""
    R, S = 96, 32
    torch.manual_seed(0)
    net = mdl.OfficialStaticNerf(make_cfg(hidden=256, S=S)).to(dev)
    runner = net.hip_runner()
    g = torch.Generator().manual_seed(2)
    o = (torch.rand(R, 3, generator=g) - 0.5).to(dev)
    d = F.normalize(torch.rand(R, 3, generator=g) - 0.5, dim=-1).to(dev)
    rgb, dist, alpha, z, st = runner.forward_rays(o, d, (-d).contiguous(), None, 0.01, 10.0, S, 0)
    assert st["frozen"] and torch.isfinite(rgb).all()
    Np = st["Np"]
    assert Np == R * S

    def tensors(v):
        if torch.is_tensor(v):
            yield v
        elif isinstance(v, dict):
            for x in v.values():
                yield from tensors(x)
        elif isinstance(v, (list, tuple)):
            for x in v:
                yield from tensors(x)
    ts = list(tensors(st))
    total = sum(t.numel() * t.element_size() for t in ts)
    assert total <= Np * 4 * (4 + 1 + 9 * 8) + 3 * R * 3 * 4, total
    assert not any(t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] >= 128 for t in ts)
    assert "acts" not in st and "cmaxes" not in st
    # the training state of the same render holds ten activations: far above the bound
    _, _, _, _, st_full = runner.forward(o, d, (-d).contiguous(), None, 0.01, 10.0, S, 0, keep=True)
    assert sum(t.numel() * t.element_size() for t in tensors(st_full)) > 10 * total
