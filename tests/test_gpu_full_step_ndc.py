"""The LLFF-style step (configs/LLFF/fern.yaml:6-8: sample_option ndc, dist_alpha, depth_range [0, 1]) on
the MI355X path, where the NDC warp is nerf_ndc_rays / nerf_ndc_rays_bwd (GPU only).

* The torch expressions are not taken: with model.rendering.get_ndc_rays_fxfy made to raise, a CUDA NDC
  render and a training step run, and equal a run without the patch bit for bit.
* A Trainer step against orc.compute_loss_full with the same ray draw (Trainer.inject): 48 x 72 image,
  R = 256, S = 32, D = 64, two cameras in both orders; pose learning, pose + distortion learning, and a
  learned focal (set up as tests/test_gpu_full_step_focal.py).  Bars of tests/test_gpu_full_step.py:
  every loss term 1e-4 relative (+1e-6), pose / distortion / focal gradients 1e-4 of the largest entry,
  NeRF gradients 2e-3 in the Frobenius norm.  Where the fp32 oracle itself lies further than such a bar
  from its own fp64 evaluation, that tensor is held to 1.5 x the oracle's distance + 1e-5 against the
  fp64 value instead (the rule of test_render_backward_as_accurate_as_reference); the test prints
  which tensors took that rule.
  The ReLU decisions are staged, as tests/test_gpu_pair_fp64.py stages its discrete choices, so that no
  discontinuous choice is compared across precisions: the oracle (fp32 and fp64) takes the field's own
  gates, read from the post-ReLU outputs the HIP forward saves, and _assert_decisions holds every gate
  that differs from fp64's to |pre-activation| <= tau, tau the fp32 oracle's own largest pre-activation
  error against fp64 on the same inputs -- a wrong gate anywhere else fails there.  Why: under NDC with
  dist_alpha the last sample of a ray has alpha = 1 and carries about half its weight, so 256 samples make
  up most of NeRF gradients that cancel to 1e-5, and ONE unit decided the other way moves them by
  1e-3 .. 1e-2.  With the first draw of this test the fp64 oracle has a pre-activation in (-1e-6, -1e-7]
  at the output of layers0.4 that the HIP step evaluates above zero: unstaged, six NeRF tensors were
  3.8e-3 .. 1.9e-3 from the oracle (the figures the fp64 oracle gives with its gates moved to -1e-6,
  tests/test_ndc_reference_cpu.py::test_first_step_draw_sits_on_a_relu_kink), and the fp32 oracle itself
  is 1.9e-3 .. 1.0e-2 from fp64 on 11 of 80 other draws.
  Measured on an MI355X, staged, all three variants: 7 to 11 of 4 456 448 decisions differ from fp64's, the
  furthest at |pre-activation| 1.7e-5 (tau 3.8e-5 .. 7.3e-5); every loss term within 2e-7 relative; pose /
  distortion / focal gradients within 3.0e-6 (bar 1e-4); every NeRF gradient within 2.9e-5 (bar 2e-3), the
  fp32 oracle within 1.9e-4 of fp64; no tensor took the fp64 rule.
* Trainer_pose under NDC: the pose gradient as the oracle's, no field parameter with a .grad.  (Measured:
  the fp32 oracle's pose gradients are 9.9e-3 (r) and 2.7e-2 (t) from fp64 here, so both take the fp64
  rule; HIP is 1.2e-2 and 1.1e-2 from fp64.)
* An NDC step captured in a hipGraph with enable_graph_rng() and replayed once equals the eager step.
* One NDC eval tile through render_dist.render_image equals the same rays of the whole frame."""
import copy

import pytest
import torch
from torch.nn import functional as F

import model as mdl
from model import _hip
from model.common import arange_pixels
from model.optim import HipAdam
from oracle import nerf_oracle as orc
from tests.helpers import camera_K, make_cfg, report_err, rigid_c2w, synthetic_rays

pytestmark = pytest.mark.gpu

NDC = {"sample_option": "ndc", "dist_alpha": True, "depth_range": [0.0, 1.0]}
H, W, FX, R, S, D, N_CAMS = 48, 72, 60.0, 256, 32, 64, 2
STEPS = ((0, 1), (1, 0))
VARIANTS = ("pose", "pose_dist", "focal")
LOSS_KEYS = ("loss", "loss_rgb", "loss_depth", "loss_pc", "loss_rgb_s", "l2_mean")


def _scene(seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    img = torch.stack([0.5 + 0.4 * torch.sin(7 * xx + 3 * yy + seed), 0.5 + 0.4 * torch.cos(6 * yy - 2 * xx),
                       0.3 + 0.5 * xx * yy], 0).unsqueeze(0)
    depth = 2.0 + 3.0 * xx + 0.2 * torch.rand(H, W, generator=g)
    depth[torch.rand(H, W, generator=g) < 0.05] = 0.0
    return img, depth.unsqueeze(0)


def _data(cam, ref, imgs, depths, c2w_gt, K):
    return {"img": imgs[cam], "img.depth": depths[cam], "img.depth_mask": depths[cam] > 0,
            "img.camera_mat": K, "img.scale_mat": torch.eye(4).unsqueeze(0), "img.pose_gt": c2w_gt[cam].unsqueeze(0),
            "img.idx": torch.tensor([cam]), "img.ref_imgs": imgs[ref], "img.ref_depths": depths[ref],
            "img.ref_idxs": torch.tensor([ref]), "img.ref_pose_gt": c2w_gt[ref].unsqueeze(0)}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _cfg(hidden=D, samples=S, rays=R):
    cfg = make_cfg(hidden=hidden, S=samples, **NDC)
    cfg["training"].update(n_training_points=rays, annealing_epochs=0, scheduling_start=0)
    return cfg


def _oracle_camera(coeffs):
    """training.py:266-273 on the LearnFocal coefficients (order 2, fx and fy)."""
    f = torch.stack([coeffs[0], coeffs[1]]) ** 2
    pad, one = torch.zeros(4, dtype=f.dtype), torch.ones(1, dtype=f.dtype)
    return torch.cat([f[0:1], pad, -f[1:2], pad, -one, pad, one]).view(1, 4, 4)


class _Given(torch.nn.Module):
    """A ReLU whose decision is given: x where the gate is open, 0 elsewhere."""

    def __init__(self, gate):
        super().__init__()
        self.gate = gate

    def forward(self, x):
        return x * self.gate.to(x.dtype)


class _Setup:
    """Both sides of one variant from the same parameters: the drop-in Trainer on the device and what
    orc.compute_loss_full needs on the CPU."""

    def __init__(self, dev, variant):
        self.variant = variant
        cfg = self.cfg = _cfg()
        self.tcfg, self.rcfg = cfg["training"], cfg["rendering"]
        self.imgs, self.depths = zip(*[_scene(s) for s in range(N_CAMS)])
        c2w = self.c2w_gt = torch.stack([rigid_c2w(11, 0.2)] * N_CAMS)
        c2w[1, :3, 3] = c2w[0, :3, 3] + torch.tensor([0.05, 0.0, -0.1])
        self.K = camera_K(H, W, FX, FX)
        torch.manual_seed(42)
        net = self.net = mdl.OfficialStaticNerf(cfg)
        self.ref = orc.OracleNerf(hidden_dim=D, white_background=self.rcfg["white_background"],
                                  dist_alpha=self.rcfg["dist_alpha"], occ_activation=cfg["model"]["occ_activation"])
        self.ref.load_state_dict(net.state_dict())
        g = torch.Generator().manual_seed(3)
        self.r0, self.t0 = 0.01 * torch.randn(N_CAMS, 3, generator=g), 0.02 * torch.randn(N_CAMS, 3, generator=g)
        self.scales0, self.shifts0 = torch.tensor([[0.9], [1.0]]), torch.tensor([[0.02], [-0.03]])
        learn_dist = variant != "pose"
        renderer = mdl.Renderer(net, self.rcfg, device=dev)
        nn_model = mdl.get_model(renderer, cfg, device=dev)
        pose = self.pose = mdl.LearnPose(N_CAMS, True, True, cfg, init_c2w=c2w.clone()).to(dev)
        dist = self.dist = mdl.Learn_Distortion(N_CAMS, learn_dist, learn_dist, cfg).to(dev)
        with torch.no_grad():
            pose.r.copy_(self.r0); pose.t.copy_(self.t0)
            dist.global_scales.copy_(self.scales0); dist.global_shifts.copy_(self.shifts0)
        kw = {}
        self.fparams, self.coeffs0 = [], []
        if learn_dist:
            kw["optimizer_distortion"] = torch.optim.Adam(dist.parameters(), lr=5e-4)
        if variant == "focal":
            k00, k11 = self.K[0, 0, 0].item(), self.K[0, 1, 1].item()
            focal = mdl.LearnFocal(True, False, order=2, init_focal=[k00, -k11]).to(dev)
            kw.update(optimizer_focal=torch.optim.Adam(focal.parameters(), lr=1e-3), focal_net=focal)
            self.fparams = [focal.fx, focal.fy]
            self.coeffs0 = [p.detach().cpu().clone() for p in self.fparams]
        self.tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), self.tcfg, device=dev,
                              optimizer_pose=torch.optim.Adam(pose.parameters(), lr=5e-4), pose_param_net=pose,
                              distortion_net=dist, **kw)

    def data(self, cam, refc):
        return _data(cam, refc, self.imgs, self.depths, self.c2w_gt, self.K)

    def oracle(self, data, ray_idx, noise, dtype, gates=None):
        """One compute_loss_full + backward at dtype -> (losses, {name: gradient}, NeRF gradients).  gates: nine
        bool [R S, width] tensors, the ReLU decisions to take instead of pre-activation > 0 (the values pass
        unchanged where a gate is open); the nine pre-activations are left in self.pre."""
        cast = lambda t: t.to(dtype) if (torch.is_tensor(t) and t.is_floating_point()) else t      # noqa: E731
        net = copy.deepcopy(self.ref).to(dtype)
        net.zero_grad()
        pre = self.pre = []
        if gates is not None:
            k = 0
            for seq in (net.layers0, net.layers1, net.rgb_layers):
                for i, m in enumerate(seq):
                    if isinstance(m, torch.nn.Linear):
                        m.register_forward_hook(lambda mod, inp, out: pre.append(out.detach()))
                    elif isinstance(m, torch.nn.ReLU):
                        seq[i] = _Given(gates[k])
                        k += 1
            assert k == 9
        learn_dist = self.variant != "pose"
        o_pose = {"r": cast(self.r0).clone().requires_grad_(True), "t": cast(self.t0).clone().requires_grad_(True),
                  "init_c2w": cast(self.c2w_gt).clone()}
        o_dist = {"scales": cast(self.scales0).clone().requires_grad_(learn_dist),
                  "shifts": cast(self.shifts0).clone().requires_grad_(learn_dist), "fix_scaleN": True}
        d = {k: cast(v) for k, v in data.items()}
        coeffs = [cast(c).clone().requires_grad_(True) for c in self.coeffs0]
        if coeffs:
            d["img.camera_mat"] = _oracle_camera(coeffs)
        lo = orc.compute_loss_full(net, o_pose, o_dist, d, self.tcfg, self.rcfg, epoch=0, scheduling_start=0,
                                   ray_idx=ray_idx, noise=cast(noise))
        lo["loss"].backward()
        small = {"pose.r": o_pose["r"].grad, "pose.t": o_pose["t"].grad}
        if learn_dist:
            small.update({"dist.scales": o_dist["scales"].grad, "dist.shifts": o_dist["shifts"].grad})
        for nm, c in zip(("focal.fx", "focal.fy"), coeffs):
            small[nm] = c.grad
        return ({k: lo[k].detach() for k in LOSS_KEYS}, small, {n: p.grad for n, p in net.named_parameters()})

    def hip(self, data, ray_idx, noise, step=0):
        """One compute_loss + backward of the Trainer -> the same three dicts, on the host."""
        tr = self.tr
        for m, o in tr._modules_and_optims():
            m.zero_grad()
        tr.inject = (ray_idx, noise)
        runner, kept = tr._field_runner(), {}
        real = runner.forward

        def forward(*a, **k):
            out = real(*a, **k)
            kept["st"] = out[4]
            return out

        runner.forward = forward
        try:
            lh = tr.compute_loss(data, it=step, epoch=0, scheduling_start=0)
        finally:
            del runner.forward
        # the field's own ReLU decisions: its saved post-ReLU outputs of l0..l7 and the colour layer, rows ray-major
        acts, n = kept["st"]["acts"], R * S
        self.gates = [(acts[i][:n, :(D // 2 if i == 9 else D)] > 0).cpu() for i in (0, 1, 2, 3, 4, 5, 6, 7, 9)]
        lh["loss"].backward()
        small = {"pose.r": self.pose.r.grad, "pose.t": self.pose.t.grad}
        if self.variant != "pose":
            small.update({"dist.scales": self.dist.global_scales.grad, "dist.shifts": self.dist.global_shifts.grad})
        for nm, p in zip(("focal.fx", "focal.fy"), self.fparams):
            small[nm] = p.grad
        c = lambda t: None if t is None else t.detach().cpu().clone()      # noqa: E731
        return ({k: c(lh[k]) for k in LOSS_KEYS}, {k: c(v) for k, v in small.items()},
                {n: c(p.grad) for n, p in self.net.named_parameters()})


def _draw(seed=5):
    g = torch.Generator().manual_seed(seed)
    for _ in STEPS:
        yield torch.randperm(H * W, generator=g)[:R], torch.rand(1, R, S, generator=g)


def _held(name, got, o32, o64, bar, metric, fallback):
    """got against the fp32 oracle at `bar`; if the fp32 oracle is itself further than `bar` from its
    fp64 run, got against the fp64 value at 1.5 x that distance + 1e-5."""
    own = metric(o32, o64)
    if own <= bar:
        err = metric(got, o32)
        print(f"{name}: vs fp32 oracle {err:.3e} (bar {bar:g}); the oracle's own fp32-fp64 distance {own:.3e}")
        assert err < bar, (name, err, bar)
    else:
        err = metric(got, o64)
        fallback.append(name)
        print(f"{name}: the fp32 oracle is {own:.3e} from fp64 (> {bar:g}): vs fp64 {err:.3e}, held to {1.5 * own + 1e-5:.3e}")
        assert err <= 1.5 * own + 1e-5, (name, err, own)
    return err


def _assert_decisions(gates, pre32, pre64, where):
    """The field's ReLU decisions against the fp64 oracle's pre-activations: they may differ only where fp64
    cannot tell an f32 evaluation which way to go, |pre-activation| <= tau, tau the largest distance of the fp32
    oracle's own pre-activations from the fp64 ones on these inputs (the reference's own error on the decision
    variable).  Everywhere else a wrong gate fails here."""
    assert len(pre32) == len(pre64) == len(gates) == 9
    tau = max(float((a.double() - b).abs().max()) for a, b in zip(pre32, pre64))
    assert 0 < tau < 1e-3, tau
    n_diff, far = 0, 0.0
    for k, (g, x) in enumerate(zip(gates, pre64)):
        assert g.shape == x.shape, (k, g.shape, x.shape)
        diff = g != (x > 0)
        n_diff += int(diff.sum())
        if bool(diff.any()):
            far = max(far, float(x[diff].abs().max()))
    print(f"{where}: {n_diff} of {sum(g.numel() for g in gates)} ReLU decisions differ from fp64's, the furthest at "
          f"|pre-activation| {far:.3e}; tau {tau:.3e}")
    assert far <= tau, f"{where}: a ReLU decision differs from fp64's at |pre-activation| {far:.3e} > {tau:.3e}"


@pytest.mark.parametrize("variant", VARIANTS)
def test_ndc_training_step_matches_oracle(dev, variant):
    s = _Setup(dev, variant)
    fallback = []
    tag = f"full_step_ndc_{variant}"
    for step, ((cam, refc), (ray_idx, noise)) in enumerate(zip(STEPS, _draw())):
        data = s.data(cam, refc)
        lh, gh, nh = s.hip(data, ray_idx, noise, step)
        l32, g32, n32 = s.oracle(data, ray_idx, noise, torch.float32, s.gates)
        pre32 = s.pre
        l64, g64, n64 = s.oracle(data, ray_idx, noise, torch.float64, s.gates)
        pre64 = s.pre
        _assert_decisions(s.gates, pre32, pre64, f"{variant} step {step}")
        assert float(l32["loss_depth"]) > 0 and float(l32["loss_rgb"]) > 0
        for k in LOSS_KEYS:
            a, b32, b64 = float(lh[k]), float(l32[k]), float(l64[k])
            own = abs(b32 - b64)
            if own <= 1e-4 * abs(b64) + 1e-6:
                print(f"step {step} {k}: HIP {a!r} oracle {b32!r} (fp64 {b64!r})")
                assert abs(a - b32) <= 1e-4 * abs(b32) + 1e-6, f"step {step} {k}: HIP {a} oracle {b32}"
            else:
                fallback.append(f"step {step} {k}")
                print(f"step {step} {k}: HIP {a!r}; the fp32 oracle {b32!r} is {own:.3e} from fp64 {b64!r}")
                assert abs(a - b64) <= 1.5 * own + 1e-5, f"step {step} {k}: HIP {a} fp64 oracle {b64}"
        assert set(gh) == set(g32)
        for nm in g32:
            if g32[nm] is None:      # no gradient reaches the parameter (the fixed last scale with camera 1)
                assert g64[nm] is None and (gh[nm] is None or not bool(gh[nm].any())), nm
                continue
            assert gh[nm] is not None and float(g64[nm].abs().max()) > 0, nm
            report_err(tag, nm, _held(f"step {step} {nm}", gh[nm], g32[nm], g64[nm], 1e-4, _rel, fallback))
        for nm in n32:
            report_err(tag, nm, _held(f"step {step} {nm}", nh[nm], n32[nm], n64[nm], 2e-3, _nrel, fallback))
    if variant == "pose":
        assert s.dist.global_scales.grad is None and s.dist.global_shifts.grad is None
    print(f"{variant}: tensors held to 1.5 x the fp32 oracle's own distance from fp64 + 1e-5: {fallback or 'none'}")


def _same(a, b, where):
    for da, db in zip(a, b):
        assert da.keys() == db.keys()
        for k in da:
            if da[k] is None or db[k] is None:
                assert da[k] is None and db[k] is None, f"{where}: {k}"
            else:
                assert torch.equal(da[k], db[k]), f"{where}: {k} differs"


def test_ndc_torch_expressions_not_taken(dev, monkeypatch):
    """get_ndc_rays_fxfy raises: a CUDA NDC render (training and eval mode) and a training step with pose
    and distortion learning still run, with the bits of a run without the patch."""
    from model import rendering

    def render():
        cfg = _cfg(hidden=64, samples=32)
        torch.manual_seed(0)
        net = mdl.OfficialStaticNerf(cfg).to(dev)
        rnd = mdl.Renderer(net, cfg["rendering"], device=dev)
        b = synthetic_rays(R=64, S=32, H=40, W=50, seed=1)
        args = [b[k].to(dev) for k in ("pixels", "depth", "K", "w2c", "scale")]
        w2c = args[3].requires_grad_(True)
        out = rnd.nope_nerf(*args, dense_depth=True)
        m = out["depth_mask"]
        (out["rgb"].square().sum() + (out["depth_pred"] - out["depth_gt"])[m].abs().sum()).backward()
        with torch.no_grad():
            ev = rnd.nope_nerf(*args, eval_=True)
        res = {k: out[k].detach().cpu() for k in ("rgb", "depth_pred", "depth_gt", "depth_mask")}
        res.update({f"eval {k}": ev[k].cpu() for k in ("rgb", "depth_pred", "depth_gt")})
        res["w2c.grad"] = w2c.grad.cpu()
        res["l0.grad"] = net.layers0[0].weight.grad.cpu()
        # a ray without a depth prior has d_src = 0, so depth_gt = 1 - 1 / 0 there, as in the reference
        assert all(bool(torch.isfinite(v[res["depth_mask"]] if k.endswith("depth_gt") else v).all())
                   for k, v in res.items())
        assert bool((res["w2c.grad"] != 0).any())
        return res

    def step():
        s = _Setup(dev, "pose_dist")
        ray_idx, noise = next(_draw())
        return s.hip(s.data(0, 1), ray_idx, noise)

    plain_render, plain_step = render(), step()

    def refuse(*a, **k):
        raise AssertionError("the torch NDC expressions ran on device tensors")
    monkeypatch.setattr(rendering, "get_ndc_rays_fxfy", refuse)
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = _hip.ndc_rays, _hip.ndc_rays_bwd
    monkeypatch.setattr(_hip, "ndc_rays", lambda *a: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a))[1])
    monkeypatch.setattr(_hip, "ndc_rays_bwd", lambda *a: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a))[1])
    _same([render()], [plain_render], "render")
    assert calls == {"fwd": 2, "bwd": 1}, calls
    _same(step(), plain_step, "step")
    assert calls == {"fwd": 3, "bwd": 2}, calls
    # the CPU path keeps the torch expressions
    cfg = _cfg(hidden=64, samples=32)
    rnd = mdl.Renderer(mdl.OfficialStaticNerf(cfg), cfg["rendering"])
    b = synthetic_rays(R=8, S=32, H=40, W=50, seed=1)
    with pytest.raises(AssertionError, match="torch NDC expressions"):
        rnd.nope_nerf(b["pixels"], b["depth"], b["K"], b["w2c"], b["scale"])


# ------------------------------------------------------------------ Trainer_pose
HP, WP, FXP, NPTS, CAM = 40, 50, 30.0, 96, 1


def test_trainer_pose_under_ndc_matches_oracle(dev, monkeypatch):
    """test_gpu_pose_refine.test_trainer_pose_step_matches_oracle's scene under the NDC config (D = 256,
    S = 32, gain 2 on the weight matrices): the loss elementwise at 1e-4, the pose gradient 2e-3 in the
    Frobenius norm (or the fp64 rule above), the field untouched and without gradients."""
    cfg = _cfg(hidden=256, samples=32)
    rcfg = cfg["rendering"]
    torch.manual_seed(3)
    net = mdl.OfficialStaticNerf(cfg)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 2:
                p.mul_(2.0)
    ref = orc.OracleNerf(hidden_dim=256, dist_alpha=True)
    ref.load_state_dict(net.state_dict())
    c2w = torch.stack([rigid_c2w(3, 0.2), rigid_c2w(3, 0.2)])
    c2w[1, :3, 3] += torch.tensor([0.05, 0.0, -0.1])
    K = camera_K(HP, WP, FXP, FXP)
    pix = arange_pixels((HP, WP), 1)[1]
    g = torch.Generator().manual_seed(3)
    depth = 1.0 + 7.0 * torch.rand(1, HP, WP, generator=g)
    img = torch.rand(1, 3, HP, WP, generator=g)
    data = {"img": img, "img.idx": torch.tensor([CAM]), "img.depth": depth, "img.camera_mat": K,
            "img.scale_mat": torch.eye(4).unsqueeze(0)}
    ray_idx = torch.randperm(HP * WP, generator=g)[:NPTS]
    r0, t0 = 0.01 * torch.randn(2, 3, generator=g), 0.02 * torch.randn(2, 3, generator=g)

    def oracle(dtype):
        c = lambda t: t.to(dtype)      # noqa: E731
        ro, to = c(r0).clone().requires_grad_(True), c(t0).clone().requires_grad_(True)
        world = torch.inverse(orc.learn_pose_forward(ro, to, c(c2w), CAM)).unsqueeze(0)
        d = c(depth).reshape(-1)[ray_idx].view(1, -1, 1)
        out = orc.render_nope_nerf(copy.deepcopy(ref).to(dtype), c(pix)[:, ray_idx], d, c(K), world,
                                   c(data["img.scale_mat"]), rcfg, eval_=True)
        lo = F.mse_loss(out["rgb"], c(img).view(1, 3, HP * WP).permute(0, 2, 1)[:, ray_idx])
        lo.backward()
        return lo.detach(), ro.grad, to.grad

    renderer = mdl.Renderer(net, rcfg, device=dev)
    nn_model = mdl.get_model(renderer, cfg, device=dev)
    pose = mdl.LearnPose(2, True, True, cfg, init_c2w=c2w.clone()).to(dev)
    with torch.no_grad():
        pose.r.copy_(r0)
        pose.t.copy_(t0)
    tr = mdl.Trainer_pose(nn_model, {"n_points": NPTS, "type": "nope_nerf"}, dev,
                          torch.optim.Adam(pose.parameters(), lr=1e-3), pose, None)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    calls = []
    bwd = _hip.ndc_rays_bwd
    monkeypatch.setattr(_hip, "ndc_rays_bwd", lambda *a: (calls.append(1), bwd(*a))[1])
    tr.inject = ray_idx
    loss = tr.train_step(data)["loss"]
    assert len(calls) == 1, "the pose step's backward did not run nerf_ndc_rays_bwd once"
    l32, r32, t32 = oracle(torch.float32)
    l64, r64, t64 = oracle(torch.float64)
    loss = loss.detach()
    print(f"loss: HIP {float(loss)!r} oracle {float(l32)!r} fp64 {float(l64)!r}")
    assert abs(float(loss) - float(l32)) <= 1e-4 * abs(float(l32)) + 1e-6
    fallback = []
    for name, a, b32, b64 in (("r", pose.r.grad, r32, r64), ("t", pose.t.grad, t32, t64)):
        assert float(b64[CAM].abs().max()) > 0
        _held(f"pose.{name}", a[CAM], b32[CAM], b64[CAM], 2e-3, _nrel, fallback)
        assert float(a[1 - CAM].abs().max()) == 0.0, name
    print(f"Trainer_pose: held to the fp64 rule: {fallback or 'none'}")
    for n, p in net.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
        assert p.grad is None, n


# ------------------------------------------------------------------ graph replay
def _graph_trainer(dev):
    from model.synthetic import vkitti_scene
    cfg = _cfg(hidden=64, samples=32, rays=256)
    t = cfg["training"]
    t["pc_weight"], t["rgb_s_weight"] = [0.0, 0.0], [0.0, 0.0]      # one view: the render path alone
    data, c2w = vkitti_scene(dev, 0, H, W, FX)
    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    renderer = mdl.Renderer(net, cfg["rendering"], device=dev)
    nn_model = mdl.get_model(renderer, cfg, device=dev)
    pose = mdl.LearnPose(1, True, True, cfg, init_c2w=c2w.unsqueeze(0).to(dev)).to(dev)
    opt_pose = torch.optim.Adam(pose.parameters(), lr=5e-4, capturable=True, fused=True)
    tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), t, device=dev, optimizer_pose=opt_pose,
                     pose_param_net=pose)
    tr.enable_graph_rng()
    return tr, net, pose, data


def _state(out, net, pose):
    res = {k: v.detach().cpu().clone() for k, v in out.items() if isinstance(v, torch.Tensor)}
    res.update({f"net.{n}": p.detach().cpu().clone() for n, p in net.named_parameters()})
    res.update({"pose.r": pose.r.detach().cpu().clone(), "pose.t": pose.t.detach().cpu().clone()})
    return res


def test_ndc_step_graph_replay_equals_eager(dev):
    """Three eager steps, then the fourth: eager on one trainer, captured and replayed once on an
    identically seeded one -- every loss term and every parameter bit for bit."""
    old = _hip.gemm_get_precision()
    _hip.gemm_set_precision(2)
    try:
        tr, net, pose, data = _graph_trainer(dev)
        step = lambda: tr.train_step(data, it=0, epoch=0, scheduling_start=0)      # noqa: E731
        for _ in range(3):
            step()
        eager = _state(step(), net, pose)
        assert tr.seed_counter.item() == 4

        tr, net, pose, data = _graph_trainer(dev)
        step = lambda: tr.train_step(data, it=0, epoch=0, scheduling_start=0)      # noqa: E731
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        graph.replay()
        torch.cuda.synchronize()
        assert tr.seed_counter.item() == 4
        replayed = _state(out, net, pose)
    finally:
        _hip.gemm_set_precision(old)
    assert bool((replayed["pose.r"] != 0).any()) and bool(torch.isfinite(replayed["loss"]))
    _same([replayed], [eager], "graph replay")


# ------------------------------------------------------------------ sharded render
def test_ndc_eval_tile_equals_whole_frame(dev, monkeypatch):
    """render_dist.render_image on one rank's ray tile of an NDC frame (the second of two tiles, no process
    group) against the same rays of the whole-frame render: bit-identical, without the torch expressions."""
    from model import rendering
    from model.render_dist import render_image, tile_bounds
    monkeypatch.setattr(rendering, "get_ndc_rays_fxfy", None)
    cfg = _cfg(hidden=256, samples=32)
    torch.manual_seed(1)
    rnd = mdl.Renderer(mdl.OfficialStaticNerf(cfg).to(dev), cfg["rendering"], device=dev)
    pix = arange_pixels((HP, WP), 1)[1].to(dev)
    K, sc = camera_K(HP, WP, FXP, FXP).to(dev), torch.eye(4, device=dev).unsqueeze(0)
    w2c = torch.inverse(rigid_c2w(2, 0.2)).unsqueeze(0).to(dev)
    g = torch.Generator().manual_seed(4)
    depth = (1.0 + 7.0 * torch.rand(1, HP, WP, generator=g)).to(dev)
    rgb, dep = render_image(rnd, pix, K, w2c, sc, depth_img=depth)
    assert rgb.shape == (HP * WP, 3) and bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(dep).all())
    start, end, _ = tile_bounds(HP * WP, 1, 2)
    rgb_t, dep_t = render_image(rnd, pix[:, start:end], K, w2c, sc, depth_img=depth.reshape(-1)[start:end])
    assert torch.equal(rgb_t, rgb[start:end]) and torch.equal(dep_t, dep[start:end])
