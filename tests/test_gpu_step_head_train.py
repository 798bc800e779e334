"""The Trainer with the step head (NERF_STEP_HEAD=1, one nerf_step_head launch for the pose, the
inverse, the draw, the gathers, the camera rays and the weight pack) against the separate launches
(NERF_STEP_HEAD=0): three training steps on a 16 x 24 scene, R = 128, S = 16, D = 256, f16x3, identical
seeds -- every tensor of the loss dict and every parameter bit for bit (GPU only)."""
import pytest
import torch

from model import _hip

pytestmark = pytest.mark.gpu

HH, WW, R, S = 16, 24, 128, 16
KINDS = ("fixed", "learned_pose", "pose_distortion", "graph_rng")


def _build(dev, kind):
    import model as mdl
    from model.optim import HipAdam
    from model.synthetic import make_cfg, vkitti_scene
    cfg = make_cfg(hidden=256, S=S)
    t = cfg["training"]
    t["n_training_points"] = R
    t["pc_weight"] = [0.0, 0.0]            # the pair terms off: the render path alone
    t["rgb_s_weight"] = [0.0, 0.0]
    data, c2w = vkitti_scene(dev, 0, HH, WW, 14.0)
    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    renderer = mdl.Renderer(net, cfg["rendering"], device=dev)
    nn_model = mdl.get_model(renderer, cfg, device=dev)
    opt = HipAdam(nn_model.parameters(), lr=1e-3)
    kw = {}
    if kind == "graph_rng":                # the benchmark's wiring: a LearnPose that learns nothing
        kw["pose_param_net"] = mdl.LearnPose(1, False, False, cfg, init_c2w=c2w.unsqueeze(0).to(dev)).to(dev)
    elif kind != "fixed":                  # "fixed": no pose net, the data dict's pose handed in
        pose = mdl.LearnPose(2, True, True, cfg, init_c2w=torch.stack([c2w, c2w]).to(dev)).to(dev)
        kw.update(pose_param_net=pose, optimizer_pose=torch.optim.Adam(pose.parameters(), lr=5e-3))
        if kind == "pose_distortion":
            dn = mdl.Learn_Distortion(2, True, True, cfg).to(dev)
            kw.update(distortion_net=dn, optimizer_distortion=torch.optim.Adam(dn.parameters(), lr=5e-3))
    tr = mdl.Trainer(nn_model, opt, t, device=dev, **kw)
    if kind == "graph_rng":
        tr.enable_graph_rng()
    return tr, net, data


def _run(dev, kind, knob, monkeypatch, steps=3, inject=None):
    """`steps` training steps from a fresh, identically seeded trainer -> (list of every tensor the
    loss dicts held, the final parameters), all on the host."""
    monkeypatch.setenv("NERF_STEP_HEAD", knob)
    tr, net, data = _build(dev, kind)
    torch.manual_seed(7)
    seen = []
    for i in range(steps):
        if inject is not None:
            tr.inject = inject
        ld = tr.train_step(data, it=i, epoch=0, scheduling_start=0)
        seen.append({k: v.detach().cpu().clone() for k, v in ld.items() if isinstance(v, torch.Tensor)})
    mods = [tr.model, tr.pose_param_net, tr.distortion_net]
    params = [p.detach().cpu().clone() for m in mods if m is not None for p in m.parameters()]
    torch.cuda.synchronize()
    return seen, params, tr


def _assert_same(a, b, where):
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    (sa, pa, _), (sb, pb, _) = a, b
    assert len(sa) == len(sb)
    for i, (da, db) in enumerate(zip(sa, sb)):
        assert da.keys() == db.keys() and "loss" in da
        for k in da:
            assert torch.equal(bits(da[k]), bits(db[k])), f"{where}: step {i}: loss dict '{k}' differs"
    assert len(pa) == len(pb) and len(pa) > 20
    for j, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(bits(x), bits(y)), f"{where}: parameter {j} differs after {len(sa)} steps"


@pytest.fixture(autouse=True)
def _f16x3():
    old = _hip.gemm_get_precision()
    _hip.gemm_set_precision(2)
    yield
    _hip.gemm_set_precision(old)


@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_bit_equal(dev, kind, monkeypatch):
    calls = {"head": 0, "pack": 0}
    head, pack = _hip.step_head, _hip.pack_weights
    monkeypatch.setattr(_hip, "step_head", lambda *a: (calls.__setitem__("head", calls["head"] + 1), head(*a))[1])
    monkeypatch.setattr(_hip, "pack_weights", lambda *a: (calls.__setitem__("pack", calls["pack"] + 1), pack(*a))[1])
    fused = _run(dev, kind, "1", monkeypatch)
    assert calls == {"head": 3, "pack": 0}, f"{kind}: the step head did not replace the launches: {calls}"
    plain = _run(dev, kind, "0", monkeypatch)
    assert calls == {"head": 3, "pack": 3}, f"{kind}: NERF_STEP_HEAD=0 did not take the separate launches: {calls}"
    _assert_same(fused, plain, kind)
    if kind != "fixed" and kind != "graph_rng":     # the learned parameters moved at all
        tr = fused[2]
        assert bool((tr.pose_param_net.r.detach() != 0).any()) and bool((tr.pose_param_net.t.detach() != 0).any())
    if kind == "pose_distortion":
        dn = fused[2].distortion_net
        assert bool((dn.global_scales.detach()[0] != 1).any()) and bool((dn.global_shifts.detach()[0] != 0).any())
    if kind == "graph_rng":
        assert fused[2].seed_counter.item() == 3 and plain[2].seed_counter.item() == 3


def test_injected_draw_keeps_the_separate_launches(dev, monkeypatch):
    """Trainer.inject set: the fused path must not engage, and the results are those of knob 0."""
    from model import training

    def refuse(*a, **k):
        raise AssertionError("the step head ran with Trainer.inject set")
    monkeypatch.setattr(training, "step_head", refuse)
    gen = torch.Generator().manual_seed(5)
    inject = (torch.randperm(HH * WW, generator=gen)[:R], torch.rand(1, R, S, generator=gen))
    _assert_same(_run(dev, "learned_pose", "1", monkeypatch, inject=inject),
                 _run(dev, "learned_pose", "0", monkeypatch, inject=inject), "inject")


def test_the_mark_is_consumed_not_left_set(dev, monkeypatch):
    """After a fused step an eval forward packs again (Adam has moved the weights since)."""
    _, _, tr = _run(dev, "learned_pose", "1", monkeypatch, steps=1)
    runner = tr._field_runner()
    assert runner.prepacked is False
    calls = []
    pack = _hip.pack_weights
    monkeypatch.setattr(_hip, "pack_weights", lambda d: (calls.append(len(d)), pack(d))[1])
    _, _, data = _build(dev, "fixed")
    from model.common import inv
    pixels = tr._pixels(HH, WW, dev)
    with torch.no_grad():
        out = tr.model(pixels, torch.arange(HH * WW, device=dev), data["img.camera_mat"],
                       inv(tr.pose_param_net(0)).unsqueeze(0), data["img.scale_mat"], "nope_nerf", add_noise=False,
                       eval_mode=True, it=0, depth_img=data["img.depth"].unsqueeze(1), img_size=(HH, WW))
    assert len(calls) >= 1 and out["rgb"].shape == (1, HH * WW, 3) and bool(torch.isfinite(out["rgb"]).all())
    w = runner.m.layers0[0].weight.detach()
    assert torch.equal(runner.w["l0"][:w.shape[0], :w.shape[1]], w), "the eval forward ran on stale packed weights"
