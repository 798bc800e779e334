"""The depth-prior kernels on the GPU: nerf_sample_rays_valid / nerf_step_head_valid against the numpy attempt
rule and the separate entries (bit for bit), nerf_ray_loss_invariant(_bwd) against fp64 autograd, and the
Trainer drawing against a sparse device mask, eagerly and from a captured hipGraph (GPU only)."""
import numpy as np
import pytest
import torch

from model import _hip
from tests import helpers as H
from tests import helpers_depth_prior as D
from tests.helpers import Guarded

_SH = D.step_head_pieces()
INT_FILL, _compare, _dev, _inputs, _ray_args, _ray_bufs, _same = (_SH.INT_FILL, _SH.compare, _SH.dev, _SH.inputs,
                                                                  _SH.ray_args, _SH.ray_bufs, _SH.same)

pytestmark = pytest.mark.gpu

# (name, (H, W, R), seed, mask): the three attempt counts at (100, 4), the stripe mask at 1024 rays, the
# sampler's cap, and a mask without a valid pixel
SAMPLER = {
    "small_1": (D.SMALL, D.SMALL_SEEDS[1], D.small_mask), "small_2": (D.SMALL, D.SMALL_SEEDS[2], D.small_mask),
    "small_5": (D.SMALL, D.SMALL_SEEDS[5], D.small_mask), "stripe_1": (D.STRIPE, D.STRIPE_SEEDS[1], D.stripe_mask),
    "stripe_2": (D.STRIPE, D.STRIPE_SEEDS[2], D.stripe_mask),
    "cap": (D.CAP, D.CAP_SEED, lambda: np.ones(D.CAP[0] * D.CAP[1], dtype=np.uint8)),
    "none_valid": (D.SMALL, 9, lambda: np.zeros(D.SMALL[0] * D.SMALL[1], dtype=np.uint8)),
}


def _sample_bufs(dev, R):
    return dict(idx=Guarded((R,), dev, torch.int64, INT_FILL), pixels=Guarded((R, 2), dev), rgb=Guarded((R, 3), dev),
                status=Guarded((1,), dev, torch.int32, INT_FILL), attempts=Guarded((1,), dev, torch.int32, INT_FILL))


def _sample_valid(dev, shape, seed, img, valid, counter=None, attempts=True):
    Hh, W, R = shape
    g = _sample_bufs(dev, R)
    _hip.sample_rays_valid(Hh * W, R, seed, W, Hh, img, valid, g["idx"].t, g["pixels"].t, g["rgb"].t, g["status"].t,
                           g["attempts"].t if attempts else None, counter)
    torch.cuda.synchronize()
    for k, b in g.items():
        assert b.intact(), f"wrote outside {k}"
    return g


def _sample_plain(dev, shape, seed, img, counter=None):
    Hh, W, R = shape
    o = dict(idx=torch.empty(R, dtype=torch.int64, device=dev), pixels=torch.empty(R, 2, device=dev),
             rgb=torch.empty(R, 3, device=dev), status=torch.empty(1, dtype=torch.int32, device=dev))
    _hip.sample_rays(Hh * W, R, seed, W, Hh, img, o["idx"], o["pixels"], o["rgb"], o["status"], counter)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("case", list(SAMPLER))
def test_sampler_draws_until_a_pixel_is_valid(dev, case):
    shape, seed, mk = SAMPLER[case]
    Hh, W, R = shape
    n = Hh * W
    mask = mk()
    img = torch.rand(3, Hh, W, generator=torch.Generator().manual_seed(n + R)).to(dev)
    valid = torch.from_numpy(mask).to(dev)
    ref_idx, ref_rounds, ref_att = D.sample_rays_valid_ref(n, R, seed, mask)
    g = _sample_valid(dev, shape, seed, img, valid)
    print(f"{case}: attempts {g['attempts'].t.item()} (reference {ref_att}), rounds {g['status'].t.item()}")
    assert g["attempts"].t.item() == ref_att and g["status"].t.item() == ref_rounds, case
    assert torch.equal(g["idx"].t.cpu(), ref_idx), case
    if case == "none_valid":
        assert ref_att == 0
    else:
        assert ref_att >= 1 and bool(valid[g["idx"].t].any())
    # the gathers ran on the accepted attempt: torch's own, and nerf_sample_rays under that attempt's seed
    assert torch.equal(g["rgb"].t, img.view(3, n)[:, g["idx"].t].t()), case
    assert (g["pixels"].t.cpu() - H.pixels_ref(ref_idx, Hh, W)).abs().max().item() <= 2.0 ** -22
    o = _sample_plain(dev, shape, D.attempt_seed(seed, (ref_att or D.MAX_ATTEMPTS) - 1), img)
    for k in o:
        _same(g[k].t, o[k], f"{case}: {k}")
    # a device counter: one advance per launch whatever the attempts, each launch the reference's draw
    ctr = Guarded((1,), dev, torch.int64, 0)
    for c in range(3):
        gc = _sample_valid(dev, shape, seed, img, valid, counter=ctr.t)
        ri, rr, ra = D.sample_rays_valid_ref(n, R, seed, mask, counter=c)
        assert torch.equal(gc["idx"].t.cpu(), ri) and gc["status"].t.item() == rr and gc["attempts"].t.item() == ra
        assert ctr.t.item() == c + 1 and ctr.intact(), f"{case}: counter after launch {c}"
    # attempts is optional
    g2 = _sample_valid(dev, shape, seed, img, valid, attempts=False)
    assert torch.equal(g2["idx"].t, g["idx"].t) and g2["attempts"].untouched()


@pytest.mark.parametrize("case", ["small_2", "stripe_1", "cap"])
def test_sampler_without_a_mask_is_nerf_sample_rays(dev, case):
    shape, seed, _ = SAMPLER[case]
    Hh, W, R = shape
    img = torch.rand(3, Hh, W, generator=torch.Generator().manual_seed(1)).to(dev)
    c0, c1, c2 = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(3))
    for counters in ((None, None, None), (c0, c1, c2)):
        for _ in range(2):
            o = _sample_plain(dev, shape, seed, img, counters[0])
            g = _sample_valid(dev, shape, seed, img, None, counter=counters[1])               # records attempts
            g2 = _sample_valid(dev, shape, seed, img, None, counter=counters[2], attempts=False)   # today's launch
            for k in o:
                _same(g[k].t, o[k], f"{case}: {k} (valid=None)")
                _same(g2[k].t, o[k], f"{case}: {k} (valid=None, no attempts)")
            assert g["attempts"].t.item() == 1 and g2["attempts"].untouched()
    assert c0.item() == c1.item() == c2.item() == 2


# ---- the step head ------------------------------------------------------------------------------------------
def _separate_valid(dev, d, shape, seed, flags, valid, counter=None, affine=None):
    """_separate of test_gpu_step_head.py with nerf_sample_rays_valid as the draw."""
    Hh, W, R = shape
    e = lambda *s: torch.empty(*s, device=dev)      # noqa: E731
    o = dict(c2w=e(4, 4), world=e(4, 4), M=e(4, 4), inverses=e(3, 4, 4), idx=torch.empty(R, dtype=torch.int64, device=dev),
             pixels=e(R, 2), rgb=e(R, 3), status=torch.empty(1, dtype=torch.int32, device=dev), cam=e(R, 3), ray=e(R, 3),
             view=e(R, 3), ray_norm=e(R), d_src=e(R), mask=torch.empty(R, dtype=torch.uint8, device=dev))
    att = torch.full((1,), INT_FILL, dtype=torch.int32, device=dev)
    _hip.pose_c2w(d["r"], d["t"], d["init"], o["c2w"])
    _hip.mat4_inv(o["c2w"], o["world"])
    _hip.unproject_matrix(d["K"], o["world"], d["scale"], o["M"], o["inverses"])
    _hip.sample_rays_valid(Hh * W, R, seed, W, Hh, d["img"], valid, o["idx"], o["pixels"], o["rgb"], o["status"], att,
                           counter)
    dep = o["depth_g"] = torch.index_select(d["depth"], 0, o["idx"])
    if affine is not None:
        dep = o["depth_d"] = e(R)
        _hip.depth_affine(o["depth_g"], d["aff_s"], d["aff_t"], affine, float("-inf"), dep)
    _hip.camera_rays(o["M"], o["pixels"], dep, R, flags, o["cam"], o["ray"], o["view"], o["ray_norm"], o["d_src"], o["mask"])
    torch.cuda.synchronize()
    return o, att


def _head_args(d, g, shape, seed, flags, counter, affine):
    Hh, W, R = shape
    a = _ray_args(d, g, Hh, W, R, flags, counter=counter, affine=affine)
    a.seed = seed
    return a


@pytest.mark.parametrize("case", list(SAMPLER))
def test_step_head_with_a_mask_equals_the_separate_entries(dev, case):
    shape, seed, mk = SAMPLER[case]
    Hh, W, R = shape
    mask = mk()
    valid = torch.from_numpy(mask).to(dev)
    flags, affine = 1, (None, False, True)[len(case) % 3]
    d = _dev(_inputs(Hh, W, R, seed=3), dev)
    where = f"step head valid {case}"
    o, att_sep = _separate_valid(dev, d, shape, seed, flags, valid, affine=affine)
    g = _ray_bufs(dev, R)
    att = Guarded((1,), dev, torch.int32, INT_FILL)
    _hip.step_head_valid(_head_args(d, g, shape, seed, flags, None, affine), valid, att.t)
    torch.cuda.synchronize()
    _compare(g, o, where, affine=affine)
    ref_idx, ref_rounds, ref_att = D.sample_rays_valid_ref(Hh * W, R, seed, mask)
    assert att.intact() and att.t.item() == att_sep.item() == ref_att, where
    assert torch.equal(g["idx"].t.cpu(), ref_idx) and g["status"].t.item() == ref_rounds, where
    # on a device counter, three launches
    c_sep = torch.zeros(1, dtype=torch.int64, device=dev)
    ctr = Guarded((1,), dev, torch.int64, 0)
    for c in range(3):
        o, att_sep = _separate_valid(dev, d, shape, seed, flags, valid, counter=c_sep, affine=affine)
        g = _ray_bufs(dev, R)
        _hip.step_head_valid(_head_args(d, g, shape, seed, flags, ctr.t, affine), valid, att.t)
        torch.cuda.synchronize()
        _compare(g, o, f"{where} counter {c}", affine=affine)
        assert att.t.item() == att_sep.item() == D.sample_rays_valid_ref(Hh * W, R, seed, mask, counter=c)[2]
        assert ctr.t.item() == c + 1 == c_sep.item() and ctr.intact()


@pytest.mark.parametrize("case", ["small_2", "stripe_1", "cap"])
def test_step_head_without_a_mask_is_nerf_step_head(dev, case):
    shape, seed, _ = SAMPLER[case]
    Hh, W, R = shape
    d = _dev(_inputs(Hh, W, R, seed=4), dev)
    g0, g1, g2 = _ray_bufs(dev, R), _ray_bufs(dev, R), _ray_bufs(dev, R)
    att = Guarded((1,), dev, torch.int32, INT_FILL)
    _hip.step_head(_head_args(d, g0, shape, seed, 3, None, True))
    _hip.step_head_valid(_head_args(d, g1, shape, seed, 3, None, True), None, None)      # nerf_step_head's kernel
    _hip.step_head_valid(_head_args(d, g2, shape, seed, 3, None, True), None, att.t)     # the loop, always accepted
    torch.cuda.synchronize()
    for k in g0:
        assert g1[k].intact() and g2[k].intact()
        _same(g1[k].buf, g0[k].buf, f"{case}: {k} (valid=None)")
        _same(g2[k].buf, g0[k].buf, f"{case}: {k} (valid=None, attempts recorded)")
    assert att.t.item() == 1 and att.intact()


# ---- the invariant depth loss -------------------------------------------------------------------------------
GO_ALL = {k: H.LOSS_GO[k] for k in ("total", "l_rgb", "l_depth", "l2_mean")}
SCALARS = ("total", "l_rgb", "l_depth", "l2_mean")


def _run_invariant(dev, inp, l1, go, want=("g_rgb", "g_dp", "g_dg")):
    R, n = inp["rgb"].shape[0], inp["dp"].shape[0]
    t = {k: (v.to(dev).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    out = {k: Guarded((1,), dev) for k in SCALARS}
    stats = Guarded((8,), dev)
    _hip.ray_loss_invariant(t["rgb"], t["gt"], R, t["dp"], t["dg"], t["mask"], n, int(l1), H.LOSS_W_RGB, H.LOSS_W_DEPTH,
                            [out[k].t for k in SCALARS], stats.t)
    gr = dict(g_rgb=Guarded((R, 3), dev), g_dp=Guarded((n,), dev), g_dg=Guarded((n,), dev))
    gos = [None if go.get(k) is None else torch.tensor(go[k], device=dev) for k in SCALARS]
    _hip.ray_loss_invariant_bwd(t["rgb"], t["gt"], R, t["dp"], t["dg"], t["mask"], n, int(l1), H.LOSS_W_RGB,
                                H.LOSS_W_DEPTH, gos, stats.t, *[gr[k].t if k in want else None for k in gr])
    torch.cuda.synchronize()
    for k, b in list(out.items()) + [("stats", stats)] + list(gr.items()):
        assert b.intact(), f"wrote outside {k}"
    for k in gr:
        assert k in want or gr[k].untouched(), f"{k} written though absent"
    return out, stats, gr


def _check_invariant(dev, inp, l1, go, where, want=("g_rgb", "g_dp", "g_dg"), worst=None):
    r64, e32, _ = D.invariant_refs(inp, l1, go)
    out, stats, gr = _run_invariant(dev, inp, l1, go, want)
    for k in SCALARS:
        got = out[k].t.cpu()
        if torch.isnan(r64[k]):
            assert bool(torch.isnan(got).all()), f"{where}: {k} = {got.item()} where fp64 gives NaN"
        else:
            H.assert_max_bar(k, got, r64[k].reshape(1), e32[k], H.T_VALUE, where, worst)
    for k in want:
        got, ref = gr[k].t.cpu(), r64[k]
        assert torch.equal(torch.isnan(got).reshape(ref.shape), torch.isnan(ref)), f"{where}: {k}: NaN pattern differs"
        fin = torch.isfinite(ref)
        assert bool(torch.isfinite(got.reshape(ref.shape)[fin]).all()), f"{where}: {k} not finite where fp64 is"
        H.assert_max_bar(k, got, ref, e32[k], H.T_GRAD, where, worst, finite=fin)
    # stats: the count, the medians bit-equal to torch.median of the masked f32 values, the tie counts
    st = stats.t.cpu()
    m = slice(None) if inp["mask"] is None else inp["mask"]
    p32, g32 = inp["dp"][m], inp["dg"][m]
    assert st[0].item() == p32.numel() == r64["cnt"] and st[7].item() == 0.0, where
    if p32.numel():
        for slot, v in ((1, p32), (3, g32)):
            assert torch.equal(st[slot].view(torch.int32), torch.median(v).view(torch.int32)), f"{where}: median {slot}"
        assert st[5].item() == r64["ties_p"] and st[6].item() == r64["ties_g"], where
        for slot, k in ((2, "s_p"), (4, "s_g")):
            assert abs(st[slot].item() - r64[k].item()) <= H.T_VALUE * abs(r64[k].item()), f"{where}: {k}"
    return r64


@pytest.mark.parametrize("mask_kind", D.INV_MASKS)
@pytest.mark.parametrize("n", D.INV_N)
def test_invariant_loss_against_fp64(dev, n, mask_kind):
    """Every per-thread slot edge of the 1024-thread workgroup (1023 .. 1025, 4096), the wave edges, the
    smallest counts; dp == dg on every third ray.  `third` at n <= 4 and `two` with n = 2 .. are the
    smallest counts: one entry (NaN, as fp64 gives) and two."""
    inp = D.invariant_inputs(n, mask_kind)
    _check_invariant(dev, inp, n % 2 == 0, GO_ALL, f"invariant n={n} mask={mask_kind}")


@pytest.mark.parametrize("n,mask_kind", [(65, "none"), (1024, "third"), (4096, "all")])
def test_invariant_loss_five_way_tie_at_the_median(dev, n, mask_kind):
    inp = D.invariant_inputs(n, mask_kind, ties=5)
    r64 = _check_invariant(dev, inp, True, GO_ALL, f"invariant ties n={n} mask={mask_kind}")
    assert r64["ties_p"] == 5 and r64["ties_g"] == 5


@pytest.mark.parametrize("absent", SCALARS + ("g_rgb", "g_dp", "g_dg"))
def test_invariant_loss_each_optional_argument_absent(dev, absent):
    inp = D.invariant_inputs(65, "third", ties=5)
    go = {k: (None if k == absent else v) for k, v in GO_ALL.items()}
    want = tuple(k for k in ("g_rgb", "g_dp", "g_dg") if k != absent)
    _check_invariant(dev, inp, False, go, f"invariant without {absent}", want=want)


def test_invariant_loss_without_a_path_to_the_depth_term(dev):
    """Neither go_total nor go_depth: the depth gradients are zeros (autograd's, even where l_depth is NaN)."""
    for inp in (D.invariant_inputs(65, "none"), D.invariant_inputs(3, "third")):
        _check_invariant(dev, inp, True, dict(l_rgb=0.7, l2_mean=0.3), "invariant rgb only")


def test_invariant_loss_nan_cases(dev):
    """cnt = 0, cnt = 1 and an all-equal input: the fp64 NaN pattern, g_rgb finite."""
    base = D.invariant_inputs(66, "none")
    zero, one = torch.zeros(66, dtype=torch.bool), torch.zeros(66, dtype=torch.bool)
    one[40] = True
    equal = dict(base, dp=torch.full((66,), 2.5))
    for name, inp in (("cnt0", dict(base, mask=zero)), ("cnt1", dict(base, mask=one)), ("equal", equal),
                      ("equal_masked", dict(equal, mask=D.invariant_inputs(66, "third")["mask"]))):
        r64 = _check_invariant(dev, inp, True, GO_ALL, f"invariant {name}")
        assert torch.isnan(r64["l_depth"]) and torch.isnan(r64["total"]) and bool(torch.isfinite(r64["g_rgb"]).all())


def test_invariant_loss_refuses_more_than_the_cap(dev):
    inp = D.invariant_inputs(4097, "none")
    with pytest.raises(RuntimeError, match="n_depth"):
        _run_invariant(dev, inp, True, GO_ALL)


@pytest.mark.parametrize("masked", [True, False])
def test_loss_forward_takes_the_fused_invariant_launch(dev, masked, monkeypatch):
    """Loss.forward with depth_loss_type 'invariant': the same dict as the torch expressions on the host, from
    one launch each way, gradients to the prediction and the prior."""
    from model import rays
    from model.losses import Loss
    from model.synthetic import make_cfg
    cfg = dict(make_cfg()["training"], depth_loss_type="invariant")
    lf = Loss(cfg)
    inp = D.invariant_inputs(1024, "third" if masked else "none", R=1024)
    w = {k: 0.0 for k in ("pc_weight", "rgb_s_weight", "depth_consistency_weight", "weight_dist_2nd_loss",
                          "weight_dist_1st_loss", "t_cycle_weight")}
    w.update(rgb_weight=1.0, depth_weight=0.04)
    calls = []
    fwd = _hip.ray_loss_invariant
    monkeypatch.setattr(_hip, "ray_loss_invariant", lambda *a: (calls.append(1), fwd(*a))[1])

    def run(device):
        leaf = lambda t: t.detach().clone().to(device).requires_grad_(True)      # noqa: E731
        rgb, dp, dg = leaf(inp["rgb"].unsqueeze(0)), leaf(inp["dp"]), leaf(inp["dg"])
        mask = None if inp["mask"] is None else inp["mask"].to(device)
        out = lf(rgb, inp["gt"].to(device).unsqueeze(0), dp, dg, weights=w, rgb_loss_type="l1", depth_mask=mask)
        out["loss"].backward()
        return out, rgb.grad, dp.grad, dg.grad
    ref = run("cpu")
    assert not calls
    got = run(dev)
    assert calls == [1]
    for k in ("loss", "loss_rgb", "loss_depth", "l2_mean"):
        a, b = got[0][k].item(), ref[0][k].item()
        assert abs(a - b) <= 1e-5 * abs(b), (k, a, b)
    for a, b in zip(got[1:], ref[1:]):
        assert (a.cpu() - b).abs().max().item() <= 1e-4 * b.abs().max().item()
    assert rays.can_fuse_invariant(inp["dp"]) and not rays.can_fuse_invariant(torch.zeros(4097))


# ---- the Trainer on a sparse device mask --------------------------------------------------------------------
TH, TW, TR, TS, TD, TSTEP = 48, 72, 64, 32, 64, 12


def _trainer(dev, depth_loss_type, graph):
    import model as mdl
    from model.optim import HipAdam
    from model.synthetic import make_cfg, vkitti_scene
    cfg = make_cfg(hidden=TD, S=TS)
    t = cfg["training"]
    t.update(n_training_points=TR, pc_weight=[0.0, 0.0], rgb_s_weight=[0.0, 0.0], depth_loss_type=depth_loss_type)
    data, c2w = vkitti_scene(dev, 0, TH, TW, 14.0)
    mask = torch.zeros(1, TH, TW, dtype=torch.bool)
    mask[:, ::TSTEP, ::TSTEP] = True                      # 4 x 6 = 24 valid pixels of 3456
    if depth_loss_type == "l1":                           # a sparse prior: no depth where the mask is off
        data["img.depth"] = torch.where(mask.to(dev), data["img.depth"].clamp_min(1.0), 0.0)
    data["img.depth_mask"] = mask.to(dev)
    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    nn_model = mdl.get_model(mdl.Renderer(net, cfg["rendering"], device=dev), cfg, device=dev)
    pose = mdl.LearnPose(1, False, False, cfg, init_c2w=c2w.unsqueeze(0).to(dev)).to(dev)
    tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), t, device=dev, pose_param_net=pose)
    if graph:
        tr.enable_graph_rng()
    return tr, data, mask.reshape(-1).to(dev)


def _spy_draws(monkeypatch):
    """Records the ray_idx tensor of every step head call (its third output)."""
    from model import training
    seen, head = [], training.step_head

    def spy(*a, **k):
        out = head(*a, **k)
        seen.append((out[2], a[-1].get("valid") is not None))
        return out
    monkeypatch.setattr(training, "step_head", spy)
    return seen


def test_trainer_draws_against_a_sparse_device_mask(dev, monkeypatch):
    """(1 - 24/3456)^64 = 0.64: most first draws miss every valid pixel, so the launch redraws."""
    tr, data, mask = _trainer(dev, "l1", graph=False)
    seen = _spy_draws(monkeypatch)
    torch.manual_seed(3)
    attempts = []
    for i in range(5):
        ld = tr.train_step(data, it=i, epoch=0, scheduling_start=0)
        assert all(bool(torch.isfinite(v).all()) for v in ld.values() if isinstance(v, torch.Tensor)), f"step {i}"
        assert tr.draw_attempts.dtype == torch.int32 and tr.draw_attempts.is_cuda
        attempts.append(tr.draw_attempts.item())
        idx, with_valid = seen[-1]
        assert with_valid and bool(mask[idx].any()), f"step {i}: no drawn ray has a valid depth"
    print("attempts per step:", attempts)
    assert len(seen) == 5 and all(a >= 1 for a in attempts)


def test_trainer_host_mask_rules(dev, monkeypatch):
    """A risky host mask is uploaded and drawn against; a host mask that rules the all-invalid draw out
    passes no mask (today's launch); graph mode refuses a risky host mask by name."""
    tr, data, mask = _trainer(dev, "l1", graph=False)
    seen = _spy_draws(monkeypatch)
    data["img.depth_mask"] = data["img.depth_mask"].cpu()
    tr.train_step(data, it=0, epoch=0, scheduling_start=0)
    assert seen[-1][1] and bool(mask[seen[-1][0]].any())
    data["img.depth_mask"] = torch.ones(1, TH, TW, dtype=torch.bool)
    tr.train_step(data, it=1, epoch=0, scheduling_start=0)
    assert not seen[-1][1]
    trg, datag, _ = _trainer(dev, "l1", graph=True)
    datag["img.depth_mask"] = datag["img.depth_mask"].cpu()
    with pytest.raises(RuntimeError, match="on the device"):
        trg.train_step(datag, it=0, epoch=0, scheduling_start=0)


@pytest.mark.parametrize("depth_loss_type", ["l1", "invariant"])
def test_trainer_graph_replay_on_a_sparse_device_mask(dev, depth_loss_type, monkeypatch):
    tr, data, mask = _trainer(dev, depth_loss_type, graph=True)
    seen = _spy_draws(monkeypatch)
    g, out = D.capture_graph(lambda: tr.train_step(data, it=0, epoch=0, scheduling_start=0))
    idx, with_valid = seen[-1]                 # the captured step's draw: replays rewrite it in place
    assert with_valid
    c0 = tr.seed_counter.item()
    draws, attempts = set(), []
    for k in range(20):
        g.replay()
        assert tr.seed_counter.item() == c0 + k + 1, "one counter advance per replay"
        assert bool(mask[idx].any()), f"replay {k}: no drawn ray has a valid depth"
        attempts.append(tr.draw_attempts.item())
        draws.add(tuple(idx[:8].tolist()))
    print("attempts per replay:", attempts)
    assert all(1 <= a <= D.MAX_ATTEMPTS for a in attempts) and len(draws) == 20
    assert "loss" in out
    # the invariant loss's value is not asserted: a draw with a single valid ray gives s = 0 and a NaN loss
    # by the reference's own expressions (include/nerf_hip.h), and the NaN then stays in the weights
    if depth_loss_type == "l1":
        assert bool(torch.isfinite(out["loss"]))
