"""The references and input sets of tests/test_gpu_prologue_fp64.py (tests/helpers.py) checked on the
CPU: Philox against its published known answers; the sampler reference's conditions on every case;
each fp64 reference against torch autograd of the oracle expression (oracle/nerf_oracle.py); every edge
set holds what it claims; and teeth -- for each bar of the GPU module the honest f32 reference passes
it on the test's own inputs and a named wrong variant does not."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as orc
from tests import helpers as H
from tests.helpers import T_GRAD, T_VALUE

F64 = torch.float64


def _close(a, b, rtol=1e-10, atol=1e-13):
    return torch.allclose(a.double().reshape(-1), b.double().reshape(-1), rtol=rtol, atol=atol)


# ---- Philox and the sampler ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox_known_answers(ctr, key, want):
    """The three known answers of Random123 for Philox-4x32-10, alone and inside a batch."""
    assert tuple(int(x) for x in H.philox4x32_10(np.array(ctr), np.array(key))) == want
    batch = H.philox4x32_10(np.array([ctr, (1, 2, 3, 4), ctr]), np.array(key))
    assert tuple(int(x) for x in batch[0]) == want == tuple(int(x) for x in batch[2])


@pytest.mark.parametrize("Hh,W,R", H.SAMPLE_CASES)
def test_sampler_reference_conditions(Hh, W, R):
    """Distinct, in range, at most 20 rounds at every (n, R) of the GPU module, plain and at the three
    counter values: a condition on the inputs (a seed that broke it would be replaced)."""
    n = Hh * W
    assert n >= 2 * R
    draws = [H.sample_rays_ref(n, R, H.SAMPLE_SEED)] + [H.sample_rays_ref(n, R, H.SAMPLE_SEED, counter=c) for c in range(3)]
    for idx, rounds in draws:
        assert idx.dtype == torch.int64 and idx.shape == (R,)
        assert int(idx.min()) >= 0 and int(idx.max()) < n and idx.unique().numel() == R
        assert 1 <= rounds <= H.SAMPLE_MAX_ROUNDS_USED
    assert H.sample_key(H.SAMPLE_SEED) != H.sample_key(H.SAMPLE_SEED, 0)
    if R > 3:
        assert not torch.equal(draws[0][0], draws[1][0]) and not torch.equal(draws[1][0], draws[2][0])


def test_sampler_cases_cover_the_slot_edges():
    Rs = [c[2] for c in H.SAMPLE_CASES]
    assert {1, 1023, 1024, 1025, 2049, 4095, 4096} <= set(Rs)
    assert sum(h * w == 2 * r for h, w, r in H.SAMPLE_CASES) >= 6 and (188, 621, 1024) in H.SAMPLE_CASES


@pytest.mark.parametrize("Hh,W,R", [c for c in H.SAMPLE_CASES if c[0] * c[1] == 2 * c[2] and c[2] > 3])
def test_sampler_teeth_larger_slot_wins(Hh, W, R):
    """A sampler in which the larger slot wins a tie draws another set at every dense case."""
    good, _ = H.sample_rays_ref(Hh * W, R, H.SAMPLE_SEED)
    bad, _ = H.sample_rays_ref(Hh * W, R, H.SAMPLE_SEED, _wrong="larger_slot_wins")
    assert bad.unique().numel() == R and not torch.equal(good, bad)


def test_pixels_ref_is_arange_pixels():
    idx = torch.tensor([0, 5, 61, 62, 2045])
    assert torch.equal(H.pixels_ref(idx, 33, 62), orc.arange_pixels(33, 62)[1][0][idx])
    assert torch.equal(H.pixels_ref(idx, 33, 62, F64), orc.arange_pixels(33, 62, dtype=F64)[1][0][idx])


# ---- fp64 references against the oracle expression -------------------------------------------------------
@pytest.mark.parametrize("scale", [s for s in H.POSE_R_SCALES if s > 0])
@pytest.mark.parametrize("with_init", [True, False])
def test_pose_reference_is_the_oracle_expression(scale, with_init):
    gen = torch.Generator().manual_seed(1)
    r0 = (scale * torch.tensor(H.POSE_AXIS, dtype=F64)).float()
    t0, g = torch.randn(3, generator=gen), torch.randn(4, 4, generator=gen)
    init = H.rigid_c2w(5) if with_init else None
    ref = H.pose_c2w_ref(r0, t0, init, g, F64)
    r, t = r0.double().requires_grad_(True), t0.double().requires_grad_(True)
    c2w = orc.make_c2w(r, t)
    c2w = c2w @ init.double() if with_init else c2w
    c2w.backward(g.double())
    assert _close(ref["c2w"], c2w.detach()) and _close(ref["g_t"], t.grad)
    assert _close(ref["g_r"], r.grad, rtol=1e-9, atol=1e-12 * max(1.0, r.grad.abs().max().item()))


def test_pose_reference_at_zero_rotation():
    """r = 0: the f32 and the fp64 expression give the same finite g_r (the norm's subgradient is 0, the
    [r]x term carries the gradient), the value the GPU module compares with."""
    g = torch.randn(4, 4, generator=torch.Generator().manual_seed(2))
    r64, e32, r32 = H.pose_c2w_refs(torch.zeros(3), torch.ones(3), H.rigid_c2w(4), g)
    assert bool(torch.isfinite(r64["g_r"]).all()) and r64["g_r"].abs().max().item() > 0 and e32["g_r"] < 1e-6
    assert abs(sum(x * x for x in H.POSE_AXIS) - 1.0) < 1e-12 and (1e-25 ** 2) < 1.4e-45      # the squares underflow


@pytest.mark.parametrize("flags", range(4))
def test_camera_reference_is_the_oracle_expression(flags):
    """With K = scale = I and world = inv(M) the oracle's unprojection matrix is M: values, the depth
    gradient, and gM through d inv(W) = -M dW M  (g_W = -M^T gM M^T)."""
    inp = H.camera_inputs(65)
    M = inp["M"].double()
    grads = {k: inp[k] for k in ("g_cam", "g_ray", "g_norm", "g_dsrc")}
    if not flags & 2:
        grads["g_view"] = inp["g_view"]
    ref = H.camera_rays_ref(M, inp["pix"], inp["depth"], flags, F64, grads)
    eye = torch.eye(4, dtype=F64)[None]
    W = torch.linalg.inv(M)[None].clone().requires_grad_(True)
    d = inp["depth"].double().view(1, -1, 1).clone().requires_grad_(True)
    cam, ray, ds, rn, mask = orc.rays_from_cameras(inp["pix"].double()[None], d, eye, W, eye, bool(flags & 1))
    for name, t in (("cam", cam), ("ray", ray), ("d_src", ds), ("ray_norm", rn)):
        assert _close(ref[name], t.detach(), 1e-9, 1e-11), name
    assert torch.equal(ref["mask"], mask)
    loss = (cam * grads["g_cam"]).sum() + (ray * grads["g_ray"]).sum() + (rn * grads["g_norm"]).sum() + (ds * grads["g_dsrc"]).sum()
    if not flags & 2:
        loss = loss + (-ray * grads["g_view"]).sum()
    loss.backward()
    gW = -(M.t() @ ref["gM"] @ M.t())
    assert _close(gW, W.grad[0], 1e-7, 1e-9 * W.grad.abs().max().item())
    assert _close(ref["g_depth"], d.grad.view(-1), 1e-9, 1e-11)
    assert bool((ref["condM"] >= ref["gM"].abs() * (1 - 1e-12)).all()) and bool((ref["gM"][3] == 0).all())


@pytest.mark.parametrize("l1", [0, 1])
def test_loss_reference_is_the_oracle_expression(l1):
    inp = H.ray_loss_inputs(342, 342, "all")
    inp["mask"] = torch.arange(342) % 4 != 1
    ref = H.ray_loss_ref(inp["rgb"], inp["gt"], inp["dp"], inp["dg"], inp["mask"], l1, 1.0, 0.04, dict(total=1.0, l2_mean=0.3), F64)
    r, p, q = (inp[k].double().clone().requires_grad_(True) for k in ("rgb", "dp", "dg"))
    l_rgb = orc.rgb_full_loss(r[None], inp["gt"].double()[None], "l1" if l1 else "l2")
    l_dep = orc.depth_l1_loss(p[inp["mask"]], q[inp["mask"]])
    l2m = torch.nn.functional.mse_loss(r, inp["gt"].double())
    total = 1.0 * l_rgb + 0.04 * l_dep
    (total + 0.3 * l2m).backward()
    for k, v in (("total", total), ("l_rgb", l_rgb), ("l_depth", l_dep), ("l2_mean", l2m)):
        assert _close(ref[k], v.detach()), k
    assert _close(ref["g_rgb"], r.grad) and _close(ref["g_dp"], p.grad) and _close(ref["g_dg"], q.grad)
    assert ref["cnt"] == float(inp["mask"].sum())


@pytest.mark.parametrize("shift_first,lo", [(False, float("-inf")), (True, float("-inf")), (False, 0.5), (True, 0.5)])
def test_affine_reference_is_torch_autograd(shift_first, lo):
    inp = H.depth_affine_inputs(1025, shift_first, lo)
    ref = H.depth_affine_ref(inp["d"], inp["s"], inp["t"], shift_first, lo, inp["g"])
    s, t = inp["s"].double().requires_grad_(True), inp["t"].double().requires_grad_(True)
    pre = (inp["d"].double() + t) * s if shift_first else inp["d"].double() * s + t
    # the clamp decision of the f32 expression, the reference's (entries within an ulp of lo differ in fp64)
    y = torch.where(ref["keep"], pre, torch.full_like(pre, lo if lo != float("-inf") else 0.0))
    y.backward(inp["g"].double())
    assert _close(ref["g_s"], s.grad) and _close(ref["g_t"], t.grad)
    assert ref["cond_s"] >= ref["g_s"].abs() and ref["cond_t"] >= ref["g_t"].abs()


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_reference_is_torch_adam(wd):
    """adam_ref at f32 against CPU torch.optim.Adam(foreach=False) within 4 ulp of max|p| after 5 steps,
    and at fp64 against the same optimiser on fp64 tensors."""
    p0, gs = H.adam_inputs(1025, steps=5)
    hyp = dict(H.ADAM_HYPER, wd=wd)
    for dt, tol in ((torch.float32, 4 * H.U24), (F64, 1e-13)):
        tp = torch.nn.Parameter(p0.to(dt).clone())
        opt = torch.optim.Adam([tp], lr=hyp["lr"], betas=(hyp["b1"], hyp["b2"]), eps=hyp["eps"], weight_decay=wd, foreach=False)
        for g in gs:
            tp.grad = g.to(dt).clone()
            opt.step()
        p, m, v = H.adam_ref(p0, gs, hyp, dt)
        st = opt.state[tp]
        for got, ref in ((p, tp.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert (got.double() - ref.double()).abs().max().item() <= tol * ref.abs().max().item()


def test_adam_reference_takes_slot_6_as_given():
    """Why adam_ref has `om2`: with slot 15 != 1 the kernel derives lr, beta1, beta2 from the f32 slots
    but still uses a non-zero slot 6 as 1 - beta2 (include/nerf_hip.h).  hyper_block stores f32(1 - 0.999)
    there, which is 1.3e-5 (relative) away from 1 - f32(0.999): a reference that formed 1 - beta2 from the
    f32 beta2 missed the bar on v by a factor 20 on the MI355X.  The reference was wrong, not the kernel."""
    b2, om2 = H.f32r(0.999), H.f32r(1 - 0.999)
    assert abs((1 - b2) / om2 - 1) > 1e-5
    p0, gs = H.adam_inputs(1025)
    hyp = dict(H.ADAM_HYPER, wd=0.0, b2=b2)
    v_own, v_slot = H.adam_ref(p0, gs, hyp, F64)[2], H.adam_ref(p0, gs, dict(hyp, om2=om2), F64)[2]
    assert (v_own - v_slot).abs().max().item() > 5e-6 * v_slot.abs().max().item()


# ---- the pack references -----------------------------------------------------------------------------------
def test_chain_perm_is_a_block_permutation():
    for t in range(0, 320, 32):
        img = [H.chain_perm_ref(c) for c in range(t, t + 32)]
        assert sorted(img) == list(range(t, t + 32)) and img != list(range(t, t + 32))
    assert [H.chain_perm_ref(c) for c in range(8)] == [0, 1, 2, 3, 16, 17, 18, 19]
    assert [H.chain_perm_ref(c) for c in range(40, 48)] == [36, 37, 38, 39, 52, 53, 54, 55]
    assert H.chain_perm_index(64, 32).tolist()[32:] == list(range(32, 64))


def _edge_matrix():
    W = H.pack_edge_rows(torch.randn(40, 50, generator=torch.Generator().manual_seed(0)))
    Wp = torch.zeros(64, 64)
    Wp[:40, :50] = W
    return W, Wp


def test_pair_image_reconstructs_and_edge_rows():
    W, Wp = _edge_matrix()
    assert bool((W[1] == 0).all()) and W[2].abs().max().item() == 0.125
    assert 0 < W[3].abs().max().item() < 2.0 ** -126 and 2.9e38 < W[4].abs().max().item() < 3.1e38
    for perm in (None, H.chain_perm_index(64, 32), H.chain_perm_index(64, 64)):
        f = H.pair_image_ref(Wp, perm, compact=True)
        assert f["e"].tolist()[1:5] == [0, 17, 140, -113] and torch.equal(f["e"], f["ce"])
        src = Wp if perm is None else Wp[:, perm]
        rmax = src.abs().amax(1).double()
        assert bool(((H.pair_image_value(f) - src.double()).abs() <= 2.0 ** -22 * rmax.unsqueeze(1) + 1e-45).all())
        scaled = rmax * torch.pow(2.0, f["e"].double())
        live = (rmax >= 2.0 ** -126)
        assert bool(((scaled[live] >= 2.0 ** 14) & (scaled[live] < 2.0 ** 15)).all())
    img = torch.stack([f["hi"], f["lo"], torch.zeros_like(f["hi"])])
    img[2, 0, :, 0:2] = f["e"].view(-1, 1).view(torch.int16).view(-1, 2)
    img[2, 1].view(-1)[:128] = f["ce"].view(torch.int16)
    back = H.pair_image_read(img, compact=True)
    assert all(torch.equal(back[k], f[k]) for k in f)


def test_pack_teeth_chain_order():
    """chain_perm with the two 16-halves exchanged, and a transposed chain image that permutes the rows
    of dst_t (the columns of the weight) instead of its columns, give other images."""
    _, Wp = _edge_matrix()
    Wp = Wp + torch.randn(64, 64, generator=torch.Generator().manual_seed(1)) * (Wp == 0)
    for k in (32, 64):
        good = H.pair_image_ref(Wp, H.chain_perm_index(64, k), True)
        bad = H.pair_image_ref(Wp, H.chain_perm_index(64, k, "halves_exchanged"), True)
        assert not torch.equal(good["hi"], bad["hi"])
    Wt = Wp.t().contiguous()
    perm = H.chain_perm_index(64, 64)
    good, bad = H.pair_image_ref(Wt, perm, True), H.pair_image_ref(Wt[perm], None, True)
    assert not torch.equal(good["hi"], bad["hi"])
    assert torch.equal(H.image_ref(Wp)[0].permute(1, 0, 2).reshape(64, 64).view(torch.bfloat16), Wp.bfloat16())


# ---- the edge sets hold what they claim --------------------------------------------------------------------
def test_edge_sets():
    for n in H.MAT4_BATCHES:
        A, kinds = H.mat4_edge_batch(n)
        assert A.shape == (n, 4, 4) and bool((torch.linalg.det(A.double()).abs() > 1e-3).all())
        if n >= 63:
            assert all(len(v) >= 7 for v in kinds.values())
            assert bool((A[kinds["zero_pivot"], 0, 0] == 0).all())
            P = A[kinds["perm"][0]]
            assert int((P != 0).sum()) == 4 and bool((P.diagonal() == 0).all())
            c = torch.linalg.cond(A[kinds["ill"]].double())
            assert bool((c > 3e4).all()) and bool((c < 3e5).all())
            Rm = A[kinds["rigid"][0], :3, :3].double()
            assert _close(Rm @ Rm.t(), torch.eye(3, dtype=F64), 0, 1e-5)
        else:
            assert A[0, 0, 0] == 0
    for n in H.AFFINE_N:
        for sf in (False, True):
            inp = H.depth_affine_inputs(n, sf, 0.5)
            pre = H.affine32(inp["d"], inp["s"], inp["t"], sf)
            if n >= 63:
                assert inp["at_lo"] and inp["below"] and inp["zero"]
                assert bool((pre[inp["at_lo"]] == 0.5).all()) and bool((pre[inp["below"]] < 0.5).all())
                assert bool((inp["d"][inp["zero"]] == 0).all())
                nxt = torch.nextafter(inp["d"][inp["below"]], torch.tensor(9.0))
                assert bool((H.affine32(nxt, inp["s"], inp["t"], sf) >= 0.5).all())
    assert {1, 1024, 1025, 65536, 65537} <= set(H.AFFINE_N)
    for R in H.CAMERA_R:
        inp = H.camera_inputs(R, nonfinite=True)
        k, d = inp["kinds"], inp["depth"]
        assert bool((d[k["zero"]] == 0).all()) and bool((d[k["neg"]] < 0).all()) and k["zero"]
        if R >= 4:
            assert d[k["inf"]].item() == float("inf") and bool(torch.isnan(d[k["nan"]]).all())
            assert k["neg"] or R < 10
        assert bool(torch.isfinite(H.camera_inputs(R)["depth"]).all())
    for R, nd in H.LOSS_SHAPES:
        for mk, cnt in (("none", None), ("all", nd), ("one", 1), ("zero", 0)):
            inp = H.ray_loss_inputs(R, nd, mk)
            assert bool((inp["rgb"] == inp["gt"]).any()) and bool((inp["dp"] == inp["dg"]).any())
            assert (inp["mask"] is None) if cnt is None else int(inp["mask"].sum()) == cnt
    assert {(341, 341), (342, 342)} <= set(H.LOSS_SHAPES) and 3 * 341 < 1024 < 3 * 342
    for n in H.ADAM_N:
        p, gs = H.adam_inputs(n)
        assert len(gs) == 3 and p.shape == (n,)
        if n > 1024:
            a = torch.cat(gs).abs()
            assert bool((a == 0).any()) and a[a > 0].min().item() < 1e-18 and a.max().item() > 1e3
        assert bool((gs[0][-(n % 4 or 1):].abs() > 1e-3).all())
    assert {n % 4 for n in H.ADAM_N} == {0, 1, 2, 3} and 524288 == 512 * 256 * 4


# ---- teeth: the honest f32 reference passes each GPU bar, a wrong one does not ---------------------------
def _both(check, good, bad):
    check(good)
    with pytest.raises(AssertionError):
        check(bad)


@pytest.mark.parametrize("n", [5, 7, 1025, 525315])
@pytest.mark.parametrize("wrong", ["tail_untouched", "step_not_advanced"])
def test_adam_teeth(n, wrong):
    p0, gs = H.adam_inputs(n)
    for wd in (0.0, 0.01):
        hyp = dict(H.ADAM_HYPER, wd=wd)
        r64, e32, r32 = H.adam_refs(p0, gs, hyp)

        def check(got):
            for t, ref, e in zip(got, r64, e32):
                assert bool(torch.isfinite(t).all())
                assert (t.double() - ref).abs().max().item() <= H.adam_bar(ref, e)
        _both(check, r32, H.adam_ref(p0, gs, hyp, torch.float32, _wrong=wrong))


def _loss_check(inp, l1, R, nd):
    r64, e32, _ = H.ray_loss_refs(inp, l1, H.LOSS_GO)
    bars = H.ray_loss_scalar_bars(r64, R, nd, l1)

    def check(got):
        for k in ("total", "l_rgb", "l_depth", "l2_mean"):
            H.assert_sum_bar(k, got[k], r64[k], torch.tensor(bars[k], dtype=F64), 1.0)
        assert got["cnt"] == r64["cnt"]
        for k in ("g_rgb", "g_dp", "g_dg"):
            H.assert_max_bar(k, got[k], r64[k], e32[k], T_VALUE)
    return check


@pytest.mark.parametrize("wrong,mask", [("div_3R", "all"), ("mask_ignored", "one"), ("cnt_unclamped", "zero")])
@pytest.mark.parametrize("l1", [0, 1])
def test_loss_teeth(wrong, mask, l1):
    for R, nd in ((22, 22), (342, 342), (5, 40)):
        inp = H.ray_loss_inputs(R, nd, mask)
        a = (inp["rgb"], inp["gt"], inp["dp"], inp["dg"], inp["mask"], l1, H.LOSS_W_RGB, H.LOSS_W_DEPTH, H.LOSS_GO, torch.float32)
        _both(_loss_check(inp, l1, R, nd), H.ray_loss_ref(*a), H.ray_loss_ref(*a, _wrong=wrong))


@pytest.mark.parametrize("wrong", ["clamped_pass", "shift_first_swapped"])
@pytest.mark.parametrize("n", [63, 1025, 66600])
def test_affine_teeth(wrong, n):
    """The f32 sum in the kernel's order stays inside tree_ceiling; clamped entries passing gradient and
    a swapped shift_first do not."""
    for sf in (False, True):
        inp = H.depth_affine_inputs(n, sf, 0.5)
        ref = H.depth_affine_ref(inp["d"], inp["s"], inp["t"], sf, 0.5, inp["g"])

        def f32_run(w):
            r = H.depth_affine_ref(inp["d"], inp["s"], inp["t"], sf, 0.5, inp["g"], torch.float32, _wrong=w)
            sfw = (not sf) if w == "shift_first_swapped" else sf
            d, s, t, g = inp["d"], inp["s"], inp["t"], inp["g"]
            ts = (g * ((d + t) if sfw else d))[r["keep"]]
            tt = (g * (s if sfw else torch.ones(1)))[r["keep"]]
            return H.f32_tree_sum(ts), H.f32_tree_sum(tt)

        def check(got):
            c = H.tree_ceiling(n, 1024)
            H.assert_sum_bar("g_s", got[0], ref["g_s"], ref["cond_s"], c)
            H.assert_sum_bar("g_t", got[1], ref["g_t"], ref["cond_t"], c)
        _both(check, f32_run(None), f32_run(wrong))


@pytest.mark.parametrize("wrong,flags", [("dsrc_no_norm_div", 0), ("dsrc_no_norm_div", 2), ("view_grad_dropped", 0),
                                         ("view_grad_dropped", 1)])
def test_camera_teeth(wrong, flags):
    for R in (65, 1025):
        inp = H.camera_inputs(R)
        grads = {k: inp[k] for k in ("g_cam", "g_ray", "g_view", "g_norm", "g_dsrc")}
        r64, e32, r32 = H.camera_rays_refs(inp["M"], inp["pix"], inp["depth"], flags, grads)

        def check(got):
            for k in ("cam", "ray", "view", "ray_norm", "d_src"):
                H.assert_max_bar(k, got[k], r64[k], e32[k], T_VALUE)
            H.assert_sum_bar("gM", got["gM"], r64["gM"], r64["condM"], H.tree_ceiling(R, 1024), e32["gM"])
            H.assert_max_bar("g_depth", got["g_depth"], r64["g_depth"], e32["g_depth"], T_GRAD)
        _both(check, r32, H.camera_rays_ref(inp["M"], inp["pix"], inp["depth"], flags, torch.float32, grads, _wrong=wrong))
        one = H.camera_rays_ref(inp["M"], inp["pix"], None, flags, torch.float32)
        assert bool((one["d_src"] == 1).all()) and bool(one["mask"].all())


def test_tree_ceiling_and_bars():
    assert H.tree_ceiling(1, 1024) == 27 * H.U24 and H.tree_ceiling(1025, 1024) == 28 * H.U24
    assert H.tree_ceiling(66600, 1024) == (66 + 26) * H.U24
    x = torch.randn(66600, generator=torch.Generator().manual_seed(0))
    assert abs(H.f32_tree_sum(x).item() - x.double().sum().item()) <= H.tree_ceiling(66600, 1024) * x.abs().double().sum().item()
    assert H.f32r(0.04) != 0.04 and H.LOSS_W_DEPTH == H.f32r(0.04)
