"""The references of tests/helpers_depth_prior.py checked on the host: the draw-until-valid rule against
helpers.sample_rays_ref, the fixed seeds of the GPU cases, the invariant depth loss against
oracle.depth_invariant_loss -- and that each wrong variant fails the same assertions (no GPU needed)."""
import numpy as np
import pytest
import torch

from model import _hip
from oracle import nerf_oracle as orc
from tests import helpers as H
from tests import helpers_depth_prior as D

GO = {k: H.LOSS_GO[k] for k in ("total", "l_rgb", "l_depth", "l2_mean")}


# ---- the binding (these fail without the four entries) ----------------------------------------------------
def test_the_four_entries_are_declared_bound_and_exported():
    names = ("nerf_sample_rays_valid", "nerf_step_head_valid", "nerf_ray_loss_invariant", "nerf_ray_loss_invariant_bwd")
    lib = _hip.load_library()
    for n in names:
        assert n in _hip.EXPORTED_SYMBOLS and hasattr(lib, n), n
    assert lib.nerf_hip_abi_version() == 15 and _hip.SAMPLE_MAX_ATTEMPTS == D.MAX_ATTEMPTS == 64
    # argument checks return before any HIP call
    one = 16
    rc = lib.nerf_ray_loss_invariant(one, one, 4, one, one, None, 4097, 0, 1.0, 1.0, one, one, one, one, one, None)
    assert rc == -1 and b"n_depth" in lib.nerf_hip_last_error()
    rc = lib.nerf_ray_loss_invariant_bwd(one, one, 4, one, one, None, 4097, 0, 1.0, 1.0, None, None, None, None, one,
                                         None, None, None, None)
    assert rc == -1 and b"n_depth" in lib.nerf_hip_last_error()
    rc = lib.nerf_sample_rays_valid(100, 80, 1, 10, 10, None, one, one, None, None, None, None, None, None)
    assert rc == -1 and b"2*n_rays" in lib.nerf_hip_last_error()
    rc = lib.nerf_step_head_valid(None, one, None, None, 0, None)
    assert rc == -1


# ---- draw until valid -------------------------------------------------------------------------------------
def _check_rule(ref):
    """What the attempt rule promises, as assertions on a reference implementation `ref`."""
    Hh, W, R = D.SMALL
    n, mask = Hh * W, D.small_mask()
    for seed in D.SMALL_SEEDS.values():
        idx, rounds, att = ref(n, R, seed, mask)
        assert 1 <= att <= D.MAX_ATTEMPTS
        want, wrounds = H.sample_rays_ref(n, R, D.attempt_seed(seed, att - 1))
        assert torch.equal(idx, want) and rounds == wrounds
        assert mask[idx.numpy()].any()
        for a in range(att - 1):      # every earlier attempt missed the valid pixel
            assert not mask[H.sample_rays_ref(n, R, D.attempt_seed(seed, a))[0].numpy()].any()
        # with a counter the attempts are those of the mixed key
        idx_c, _, att_c = ref(n, R, seed, mask, counter=3)
        assert torch.equal(idx_c, H.sample_rays_ref(n, R, D.attempt_seed(seed, att_c - 1), counter=3)[0])


def test_attempt_rule_and_its_wrong_variants():
    _check_rule(D.sample_rays_valid_ref)
    for wrong in ("same_seed", "attempt_in_counter"):
        with pytest.raises(AssertionError):
            _check_rule(lambda *a, **k: D.sample_rays_valid_ref(*a, _wrong=wrong, **k))


def test_attempt_zero_is_the_plain_draw():
    for (Hh, W, R), seed in ((D.SMALL, 5), (D.STRIPE, 11)):
        n = Hh * W
        idx, rounds, att = D.sample_rays_valid_ref(n, R, seed, np.ones(n, dtype=np.uint8))
        ref, rr = H.sample_rays_ref(n, R, seed)
        assert att == 1 and rounds == rr and torch.equal(idx, ref)
        idx, rounds, att = D.sample_rays_valid_ref(n, R, seed, None, counter=2)
        assert att == 1 and torch.equal(idx, H.sample_rays_ref(n, R, seed, counter=2)[0])
    assert D.attempt_seed(2 ** 64 - 1, 1) == D.ATTEMPT_STEP - 1      # mod 2^64


def test_fixed_seeds_need_the_attempts_they_are_named_for():
    """The GPU cases' seeds: exactly 1, exactly 2 and >= 5 attempts at (100, 4); 1 and >= 2 on the stripe mask;
    all within the cap, by the reference alone."""
    Hh, W, R = D.SMALL
    att = {k: D.sample_rays_valid_ref(Hh * W, R, s, D.small_mask())[2] for k, s in D.SMALL_SEEDS.items()}
    assert att[1] == 1 and att[2] == 2 and 5 <= att[5] <= D.MAX_ATTEMPTS, att
    Hh, W, R = D.STRIPE
    att = {k: D.sample_rays_valid_ref(Hh * W, R, s, D.stripe_mask())[2] for k, s in D.STRIPE_SEEDS.items()}
    assert att[1] == 1 and 2 <= att[2] <= D.MAX_ATTEMPTS, att
    assert D.stripe_mask().sum() == 16
    # no valid pixel: attempts 0 and the last attempt's draw
    Hh, W, R = D.SMALL
    idx, rounds, a0 = D.sample_rays_valid_ref(Hh * W, R, 9, np.zeros(Hh * W, dtype=np.uint8))
    assert a0 == 0 and torch.equal(idx, H.sample_rays_ref(Hh * W, R, D.attempt_seed(9, D.MAX_ATTEMPTS - 1))[0])


# ---- the invariant loss -----------------------------------------------------------------------------------
def _masked(inp, dtype):
    m = slice(None) if inp["mask"] is None else inp["mask"]
    return inp["dp"].to(dtype)[m], inp["dg"].to(dtype)[m]


@pytest.mark.parametrize("n,kind,ties", [(65, "none", 0), (64, "all", 0), (1025, "third", 0), (4, "two", 0),
                                         (1023, "none", 5), (66, "third", 5)])
def test_invariant_reference_agrees_with_the_oracle(n, kind, ties):
    inp = D.invariant_inputs(n, kind, ties=ties)
    r64, e32, r32 = D.invariant_refs(inp, True, GO)
    for dtype, r in ((torch.float64, r64), (torch.float32, r32)):
        p, g = _masked(inp, dtype)
        assert torch.equal(r["l_depth"], orc.depth_invariant_loss(p, g))
    assert e32["l_depth"] <= 1e-5 * abs(r64["l_depth"].item())
    if ties:
        assert r64["ties_p"] == ties and r64["ties_g"] == ties
    # the closed form the kernels evaluate is autograd's gradient
    a_dep = GO["total"] * H.LOSS_W_DEPTH + GO["l_depth"]
    l, gp, gg, st = D.invariant_closed_form(inp["dp"], inp["dg"], inp["mask"], a_dep)
    assert abs(l.item() - r64["l_depth"].item()) <= 1e-13 * abs(r64["l_depth"].item())
    assert st["t_p"] == r64["t_p"] and st["t_g"] == r64["t_g"] and st["ties_p"] == r64["ties_p"]
    for got, ref in ((gp, r64["g_dp"]), (gg, r64["g_dg"])):
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def _check_median_and_ties(ref):
    # the even count's lower middle value
    d = dict(rgb=torch.rand(3, 3), gt=torch.rand(3, 3), dp=torch.tensor([4.0, 1.0, 3.0, 2.0]),
             dg=torch.tensor([1.0, 5.0, 2.0, 9.0]), mask=None)
    r = ref(d["rgb"], d["gt"], d["dp"], d["dg"], None, True, 1.0, 1.0, dict(l_depth=1.0), torch.float64)
    assert r["t_p"].item() == 2.0 and r["t_g"].item() == 2.0
    # the median's gradient is spread evenly over the entries equal to it: with p = [1, 2, 2, 3, 5, 0] the two
    # tied entries carry the same gradient
    dp = torch.tensor([1.0, 2.0, 2.0, 3.0, 5.0, 0.0])
    dg = torch.tensor([0.3, 1.1, 1.1, 2.0, 0.7, 5.0])
    r = ref(d["rgb"], d["gt"], dp, dg, None, True, 1.0, 1.0, dict(l_depth=1.0), torch.float64)
    assert r["g_dp"][1].item() == r["g_dp"][2].item() and r["g_dg"][1].item() == r["g_dg"][2].item()
    _, gp, gg, _ = D.invariant_closed_form(dp, dg, None, 1.0)
    assert (gp - r["g_dp"]).abs().max().item() < 1e-12 and (gg - r["g_dg"]).abs().max().item() < 1e-12


def test_lower_median_tie_gradient_and_their_wrong_variants():
    _check_median_and_ties(D.invariant_ref)
    for wrong in ("upper_median", "single_tie"):
        with pytest.raises(AssertionError):
            _check_median_and_ties(lambda *a, **k: D.invariant_ref(*a, _wrong=wrong, **k))


def test_nan_pattern_at_degenerate_counts():
    """cnt = 0, cnt = 1 and an all-equal input: l_depth and total are NaN, g_rgb is finite, the depth
    gradients are NaN on the masked entries (none at cnt = 0) and 0 elsewhere."""
    rgb, gt = torch.rand(5, 3), torch.rand(5, 3)
    dp, dg = torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([2.0, 2.5, 1.0, 7.0])
    cases = [(dp, dg, torch.zeros(4, dtype=torch.bool)), (dp, dg, torch.tensor([False, True, False, False])),
             (torch.full((4,), 2.0), dg, torch.ones(4, dtype=torch.bool))]
    for p, g, m in cases:
        for dtype in (torch.float64, torch.float32):
            r = D.invariant_ref(rgb, gt, p, g, m, False, 1.0, 0.04, GO, dtype)
            assert torch.isnan(r["l_depth"]) and torch.isnan(r["total"]) and torch.isfinite(r["l2_mean"])
            assert torch.isfinite(r["g_rgb"]).all()
            for k in ("g_dp", "g_dg"):
                assert torch.equal(torch.isnan(r[k]), m) and bool((r[k][~m] == 0).all())
        l, gp, gg, _ = D.invariant_closed_form(p, g, m, 1.0)
        assert torch.isnan(l) and torch.equal(torch.isnan(gp), m) and torch.equal(torch.isnan(gg), m)
