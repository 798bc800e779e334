"""The torch restatements of tests/march_ref.py against the code they restate (Renderer.ray_marching,
Renderer.secant, on CPU tensors with an injected field), the edge rows against three wrong select
rules, and the segment identity of nerf_march_rays.  No GPU."""
import math

import pytest
import torch

from model.rendering import Renderer, get_sphere_intersection
from tests import march_ref as MR


class _InjectedField:
    """model(p, only_occupancy=True) returning injected occupancies in call order."""

    def __init__(self, occ_rows, mids=()):
        self.occ_rows, self.mids, self.calls = occ_rows, list(mids), 0

    def __call__(self, p, only_occupancy=True, it=0):
        self.calls += 1
        if self.calls == 1:
            return self.occ_rows.reshape(-1, 1)
        return self.mids.pop(0).reshape(*p.shape[:-1], 1)


def _renderer():
    r = Renderer.__new__(Renderer)
    torch.nn.Module.__init__(r)
    return r


def _rays(R, seed=0):
    g = torch.Generator().manual_seed(seed)
    cam = torch.tensor([0.15, -0.1, 2.0]).expand(R, 3).contiguous()
    ray = torch.randn(R, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, -1.0])
    return cam, ray / ray.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("n", [2, 5, 64, 65])
def test_select_ref_is_ray_marching(n):
    """With no secant step, ray_marching's output is the first d_pred of the bracket rows, inf and 0
    elsewhere: the dense restatement gives the same numbers on the edge rows and on generic ones."""
    R, rad = 40, 4.0
    cam, ray = _rays(R)
    occ, _, names = MR.select_case(n, R, 0.0)
    assert len(names) >= 5
    d_far = get_sphere_intersection(cam[:1], ray.unsqueeze(0), r=rad)[0][0, :, 1]
    rnd = _renderer()
    got = rnd.ray_marching(cam.unsqueeze(0), ray.unsqueeze(0), _InjectedField(occ), tau=0.0,
                           n_steps=[n, n + 1], n_secant_steps=0, rad=rad)[0]
    state, f_low, f_high, d_low, d_high = MR.select_ref(occ, d_far, 0.0, 0.0)
    want = torch.where(state == MR.BRACKET, MR.secant_pred(f_low, f_high, d_low, d_high),
                       torch.where(state == MR.INSIDE, 0.0, math.inf))
    assert torch.equal(got, want)
    assert {int(s) for s in state} == {0, 1, 2}


EXPECT = {   # name -> (state, j*) of the right rule
    "last_pair": (1, None), "all_negative": (0, None), "first_zero_later_change": (2, None),
    "first_positive_later_change": (2, None), "zero_product": (0, None), "zero_then_change": (1, 2),
    "first_change_wrong_way": (0, None), "wrong_way_then_right": (0, None), "underflow_pair": (0, None),
    "underflow_then_change": (0, None), "subnormal_product": (1, 0), "first_pair": (1, 0), "nan_product": (1, 2)}


def test_edge_rows_have_the_states_the_rule_gives():
    n = 9
    rows = MR.select_edge_rows(n)
    assert set(rows) == set(EXPECT)
    d_far = torch.full((1,), 2.0)
    for name, row in rows.items():
        state, f_low, f_high, d_low, d_high = MR.select_ref(row.view(1, n), d_far, 0.0, 0.0)
        st, j = EXPECT[name]
        assert int(state[0]) == st, name
        if name == "last_pair":
            j = n - 2
        if st == 1:
            assert f_low[0] == row[j] and f_high[0] == row[j + 1], name
            assert abs(d_low[0].item() - 2.0 * j / (n - 1)) < 1e-6 and abs(d_high[0].item() - 2.0 * (j + 1) / (n - 1)) < 1e-6
    # the f32 products behave as the rows assume
    t, s = torch.tensor(1e-30), torch.tensor(1e-20)
    assert (-t * t).item() == 0.0 and math.copysign(1.0, (-t * t).item()) == -1.0
    assert -1.5e-38 < (-s * s).item() < 0.0


@pytest.mark.parametrize("wrong,rows", [("neg_to_pos", ["wrong_way_then_right"]),
                                        ("no_product", ["underflow_pair", "wrong_way_then_right"]),
                                        ("no_first", ["first_zero_later_change", "first_positive_later_change"])])
def test_edge_rows_separate_the_wrong_rules(wrong, rows):
    n = 9
    edge = MR.select_edge_rows(n)
    d_far = torch.full((1,), 2.0)
    for name in rows:
        right = MR.select_ref(edge[name].view(1, n), d_far, 0.0, 0.0)[0]
        bad = MR.select_ref(edge[name].view(1, n), d_far, 0.0, 0.0, _wrong=wrong)[0]
        assert int(right[0]) != int(bad[0]), (wrong, name)
    # and on rows without an edge the wrong rules agree with the right one: they are wrong only there
    occ, d_far, _ = MR.select_case(33, 50, 0.5)
    right = MR.select_ref(occ, d_far, 0.0, 0.5)
    bad = MR.select_ref(occ, d_far, 0.0, 0.5, _wrong=wrong)
    if wrong != "no_first":
        assert all(torch.equal(a, b) for a, b in zip(right, bad))


def test_secant_update_is_renderer_secant():
    """Renderer.secant over three steps with injected mid occupancies = three secant_update calls."""
    R, tau = 64, 0.5
    g = torch.Generator().manual_seed(4)
    f_low, f_high = -0.05 - 0.4 * torch.rand(R, generator=g), 0.05 + 0.4 * torch.rand(R, generator=g)
    d_low = 0.5 + torch.rand(R, generator=g)
    d_high = d_low + 0.01 + 0.1 * torch.rand(R, generator=g)
    mids = [torch.rand(R, generator=g) for _ in range(3)]
    cam, ray = _rays(R)
    field = _InjectedField(None, mids)
    field.calls = 1
    got = _renderer().secant(f_low, f_high, d_low, d_high, 3, cam, ray, tau, model=field)
    b = (f_low, f_high, d_low, d_high, MR.secant_pred(f_low, f_high, d_low, d_high))
    for m in mids:
        b = MR.secant_update(*b, m - tau)
    assert torch.equal(got, b[4])
    # the f64 variant differs from it by rounding only
    b64 = tuple(t.double() for t in (f_low, f_high, d_low, d_high))
    assert (MR.secant_pred(*b64) - MR.secant_pred(f_low, f_high, d_low, d_high)).abs().max() < 1e-6


@pytest.mark.parametrize("n,seg", [(512, 128), (512, 512), (256, 64), (6, 2)])
def test_segment_identity(n, seg):
    """The pseudo-rays of nerf_march_rays sampled at linspace(0, 1, seg) are the reference's d_proposal
    points: in f64 to rounding of the f32 pseudo-rays, in f32 arithmetic within 4 ulp of |cam| + d_far."""
    R, rad, d0 = 48, 4.0, 0.0
    cam, ray = _rays(R, seed=2)
    d_far32 = get_sphere_intersection(cam[:1], ray.unsqueeze(0), r=rad)[0][0, :, 1]
    d_far, o_seg, d_seg = MR.march_rays_ref(cam, ray, rad, d0, n, seg)
    assert o_seg.shape == (R, n // seg, 3) and d_seg.shape == (R, n // seg, 3)
    scale = MR.ulp32(cam.double().norm(dim=-1) + d_far.double()).view(R, 1, 1)
    assert ((d_far.double() - d_far32.double()).abs() <= 4 * MR.ulp32(d_far.double())).all()
    ref64 = MR.proposal_points(cam.double(), ray.double(), MR.sphere_far(cam[0].double(), ray.double(), rad)[0], d0, n)
    got64 = MR.segment_points(o_seg, d_seg, seg, torch.float64)
    assert ((got64 - ref64).abs() <= 4 * scale).all()
    ref32 = MR.proposal_points(cam, ray, d_far32, d0, n)
    got32 = MR.segment_points(o_seg, d_seg, seg, torch.float32)
    assert ((got32.double() - ref32.double()).abs() <= 4 * scale).all()


def test_sphere_far_decides_the_tangent_rays():
    """The two near-tangent rays of the GPU test: u is a few f32 roundings from 0 and has one sign in
    f32 and in f64."""
    ray = torch.tensor([[0.0, 1.0, 0.0]])
    for x, positive in ((1.0 - 2.0 ** -20, True), (1.0 + 2.0 ** -20, False)):
        cam0 = torch.tensor([x, 0.0, 0.0])
        u32, u64 = MR.sphere_far(cam0, ray, 1.0)[1], MR.sphere_far(cam0.double(), ray.double(), 1.0)[1]
        assert 0 < abs(u64.item()) < 4e-6
        assert (u32.item() > 0) == positive and (u64.item() > 0) == positive
