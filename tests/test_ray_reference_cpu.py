"""The fp64 / f32 composite reference and the edge inputs of tests/test_gpu_ray_kernels_fp64.py
(tests/helpers.py) checked on the CPU: finite at every (S, flags) the GPU test uses, and the
saturated set holds the rays it claims."""
import pytest
import torch

from tests import helpers as H

R = H.COMPOSITE_R


@pytest.mark.parametrize("S", H.COMPOSITE_S16 + H.COMPOSITE_SWAVE)
def test_references_are_finite(S):
    """Both references stay finite on both input kinds under all eight flag values: the bar of the
    GPU test (T_project + 4 E_f32) is a number everywhere."""
    for kind in H.COMPOSITE_KINDS:
        raw, z, g_rgb, g_dist = H.composite_edge_inputs(R, S, S, kind)
        assert bool((z[:, 1:] >= z[:, :-1]).all())                     # depths stay sorted
        for flags in range(8):
            for dtype in (torch.float64, torch.float32):
                for name, t in zip(("rgb", "dist", "alpha", "grad"), H.composite_ref(raw, z, flags, g_rgb, g_dist, dtype)):
                    assert bool(torch.isfinite(t).all()), (S, kind, flags, dtype, name)
            _, e32 = H.composite_refs(raw, z, flags, g_rgb, g_dist)
            assert all(0.0 <= e < 1e-2 for e in e32.values()), (S, kind, flags, e32)


@pytest.mark.parametrize("S", [17, 64, 129, 257, 1024])
def test_saturated_set_contains_its_edges(S):
    """At least one ray whose f32 transmittance reaches exactly 0, one sample with a softplus input
    above 20 (torch's linear branch), one zero depth step, one sample with relu(raw) == 0, a ray
    with saturated colours and a ray with a zero upstream gradient."""
    raw, z, g_rgb, g_dist = H.composite_edge_inputs(R, S, S, "saturated")
    r3 = raw.view(R, S, 4)
    assert bool((r3[:, :, 0] > 20).any())
    assert bool((torch.relu(r3[:, :, 0]) == 0).any()) and bool((r3[:, :, 0] == 0).any())
    assert bool(((z[:, 1:] - z[:, :-1]) == 0).any())
    assert bool((torch.sigmoid(r3[:, :, 1:]) == 1).any()) and bool((r3[:, :, 1:] == -40).any())
    assert bool(((g_rgb == 0).all(1) & (g_dist == 0)).any())
    # the f32 transmittance of rendering.py:123 (exclusive cumprod of 1 - alpha + eps), softplus density
    alpha = H.composite_ref(raw, z, 0, g_rgb, g_dist, torch.float32)[2]
    assert bool((alpha == 1).any())
    trans = torch.cumprod(1.0 - alpha + 1e-6, -1)
    hit = (trans == 0).any(1)
    assert bool(hit.any()) and bool((trans[hit][:, 0] > 0).all())      # it gets there by underflow
    # the generic set stays at moderate densities and colours: no alpha of exactly 1, no colour of 0 or 1
    raw_g, z_g, gr, gd = H.composite_edge_inputs(R, S, S, "generic")
    assert bool((raw_g.abs() < 15).all())
    assert bool((H.composite_ref(raw_g, z_g, 0, gr, gd, torch.float32)[2] < 1).all())


def test_reference_is_the_inline_oracle_of_the_existing_test():
    """composite_ref in fp64 is what test_composite_fwd_bwd builds inline, bit for bit."""
    from oracle import nerf_oracle as orc
    S, flags = 100, 1
    raw, z, g_rgb, g_dist = H.composite_edge_inputs(R, S, 3, "generic")
    rgb, dist, alpha, graw = H.composite_ref(raw, z, flags, g_rgb, g_dist, torch.float64)
    rr = raw.double().clone().requires_grad_(True)
    sig = torch.nn.functional.softplus(rr[:, 0])
    c = torch.sigmoid(rr[:, 1:])
    o_rgb, o_dist, o_alpha, _ = orc.composite(sig.view(R, S), c.view(R, S, 3), z.double(), dist_alpha=True,
                                              white_background=False)
    (o_rgb * g_rgb.double()).sum().add((o_dist * g_dist.double()).sum()).backward()
    assert torch.equal(rgb, o_rgb) and torch.equal(dist, o_dist) and torch.equal(alpha, o_alpha)
    assert torch.equal(graw, rr.grad)


def test_lattice_distances_are_exact():
    """Squared distances on the {0..3}^3 lattice are small integers: exact in f32, many ties."""
    X, Y = H.lattice_points(257, 1), H.lattice_points(513, 2)
    d2 = ((X[:, :, None] - Y[:, None, :]) ** 2).sum(0)
    assert torch.equal(d2, d2.round()) and d2.max().item() <= 27
    first = d2.argmin(1)
    ties = (d2 == d2.gather(1, first[:, None])).sum(1)
    assert ties.max().item() > 1
