"""The fp64 reference of the fused eval render (tests/fused_eval_ref.py) checked on the CPU: it is the
oracle's field and composite; the cases of CASES keep the input conditions they were built for; and
every wrong kernel of MUTANTS is told from the truth, on a named case, by more than ten times the
part of the GPU bar that is known without a GPU (tests/test_gpu_fused_eval_fp64.py)."""
import math

import pytest
import torch

from oracle import nerf_oracle as orc
from tests import fused_eval_ref as F
from tests import helpers as H

# the kernel's pass sizes, written out here: rays per pass of the view encoding and of the composite
VIEW_PASS, COMP_PASS, BLOCK_ROWS = 16, 32, 128
NAMES = ("rgb", "dist", "alpha")


def _oracle(net, c, dtype):
    """OracleNerf + orc.composite on the reference's own f32 sample points."""
    o, d, view = F.case_rays(c)
    ref = orc.OracleNerf(hidden_dim=256, white_background=bool(c.flags & 2), dist_alpha=bool(c.flags & 1),
                         occ_activation="relu" if c.flags & 4 else "softplus").to(dtype)
    ref.load_state_dict({k: v.to(dtype) for k, v in net.state_dict().items()})
    z = orc.stratified_z(c.R, c.S, c.near, c.far, None)[0]
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).to(dtype)
    with torch.no_grad():
        rgb_s, a_s = ref(pts, view[:, None, :].expand(c.R, c.S, 3).reshape(-1, 3).to(dtype))
        return orc.composite(a_s.reshape(c.R, c.S), rgb_s.reshape(c.R, c.S, 3), z.to(dtype), dist_alpha=bool(c.flags & 1),
                             white_background=bool(c.flags & 2))[:3]


ORACLE_ULP = 16      # |f32 reference - f32 oracle| in ulp of max(1, max |ref|), see test_reference_is_the_oracle


@pytest.mark.parametrize("variant", F.VARIANTS)
def test_reference_is_the_oracle(variant):
    """Every case, every output, against OracleNerf + orc.composite on the same inputs:
      * the fp64 reference is the fp64 oracle to 1e-12 (the same operations);
      * the f32 reference is the f32 oracle to the oracle's own rounding, ORACLE_ULP = 16 ulp of
        max(1, max |ref|): the two f32 runs do the same operations and differ only in the summation
        order inside the three matmuls whose input the reference pads or concatenates itself and in
        the heads; 16 ulp is what helpers.pair_ceiling allows an epilogue;
      * the fp64 reference equals the f32 oracle to E_f32, and E_f32 is no larger than the oracle's own
        f32 error e_orc: each within helpers.tight_bar of the other (1.5 x + 4 ulp scaled, the
        project's allowance for another summation order).  E_f32 is the yardstick of every GPU bar:
        a careless f32 path of the reference would inflate it, and fails here."""
    worst = dict(direct=0.0, e_orc=0.0, E_f32=0.0)
    for c in F.CASES:
        net = F.variant_net(variant, c)
        r64, r32 = F.case_refs(variant, c)
        e32 = F.e_f32(variant, c)
        o64, o32 = _oracle(net, c, torch.float64), _oracle(net, c, torch.float32)
        for i, n in enumerate(NAMES):
            where = (F.case_name(c), n)
            scale = max(1.0, r64[i].abs().max().item())
            assert r32[i].dtype == torch.float32 and o32[i].dtype == torch.float32
            assert F.max_err(o64[i], r64[i]) <= 1e-12 * scale, where
            direct = F.max_err(r32[i], o32[i].double()) / (H.U24 * scale)
            e_orc = F.max_err(o32[i], r64[i])
            worst["direct"] = max(worst["direct"], direct)
            worst["e_orc"] = max(worst["e_orc"], e_orc / F.scaled_tight_bar(e32[n], scale))
            worst["E_f32"] = max(worst["E_f32"], e32[n] / F.scaled_tight_bar(e_orc, scale))
            assert direct <= ORACLE_ULP, (where, direct)
            assert e_orc <= F.scaled_tight_bar(e32[n], scale), (where, e_orc, e32[n])
            assert e32[n] <= F.scaled_tight_bar(e_orc, scale), (where, e32[n], e_orc)
        assert torch.equal(r64[3], orc.stratified_z(c.R, c.S, c.near, c.far, None)[0]) and r64[3].dtype == torch.float32
    print(f"{variant}: |f32 reference - f32 oracle| <= {worst['direct']:.2f} ulp; e_orc / tight_bar(E_f32) <= "
          f"{worst['e_orc']:.2f}; E_f32 / tight_bar(e_orc) <= {worst['E_f32']:.2f}")


def test_written_out_composite_is_composite_ref():
    """fused_eval_ref.composite without a mutant is helpers.composite_ref's forward, at every flag
    value: each composite mutant is one edit away from the reference."""
    raw, z, g_rgb, g_dist = H.composite_edge_inputs(7, 16, 3, "saturated")
    for flags in range(8):
        for dt in (torch.float64, torch.float32):
            want = H.composite_ref(raw, z, flags, g_rgb, g_dist, dt)[:3]
            got = F.composite(raw, z, flags, dt)
            for a, b in zip(got, want):
                assert torch.equal(a, b), (flags, dt)


def test_cases_cover_what_they_were_built_for():
    """The case list itself: every S with one block, a second block of one ray and 2 blocks + 1 ray
    at all eight flag values; a live ray in every view and composite pass at S = 2 and S = 4, the
    single-ray passes of the extra cases; the geometry route's settings; under 100k rows in all."""
    by_s = {S: [c for c in F.CASES if c.S == S and not c.geom] for S in F.SAMPLE_COUNTS}
    for S, cs in by_s.items():
        nr = BLOCK_ROWS // S
        Rs = {c.R for c in cs}
        assert {nr, nr + 1, 2 * nr + 1} <= Rs, S
        assert {c.flags for c in cs if c.R == 2 * nr + 1} == set(range(8)), S
    passes = lambda R, S, per: sorted({(r % (BLOCK_ROWS // S)) // per for r in range(R)})      # noqa: E731
    for S in (2, 4):
        nr = BLOCK_ROWS // S
        for c in by_s[S]:
            if c.R >= nr:
                assert passes(c.R, S, VIEW_PASS) == list(range(nr // VIEW_PASS)), F.case_name(c)
                assert passes(c.R, S, COMP_PASS) == list(range(-(-nr // COMP_PASS))), F.case_name(c)
    assert VIEW_PASS == F.VIEW_PASS and COMP_PASS == F.COMP_PASS and BLOCK_ROWS == F.ROWS
    # the extra cases: exactly one live ray in the last pass they reach
    for name, per, last in (("S2-R17-f0", VIEW_PASS, 1), ("S2-R33-f0", COMP_PASS, 1), ("S2-R33-f0", VIEW_PASS, 2),
                            ("S4-R17-f0", VIEW_PASS, 1)):
        c = F.CASE_BY_NAME[name]
        assert c.R < BLOCK_ROWS // c.S
        assert passes(c.R, c.S, per)[-1] == last and sum(1 for r in range(c.R) if r // per == last) == 1, name
    geom = [c for c in F.CASES if c.geom]
    assert len(geom) == 1 and (geom[0].near, geom[0].far) == (0.0, 1.0)
    o, d, view = F.case_rays(geom[0])
    assert torch.equal(view, d)
    for c in F.CASES:
        o, d, view = F.case_rays(c)
        assert (d.norm(dim=1) - 1).abs().min().item() > 1e-3, F.case_name(c)      # no unit direction
        if not c.geom:
            assert (view - d).abs().amax(1).min().item() > 1e-2, F.case_name(c)   # view is not d
    rows = sum(c.R * c.S for c in F.CASES)
    print(f"{len(F.CASES)} cases, {rows} rows, largest {max(c.R * c.S for c in F.CASES)}")
    assert len(F.VARIANTS) * rows < 100_000


def test_flat_weights_lie_within_a_factor_e():
    """flat: the fp64 compositing weights' max / min ratio is <= e on every ray of every case, so one
    sample's wrong colour moves rgb by at least 1 / (e S) of the colour error.  Under dist_alpha the
    composite forces the last alpha to 1 whatever the field says (its weight is the whole remaining
    transmittance, up to S / e times the others): the ratio is taken over the samples before it, and
    the last weight is the largest."""
    for c in F.CASES:
        rgb, dist, alpha, z, raw4 = F.case_refs("flat", c)[0]
        trans = torch.cumprod(torch.cat([alpha.new_ones(c.R, 1), 1.0 - alpha + F.EPS], 1), 1)[:, :-1]
        w = alpha * trans
        if c.flags & F.F_DIST_ALPHA:
            assert bool((w[:, -1:] >= w[:, :-1]).all()), F.case_name(c)
            w = w[:, :-1]
        ratio = (w.amax(1) / w.amin(1)).max().item()
        assert ratio <= math.e, (F.case_name(c), ratio)
        # and the colours are not saturated: the colour logits are of order 1
        assert raw4[:, 1:].abs().max().item() < 30 and raw4[:, 1:].std().item() > 0.3, F.case_name(c)


def test_saturated_reaches_alpha_one_and_alpha_zero():
    """saturated, on the f32 run of the reference.  softplus: every ray has a sample (not the last,
    which dist_alpha forces) whose logit is past softplus' x > 20 branch and whose f32 alpha == 1.
    ReLU: at least a quarter of the samples have alpha == 0 -- the dead rays, whose largest logit is
    below zero by a margin of at least 64 times the f32 reference's own error of the logit."""
    for c in F.CASES:
        r64, r32 = F.case_refs("saturated", c)
        alpha32, raw32 = r32[2], r32[4][:, 0].view(c.R, c.S)
        assert alpha32.dtype == torch.float32
        body = slice(0, c.S - 1) if c.flags & F.F_DIST_ALPHA else slice(None)
        if c.flags & F.F_RELU:
            dead, _, margin = F.dead_rays(c)
            e_raw = F.max_err(r32[4][:, 0], r64[4][:, 0])
            assert margin >= 64 * e_raw, (F.case_name(c), margin, e_raw)
            assert int(dead.sum()) == (c.R + 1) // 2
            assert bool((r64[4][:, 0].view(c.R, c.S)[dead] < -margin / 2).all()) and bool((raw32[dead] < 0).all())
            assert bool((alpha32[dead][:, body] == 0).all()), F.case_name(c)
            assert int((alpha32[:, body] == 0).sum()) >= c.R * c.S / 4, F.case_name(c)
        else:
            hit = (alpha32[:, body] == 1) & (raw32[:, body] > 20)
            assert bool(hit.any(1).all()), F.case_name(c)


# mutant -> (variant, case) that catches it
CATCHES = {
    "view2": ("flat", "S2-R17-f0"),
    "comp2": ("flat", "S2-R33-f0"),
    "view_is_d": ("flat", "S8-R33-f0"),
    "lvl9": ("generic", "S8-R33-f0"),
    "dz_back": ("flat", "S16-R17-f1"),
    "last_alpha": ("saturated", "S16-R17-f5"),
    "no_white": ("flat", "S16-R17-f2"),
    "no_eps": ("flat", "S128-R3-f0"),
    "block0": ("flat", "S32-R9-f0"),
}


def mutant_ratios(variant, c, mutant):
    """max |mutant's fp64 output - truth| / tight_bar(E_f32) (4 ulp scaled by max(1, max |ref|)) per output."""
    r64, _ = F.case_refs(variant, c)
    e32 = F.e_f32(variant, c)
    got = F.fused_eval_ref(F.variant_net(variant, c), *F.case_rays(c), c.near, c.far, c.S, c.flags, torch.float64,
                           _wrong=mutant)
    return {n: F.max_err(got[i], r64[i]) / F.scaled_tight_bar(e32[n], r64[i]) for i, n in enumerate(NAMES)}


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_mutant_is_caught(mutant):
    """The mutant's fp64 output differs from the truth, on its catching case, by more than 10 x the
    CPU-known part of the GPU bar (tight_bar(E_f32); the GPU bar is tight_bar(max(e_staged, E_f32)))."""
    variant, name = CATCHES[mutant]
    c = F.CASE_BY_NAME[name]
    ratios = mutant_ratios(variant, c, mutant)
    print(f"{mutant}: {variant} {name}: " + ", ".join(f"{n} {r:.1f} x the bar" for n, r in ratios.items()))
    assert max(ratios.values()) > 10.0, (mutant, ratios)


def test_every_mutant_has_a_catching_case():
    assert set(CATCHES) == set(F.MUTANTS)
    assert all(v in F.VARIANTS and n in F.CASE_BY_NAME for v, n in CATCHES.values())
