"""The fused per-ray eval render (nerf_render_eval_fused, k_render_fused2 in csrc/chain.hip) against the
fp64 reference of tests/fused_eval_ref.py, at every sample count and pass (GPU only, GEMM precision
mode 2, D = 256).

_hip.render_eval_fused is called directly, every output a helpers.Guarded buffer, on every case of
fused_eval_ref.CASES and each field variant (generic, flat, saturated: the ten layers are the same
packed field, the variants differ in the density / colour heads the entry takes as plain pointers).

The bar is measured, per case and output, against the path that is already pinned layer by layer
(tests/test_gpu_chain_fp64.py, test_gpu_ray_kernels_fp64.py): the staged two-wave path
nerf_encode_samples (no noise) -> nerf_mlp_chain_frozen -> nerf_composite_fwd on the same inputs.
With e_staged its error against fp64 and E_f32 the CPU f32 reference's,
    e_fused <= helpers.tight_bar(max(e_staged, E_f32)),  the 4 ulp scaled by max(1, max |ref|)
-- the 1.5 is the project's allowance for another summation order and leaves no room for a wrong tap
(tests/test_fused_eval_reference_cpu.py: every mutant is over 10 x that bar on its case).  The
ratios e_fused / max(e_staged, E_f32) go through helpers.report_err and are tabled in DESIGN.md."""
import copy

import pytest
import torch

from model import _hip
from tests import fused_eval_ref as F
from tests import helpers as H

pytestmark = pytest.mark.gpu

NAMES = ("rgb", "dist", "alpha")
OUTS = ("rgb", "dist", "alpha", "z")
_STATE, _RUNS = {}, {}


@pytest.fixture(autouse=True)
def h16(dev):
    old = _hip.gemm_get_precision()
    _hip.gemm_set_precision(2)
    yield
    _hip.gemm_set_precision(old)


def _field(dev):
    """fused_eval_ref.generic_net() packed on the device, once."""
    if "runner" not in _STATE:
        net = copy.deepcopy(F.generic_net()).to(dev)
        runner = net.hip_runner()
        runner.pack()
        torch.cuda.synchronize()
        _STATE.update(net=net, runner=runner)
    return _STATE["runner"]


def _fused(dev, heads, o, d, view, c):
    """One launch of the entry into guarded outputs -> {name: Guarded}."""
    runner, none = _field(dev), [None] * 10
    G = dict(rgb=H.Guarded((c.R, 3), dev), dist=H.Guarded((c.R,), dev), alpha=H.Guarded((c.R, c.S), dev),
             z=H.Guarded((c.R * c.S,), dev))
    _hip.render_eval_fused(o, d, view, c.R, c.S, c.near, c.far, c.flags, H.chain_descs(runner, none, none, none), *heads,
                           G["rgb"].t, G["dist"].t, G["alpha"].t, G["z"].t)
    torch.cuda.synchronize()
    return G


def _staged(dev, heads, o, d, view, c):
    """nerf_encode_samples (no noise) -> nerf_mlp_chain_frozen -> nerf_composite_fwd -> (rgb, dist, alpha, z)."""
    runner, none = _field(dev), [None] * 10
    R, S = c.R, c.S
    Np = -(-R * S // F.ROWS) * F.ROWS
    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)      # noqa: E731
    z, ep, ed, rp, rd, raw4 = e(Np), e(Np, 64), e(Np, 64), e(Np), e(Np), e(Np, 4)
    _hip.encode_samples(o, d, view, None, R, S, Np, c.near, c.far, z, ep, ed, enc_p_rmax=rp, enc_d_rmax=rd)
    masks = [torch.zeros(Np, l.out_p // 32, device=dev, dtype=torch.int32) if l.relu else None for l in runner.layers]
    _hip.mlp_chain_frozen(ep, ed, rp, rd, Np, H.chain_descs(runner, none, masks, none), *heads, raw4)
    rgb, dist, alpha = e(R, 3), e(R), e(R, S)
    _hip.composite_fwd(raw4, z, R, S, c.flags, rgb, dist, alpha)
    torch.cuda.synchronize()
    return rgb, dist, alpha, z[:R * S]


def _heads(dev, variant, c):
    return tuple(t.to(dev).contiguous() for t in F.variant_heads(variant, c))


def _run(dev, variant, c):
    """The fused and the staged render of one case and variant, once: CPU copies of the outputs, the
    state of the guards and of the payloads right after the launch."""
    key = (variant, c)
    if key not in _RUNS:
        heads = _heads(dev, variant, c)
        o, d, view = (t.to(dev) for t in F.case_rays(c))
        G = _fused(dev, heads, o, d, view, c)
        st = _staged(dev, heads, o, d, view, c)
        run = dict(fused={n: G[n].t.cpu().clone() for n in OUTS}, staged=dict(zip(OUTS, (t.cpu() for t in st))),
                   intact={n: G[n].intact() for n in OUTS},
                   written={n: bool((G[n].t != H.SENT).all()) and bool(torch.isfinite(G[n].t).all()) for n in OUTS})
        _RUNS[key] = run
    return _RUNS[key]


def _errors(variant, c, out):
    """Errors of (rgb, dist, alpha, z) `out` against the fp64 truth, and of rgb / dist against the fp64
    composite of out's OWN alpha and z with the fp64 colours (a colour error apart from a density error)."""
    r64 = F.case_refs(variant, c)[0]
    e = {n: F.max_err(out[n], r64[i]) for i, n in enumerate(NAMES)}
    colours = torch.sigmoid(r64[4][:, 1:]).view(c.R, c.S, 3)
    rgb_a, dist_a = F.composite_of_alpha(out["alpha"].view(c.R, c.S), out["z"], colours, c.flags)
    e["rgb|alpha"], e["dist|alpha"] = F.max_err(out["rgb"], rgb_a), F.max_err(out["dist"], dist_a)
    return e


@pytest.mark.parametrize("S", F.SAMPLE_COUNTS)
@pytest.mark.parametrize("variant", F.VARIANTS)
def test_accuracy_against_fp64(dev, variant, S):
    """alpha, rgb and dist of every case with this S against the fp64 truth, and rgb and dist against
    the fp64 composite of the kernel's own alpha and z, under tight_bar(max(e_staged, E_f32)); z
    bit-equal to the reference."""
    test = "test_fused_eval_accuracy"
    fails, worst = [], {}
    for c in (c for c in F.CASES if c.S == S):
        name = F.case_name(c)
        run = _run(dev, variant, c)
        r64, r32 = F.case_refs(variant, c)
        ref32 = dict(rgb=r32[0], dist=r32[1], alpha=r32[2], z=r64[3])
        e_f, e_s, e_32 = (_errors(variant, c, o) for o in (run["fused"], run["staged"], ref32))
        if not torch.equal(run["fused"]["z"].view(c.R, c.S), r64[3]):
            fails.append(f"{variant} {name}: z differs from the reference")
        refs = {"rgb": r64[0], "dist": r64[1], "alpha": r64[2], "rgb|alpha": r64[0], "dist|alpha": r64[1]}
        line = []
        for n, ref in refs.items():
            base = max(e_s[n], e_32[n])
            bar = F.scaled_tight_bar(base, ref)
            ratio = 0.0 if e_f[n] == 0 else e_f[n] / max(base, 1e-300)
            worst[n] = max(worst.get(n, 0.0), H.report_err(test, f"{variant} {name} {n} e_fused/max(e_staged,E_f32)", ratio))
            line.append(f"{n} {e_f[n]:.2e} (staged {e_s[n]:.2e}, E_f32 {e_32[n]:.2e}, ratio {ratio:.2f})")
            if e_f[n] > bar:
                fails.append(f"{variant} {name}: {n}: e_fused {e_f[n]:.3e} > 1.5 x max(e_staged {e_s[n]:.3e}, "
                             f"E_f32 {e_32[n]:.3e}) + 4 ulp")
        print(f"{variant} {name}: " + "; ".join(line))
    print(f"{variant} S={S}: worst ratio " + ", ".join(f"{n} {r:.2f}" for n, r in worst.items()))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("variant", F.VARIANTS)
def test_bit_identical_to_the_staged_path(dev, variant):
    """The composite has the arithmetic of k_composite16_fwd and the chain body is the template of
    nerf_mlp_chain_frozen; the samples and encodings are those of nerf_encode_samples: all four outputs
    of every case equal the staged path's bit for bit."""
    differ = []
    for c in F.CASES:
        run = _run(dev, variant, c)
        for n in OUTS:
            a, b = run["fused"][n].reshape(-1), run["staged"][n].reshape(-1)
            if not torch.equal(a, b):
                differ.append(f"{variant} {F.case_name(c)}: {n}: {int((a != b).sum())} of {a.numel()} elements differ, "
                              f"max |diff| {float((a - b).abs().max()):.3e}")
    print(f"{variant}: {len(F.CASES)} cases, {len(differ)} outputs differ from the staged path")
    assert not differ, "\n".join(differ)


@pytest.mark.parametrize("variant", F.VARIANTS)
def test_guards_and_payloads(dev, variant):
    """After every launch the sentinels before and after rgb, dist, alpha and z are intact (the ragged
    last block, the float4 alpha stores, the z tail store), and every payload element is written:
    none still holds the sentinel, all are finite."""
    fails = []
    for c in F.CASES:
        run = _run(dev, variant, c)
        fails += [f"{variant} {F.case_name(c)}: wrote outside {n}" for n in OUTS if not run["intact"][n]]
        fails += [f"{variant} {F.case_name(c)}: {n} not wholly written or not finite" for n in OUTS if not run["written"][n]]
    assert not fails, "\n".join(fails)


# S -> the numbers of rays prepended (none a multiple of the 128 / S rays of a block, but at S = 128,
# where a block is one ray and every shift is a whole block): 17 and 33 move a ray of S = 2 across
# the view passes (16 rays) and the composite passes (32)
SHIFTS = {2: (17, 33), 4: (17,), 16: (3,), 128: (1,)}


@pytest.mark.parametrize("S", sorted(SHIFTS))
def test_result_is_independent_of_block_and_slot(dev, S):
    """A ray list rendered alone and behind k extra rays: every original ray's rgb, dist, alpha row
    and z row bit-identical, whatever block and slot it lands in.  Rendered with the generic field,
    whose density depends on the ray: at flags = 0 the kernel's own rgb, dist and alpha rows are
    asserted pairwise different between all rays, so any wrong ray or slot index moves each of them
    (z carries no noise and is the same row for every ray: its comparison only shows the store landed
    where it belongs).  flat (one alpha row for every ray, colours of order 1) is an extra for rgb."""
    nr = F.ROWS // S
    for variant, flags in (("generic", 0), ("generic", 3), ("flat", 0), ("flat", 3)):
        c0 = F.Case(2 * nr + 1, S, flags, 0.01, 10.0, False)
        heads = _heads(dev, variant, c0)
        rays0 = F.case_rays(c0)
        base = _fused(dev, heads, *(t.to(dev) for t in rays0), c0)
        distinct = {n: int(torch.unique(base[n].t.reshape(c0.R, -1), dim=0).shape[0]) for n in NAMES}
        print(f"S={S} {variant} flags={flags}: distinct rows among {c0.R} rays: {distinct}")
        if variant == "generic" and flags == 0:
            assert all(v == c0.R for v in distinct.values()), distinct
        for k in SHIFTS[S]:
            assert k % nr != 0 or nr == 1
            c1 = c0._replace(R=c0.R + k)
            extra = F.case_rays(F.Case(k, S, flags, 0.01, 10.0, True))      # k other rays (the geom seed offset)
            rays1 = tuple(torch.cat([x, t]).to(dev) for x, t in zip(extra, rays0))
            got = _fused(dev, heads, *rays1, c1)
            for n in OUTS:
                assert got[n].intact(), (S, variant, flags, k, n)
                a = got[n].t.reshape(c1.R, -1)[k:]
                assert torch.equal(a, base[n].t.reshape(c0.R, -1)), f"S={S} {variant} flags={flags} k={k}: {n} moved with the slot"
            assert bool((base["rgb"].t != H.SENT).all())


@pytest.mark.parametrize("S", F.SAMPLE_COUNTS)
def test_two_launches_give_the_same_bits(dev, S):
    c = F.Case(2 * (F.ROWS // S) + 1, S, 7, 0.01, 10.0, False)
    assert c in F.CASES
    heads = _heads(dev, "generic", c)
    rays = tuple(t.to(dev) for t in F.case_rays(c))
    a, b = _fused(dev, heads, *rays, c), _fused(dev, heads, *rays, c)
    for n in OUTS:
        assert torch.equal(a[n].t, b[n].t), (S, n)


@pytest.mark.parametrize("variant", F.VARIANTS)
def test_exact_values(dev, variant):
    """dist_alpha: the last alpha of every ray is exactly 1.  saturated under ReLU: on the dead rays
    (every density logit below zero) alpha is exactly 0 -- before the forced last one under
    dist_alpha -- and, without dist_alpha, rgb is exactly the background (0, or 1 with the
    white-background flag) and dist exactly 0."""
    n_dead = 0
    for c in F.CASES:
        out = _run(dev, variant, c)["fused"]
        alpha = out["alpha"].view(c.R, c.S)
        if c.flags & F.F_DIST_ALPHA:
            assert bool((alpha[:, -1] == 1.0).all()), F.case_name(c)
        if variant == "saturated" and c.flags & F.F_RELU:
            dead = F.dead_rays(c)[0]
            n_dead += int(dead.sum())
            body = slice(0, c.S - 1) if c.flags & F.F_DIST_ALPHA else slice(None)
            assert bool((alpha[dead][:, body] == 0.0).all()), F.case_name(c)
            if not c.flags & F.F_DIST_ALPHA:
                bg = 1.0 if c.flags & F.F_WHITE else 0.0
                assert bool((out["rgb"][dead] == bg).all()) and bool((out["dist"][dead] == 0.0).all()), F.case_name(c)
    assert variant != "saturated" or n_dead > 0
