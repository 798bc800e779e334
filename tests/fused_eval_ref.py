"""The fp64 reference of the fused per-ray eval render (nerf_render_eval_fused, k_render_fused2 in
csrc/chain.hip) in plain torch on the CPU, from the pieces the suite already holds: the oracle's
sample depths and encodings, the chain's layer reference (helpers.chain_params /
chain_compose_fwd) and the composite reference (helpers.composite_ref).  Shared by
tests/test_fused_eval_reference_cpu.py (the reference is the oracle, the input conditions, the
mutants) and tests/test_gpu_fused_eval_fp64.py (the kernel).

Block geometry of the kernel, as constants here: a block holds ROWS = 128 rows = 128 / S rays; the
view encoding serves VIEW_PASS = 16 rays per pass and the composite COMP_PASS = 32."""
from __future__ import annotations

import copy
import functools
import math
from collections import namedtuple

import torch

from oracle import nerf_oracle as orc
from tests import helpers as H

ROWS, VIEW_PASS, COMP_PASS = 128, 16, 32
SAMPLE_COUNTS = (2, 4, 8, 16, 32, 64, 128)
VARIANTS = ("generic", "flat", "saturated")
MUTANTS = ("view2", "comp2", "view_is_d", "lvl9", "dz_back", "last_alpha", "no_white", "no_eps", "block0")
F_DIST_ALPHA, F_WHITE, F_RELU = 1, 2, 4
EPS = orc.EPS_COMPOSITE
SAT_RAW = 25.0          # saturated: softplus' x > 20 branch, and exp(-25) < 2^-25: alpha rounds to 1 in f32

Case = namedtuple("Case", "R S flags near far geom")


def case_name(c: Case) -> str:
    return f"S{c.S}-R{c.R}-f{c.flags}" + ("-geom" if c.geom else "")


def _cases():
    out = []
    for S in SAMPLE_COUNTS:
        nr = ROWS // S
        out.append(Case(nr, S, 0, 0.01, 10.0, False))               # exactly one block
        out.append(Case(nr + 1, S, 1, 0.01, 10.0, False))           # a second block holding one ray
        out += [Case(2 * nr + 1, S, f, 0.01, 10.0, False) for f in range(8)]
    out += [Case(17, 2, 0, 0.01, 10.0, False),      # one live ray in view pass 2
            Case(33, 2, 0, 0.01, 10.0, False),      # one in composite pass 2 / view pass 3
            Case(17, 4, 0, 0.01, 10.0, False),      # one live ray in view pass 2 at S = 4
            Case(5, 64, 0, 0.0, 1.0, True)]         # the geometry route: near = 0, far = 1, view = pts_d
    assert Case(1, 128, 0, 0.01, 10.0, False) in out      # R = 1 at S = 128 is that S's one-block case
    return tuple(out)


# The smallest shapes that reach each path: 74 cases of R S <= 256 + S rows (384 at S = 128), 18 902 rows
# in all, 56 706 over the three field variants.
CASES = _cases()
CASE_BY_NAME = {case_name(c): c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def case_rays(c: Case):
    """(o, d, view) [R][3] f32: origins in [-2, 2]^3, directions of length 0.5 .. 1.5 (not unit), and a
    unit view direction drawn independently of d -- except on the geometry route, where view = d.
    The same rays for every flag value of an (R, S)."""
    g = torch.Generator().manual_seed(7919 * c.S + c.R + (50000 if c.geom else 0))
    o = (torch.rand(c.R, 3, generator=g) - 0.5) * 4
    d = torch.nn.functional.normalize(torch.rand(c.R, 3, generator=g) - 0.5, dim=-1)
    u = torch.rand(c.R, 1, generator=g)
    d = d * torch.where(u < 0.5, 0.5 + 0.8 * u, 0.7 + 0.8 * u)      # lengths in [0.5, 0.9) and [1.1, 1.5)
    view = torch.nn.functional.normalize(torch.rand(c.R, 3, generator=g) - 0.5, dim=-1)
    return o, d, (d.clone() if c.geom else view)


def ray_slots(R: int, S: int):
    """-> (ray index [R], the slot of each ray in its block)."""
    ray = torch.arange(R)
    return ray, ray % (ROWS // S)


def _compose(params, heads, enc_p, enc_d, dtype):
    """raw4 [n][4] of the ten layers and both heads: helpers.chain_compose_fwd in fp64; at float32 the
    same layers in plain f32 arithmetic (chain_compose_fwd computes in fp64 whatever it is given)."""
    if dtype == torch.float64:
        return H.chain_compose_fwd(params, heads, enc_p, enc_d)[1]
    wd, bd, wc, bc = (t.to(dtype) for t in heads)
    x = h8 = enc_p
    for l, (W, b) in enumerate(params):
        xin = torch.cat([x, enc_p], 1) if l == 4 else torch.cat([x, enc_d], 1) if l == 9 else x
        pre = xin @ H._pad_cols(W, xin.shape[1]).to(dtype).t() + b.to(dtype)      # (the 64-wide encodings: zero pad columns)
        x = H.chain_act(l, pre)
        if l == 7:
            h8 = x
    return torch.cat([h8 @ wd.t() + bd, x @ wc.t() + bc], 1)


def composite(raw4, z, flags, dtype, _wrong=None):
    """helpers.composite_ref's forward written out, for the composite mutants (None: no mutant; the CPU
    test holds it equal to composite_ref) -> (rgb [R][3], dist [R], alpha [R][S])."""
    R, S = z.shape
    rr, zz = raw4.detach().to(dtype), z.detach().to(dtype)
    sig = torch.relu(rr[:, 0]) if flags & F_RELU else torch.nn.functional.softplus(rr[:, 0])
    sig = sig.view(R, S)
    c = torch.sigmoid(rr[:, 1:]).view(R, S, 3)
    if flags & F_DIST_ALPHA:
        if _wrong == "dz_back":      # z[i] - z[i - 1] in the flat z array (0 before the first row)
            zf = zz.reshape(-1)
            delta = (zf - torch.cat([zf.new_zeros(1), zf[:-1]])).view(R, S)
        else:
            delta = torch.cat([zz[:, 1:] - zz[:, :-1], zz.new_full((R, 1), 1e10)], 1)
        alpha = 1 - torch.exp(-1.0 * sig * delta)
        if _wrong == "last_alpha":
            alpha[:, -1] = 1 - torch.exp(-1.0 * sig[:, -1] * 1e10)
        else:
            alpha = torch.cat([alpha[:, :-1], torch.ones_like(alpha[:, -1:])], 1)
    else:
        alpha = 1 - torch.exp(-1.0 * sig)
    eps = 0.0 if _wrong == "no_eps" else EPS
    trans = torch.cumprod(torch.cat([alpha.new_ones(R, 1), 1.0 - alpha + eps], 1), 1)[:, :-1]
    w = alpha * trans
    rgb = (w.unsqueeze(-1) * c).sum(1)
    dist = (w * zz).sum(1)
    if flags & F_WHITE and _wrong != "no_white":
        rgb = rgb + (1.0 - w.sum(1)).unsqueeze(-1)
    return rgb, dist, alpha


COMPOSITE_MUTANTS = ("dz_back", "last_alpha", "no_white", "no_eps")


def fused_eval_ref(net, o, d, view, near, far, S, flags, dtype, _wrong=None):
    """The fused eval render of the rays (o, d, view) [R][3] f32 by the field `net` (CPU) at `dtype`
    -> (rgb [R][3], dist [R], alpha [R][S], z [R][S] f32, raw4 [R*S][4]).
    z: the oracle's stratified depths without noise, f32 (bit-exact: test_encode_samples_edges); the
    sample point o + d z in f32, multiply and add rounded separately (csrc/samples.hpp); everything
    after it at dtype: float64 is the truth, float32 the reference's own arithmetic.
    _wrong: one of MUTANTS -- the wrong kernels of tests/test_fused_eval_reference_cpu.py, nothing else."""
    assert _wrong is None or _wrong in MUTANTS, _wrong
    o, d, view = o.detach().cpu().float(), d.detach().cpu().float(), view.detach().cpu().float()
    R = o.shape[0]
    ray, slot = ray_slots(R, S)
    if _wrong == "block0":           # every block renders block 0's rays
        o, d, view = o[slot], d[slot], view[slot]
    z = orc.stratified_z(R, S, near, far, None)[0]
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(R * S, 3)
    vsrc = d if _wrong == "view_is_d" else view
    if _wrong == "view2":            # a ray in slot r >= 16 takes the view direction of slot r - 16
        vsrc = vsrc[torch.where(slot >= VIEW_PASS, ray - VIEW_PASS, ray)]
    enc_p = torch.cat([orc.encode_position(pts.to(dtype), 10), torch.zeros(R * S, 1, dtype=dtype)], 1)
    if _wrong == "lvl9":             # sin and cos of the last position level swapped
        enc_p = torch.cat([enc_p[:, :57], enc_p[:, 60:63], enc_p[:, 57:60], enc_p[:, 63:]], 1)
    enc_d = torch.cat([orc.encode_position(vsrc.to(dtype), 4), torch.zeros(R, 37, dtype=dtype)], 1)
    enc_d = enc_d[:, None, :].expand(R, S, 64).reshape(R * S, 64)
    params, heads = H.chain_params(net)
    raw4 = _compose(params, heads, enc_p, enc_d, dtype)
    if _wrong == "comp2":            # a ray in slot r >= 32 is composited from slot r - 32's samples
        raw4 = raw4.view(R, S, 4)[torch.where(slot >= COMP_PASS, ray - COMP_PASS, ray)].reshape(R * S, 4)
    if _wrong in COMPOSITE_MUTANTS:
        rgb, dist, alpha = composite(raw4, z, flags, dtype, _wrong)
    else:
        zero = torch.zeros(R, 3), torch.zeros(R)
        rgb, dist, alpha, _ = H.composite_ref(raw4, z, flags, *zero, dtype)
    return rgb, dist, alpha, z, raw4.detach()


def composite_of_alpha(alpha, z, colours, flags):
    """The fp64 composite of given final alphas [R][S] and depths with the colours [R][S][3]: what rgb
    and dist must be for THIS alpha (separates a colour error from a density error)."""
    rgb, dist, _, _ = orc.composite(alpha.detach().cpu().double(), colours.double(), z.detach().cpu().double().view_as(alpha),
                                    dist_alpha=False, white_background=bool(flags & F_WHITE))
    return rgb, dist


def scaled_tight_bar(e: float, ref) -> float:
    """helpers.tight_bar with its 4 ulp term scaled by max(1, max |ref|)."""
    m = max(1.0, float(ref.abs().max())) if torch.is_tensor(ref) else max(1.0, float(ref))
    return H.tight_bar(e) + 4 * H.U24 * (m - 1.0)


def max_err(a, ref64) -> float:
    return (a.detach().cpu().double().reshape(ref64.shape) - ref64).abs().max().item()


# ---- the field variants ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def generic_net():
    """helpers.chain_test_net as it is built (never modified: the variants are copies)."""
    return H.chain_test_net(0, "P1")


@functools.lru_cache(maxsize=None)
def _generic_raw0(R, S, near, far, geom):
    c = Case(R, S, 0, near, far, geom)
    raw4 = fused_eval_ref(generic_net(), *case_rays(c), near, far, S, 0, torch.float64)[4]
    return raw4[:, 0].view(R, S)


def _sat_gain(c: Case):
    """saturated: the power of two on the generic density weight -- 16 (the generic logit has a standard
    deviation near 1.6: alpha then runs from 0 to 1 along a ray), times 1 / delta rounded up to a
    power of two under dist_alpha (alpha = 1 - exp(-sigma delta))."""
    delta = (c.far - c.near) / (c.S - 1) if c.flags & F_DIST_ALPHA else 1.0
    return 16.0 * 2.0 ** max(0, math.ceil(math.log2(1.0 / delta))), delta


def _sat_logits(c: Case):
    """The weight part of the saturated variant's density logit, fp64 [R][S]."""
    b0 = generic_net().fc_density.bias.item()
    return _sat_gain(c)[0] * (_generic_raw0(c.R, c.S, c.near, c.far, c.geom) - b0)


def dead_rays(c: Case):
    """saturated under ReLU: the ceil(R / 2) rays with the lowest maximum of the density logit, whose
    every logit the bias takes below zero -> (bool [R], that bias, the margin: half the gap between
    the highest dead and the lowest live ray maximum)."""
    m = _sat_logits(c).amax(1)
    srt, k = torch.sort(m).values, (c.R + 1) // 2
    if k < c.R:
        cut, margin = 0.5 * (srt[k - 1] + srt[k]).item(), 0.5 * (srt[k] - srt[k - 1]).item()
    else:
        cut, margin = srt[-1].item() + 1.0, 1.0
    return m < cut, -cut, margin


FLAT_RGB_GAIN = 2.0 ** -11


def variant_heads(variant: str, c: Case):
    """(fc_density.weight [1][256], fc_density.bias [1], fc_rgb.weight [3][128], fc_rgb.bias [3]) f32 of
    a field variant for a case; the ten layers are generic_net()'s in every variant.
    flat: density weight 0 and the bias that gives every sample alpha = 1 / S (under dist_alpha every
    sample but the last, which the composite forces to 1); fc_rgb.weight times 2^-11 -- the generic
    colour logits have a standard deviation near 4000, every sigmoid is 0 or 1 and no colour depends
    on the view direction; scaled, they are of order 1.
    saturated: the generic density weight times _sat_gain and the bias that takes the largest logit
    of the least dense ray (its last sample aside) to SAT_RAW (SAT_RAW / delta under dist_alpha:
    sigma delta = SAT_RAW); under ReLU the bias that leaves half the rays (dead_rays) without a
    positive logit."""
    assert variant in VARIANTS, variant
    net = generic_net()
    w, b = net.fc_density.weight.detach().clone(), net.fc_density.bias.detach().clone()
    wc, bc = net.fc_rgb.weight.detach().clone(), net.fc_rgb.bias.detach().clone()
    if variant == "flat":
        delta = (c.far - c.near) / (c.S - 1) if c.flags & F_DIST_ALPHA else 1.0
        sigma = -math.log1p(-1.0 / c.S) / delta
        w.zero_()
        b.fill_(sigma if c.flags & F_RELU or sigma > 30 else math.log(math.expm1(sigma)))
        wc *= FLAT_RGB_GAIN
    elif variant == "saturated":
        gain, delta = _sat_gain(c)
        w *= gain
        if c.flags & F_RELU:
            b.fill_(dead_rays(c)[1])
        else:
            b.fill_(SAT_RAW * max(1.0, 1.0 / delta) - _sat_logits(c)[:, :-1].amax(1).min().item())
    return w, b, wc, bc


def variant_net(variant: str, c: Case):
    """A copy of generic_net() carrying the variant's heads."""
    net = copy.deepcopy(generic_net())
    w, b, wc, bc = variant_heads(variant, c)
    with torch.no_grad():
        net.fc_density.weight.copy_(w)
        net.fc_density.bias.copy_(b)
        net.fc_rgb.weight.copy_(wc)
        net.fc_rgb.bias.copy_(bc)
    return net


@functools.lru_cache(maxsize=None)
def case_refs(variant: str, c: Case):
    """(the fp64 truth, the f32 run of the reference) of a case and variant, each the tuple
    fused_eval_ref returns; computed once and never modified."""
    net = variant_net(variant, c)
    o, d, view = case_rays(c)
    return tuple(fused_eval_ref(net, o, d, view, c.near, c.far, c.S, c.flags, dt) for dt in (torch.float64, torch.float32))


def e_f32(variant: str, c: Case):
    """E_f32 per output: max |f32 reference - fp64 reference| of rgb, dist, alpha."""
    r64, r32 = case_refs(variant, c)
    return {n: max_err(r32[i], r64[i]) for i, n in enumerate(("rgb", "dist", "alpha"))}
