"""Torch restatements of the per-ray rules of the geometry visualisation (csrc/march.hip), taken
from Renderer.ray_marching / Renderer.secant / get_sphere_intersection, dense over the rays and
in the dtype of their inputs (f32 as the reference runs, f64 as the yardstick), plus three
deliberately wrong select rules that the edge rows must tell apart from the right one."""
from __future__ import annotations

import math

import torch

NONE, BRACKET, INSIDE = 0, 1, 2


def ulp32(x):
    """Spacing of f32 at the magnitude of x (f64 tensor or float): 2^(floor(log2 |x|) - 23), the
    subnormal spacing 2^-149 at and near zero."""
    x = torch.as_tensor(x, dtype=torch.float64).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)


def d_proposal(d_far, d0, n, dtype):
    """d(j) = d0 (1 - t_j) + d_far t_j, t = linspace(0, 1, n) -> [R][n] (ray_marching's d_prop)."""
    t = torch.linspace(0, 1, steps=n, dtype=dtype).view(1, n)
    return d0 * (1.0 - t) + d_far.to(dtype).view(-1, 1) * t


def select_ref(occ, d_far, d0, tau, d_dtype=None, _wrong=None):
    """Renderer.ray_marching's selection (rendering.py:137-147), dense: occ [R][n] ->
    (state [R] uint8, f_low, f_high, d_low, d_high [R]).  val = occ - tau and its products are
    formed in occ's dtype; the distances in d_dtype (default: occ's).  f / d are 0 off state 1.
    _wrong: 'neg_to_pos' takes the first negative-to-positive change instead of the first change;
    'no_product' tests val[j] < 0 < val[j+1] without forming the product; 'no_first' drops the
    val[0] rule."""
    R, n = occ.shape
    d_dtype = d_dtype or occ.dtype
    val = occ - tau
    mask_0_not_occ = val[:, 0] < 0
    if _wrong == "no_product":
        change = (val[:, :-1] < 0) & (val[:, 1:] > 0)
        sign = torch.where(change, -torch.ones_like(val[:, :-1]), torch.ones_like(val[:, :-1]))
    else:
        sign = torch.sign(val[:, :-1] * val[:, 1:])
        if _wrong == "neg_to_pos":
            sign = torch.where((sign < 0) & ~(val[:, :-1] < 0), torch.ones_like(sign), sign)
    sign = torch.cat([sign, torch.ones(R, 1, dtype=val.dtype)], -1)
    cost = sign * torch.arange(n, 0, -1, dtype=val.dtype)
    values, idx = torch.min(cost, -1)
    mask_sign_change = values < 0
    take = lambda a, i: torch.gather(a, 1, i.unsqueeze(-1)).squeeze(-1)   # noqa: E731
    mask_neg_to_pos = take(val, idx) < 0
    mask = mask_sign_change & mask_neg_to_pos & mask_0_not_occ
    if _wrong == "no_first":
        mask = mask_sign_change & mask_neg_to_pos
    idx_h = torch.clamp(idx + 1, max=n - 1)
    dp = d_proposal(d_far, d0, n, d_dtype)
    zf, zd = torch.zeros(R, dtype=val.dtype), torch.zeros(R, dtype=d_dtype)
    f_low, f_high = torch.where(mask, take(val, idx), zf), torch.where(mask, take(val, idx_h), zf)
    d_low, d_high = torch.where(mask, take(dp, idx), zd), torch.where(mask, take(dp, idx_h), zd)
    state = torch.where(mask, BRACKET, NONE)
    if _wrong != "no_first":
        state = torch.where(mask_0_not_occ, state, INSIDE)
    return state.to(torch.uint8), f_low, f_high, d_low, d_high


def secant_pred(f_low, f_high, d_low, d_high):
    """rendering.py:415 / :434."""
    return -f_low * (d_high - d_low) / (f_high - f_low) + d_low


def secant_update(f_low, f_high, d_low, d_high, d_pred, f_mid):
    """One pass of Renderer.secant's loop body after f_mid is known (rendering.py:428-434) ->
    (f_low, f_high, d_low, d_high, d_pred)."""
    low = f_mid < 0
    d_low = torch.where(low, d_pred, d_low)
    f_low = torch.where(low, f_mid, f_low)
    d_high = torch.where(low, d_high, d_pred)
    f_high = torch.where(low, f_high, f_mid)
    return f_low, f_high, d_low, d_high, secant_pred(f_low, f_high, d_low, d_high)


def density_ref(raw, relu, dist_alpha):
    """OfficialStaticNerf._density in raw's dtype."""
    sigma = raw.relu() if relu else torch.nn.functional.softplus(raw)
    return sigma if dist_alpha else 1 - torch.exp(-1.0 * sigma)


def sphere_far(cam0, ray, rad):
    """get_sphere_intersection's far root for c = cam0 [3], ray [R][3] -> (d_far [R], u [R])."""
    b = ray @ cam0
    u = b ** 2 - (cam0.norm(2) ** 2 - rad ** 2)
    d_far = torch.where(u > 0, (torch.sqrt(u.clamp_min(0)) - b).clamp_min(0), torch.zeros_like(u))
    return d_far, u


def proposal_points(cam, ray, d_far, d0, n):
    """ray_marching's p_proposal [R][n][3] in cam's dtype."""
    d = d_proposal(d_far, d0, n, cam.dtype)
    return cam.unsqueeze(1) + ray.unsqueeze(1) * d.unsqueeze(-1)


def march_rays_ref(cam, ray, rad, d0, n, seg):
    """nerf_march_rays as include/nerf_hip.h states it: d_far in f64 from the f32 inputs, rounded to
    f32; the pseudo-rays in f64 from the rounded d_far, rounded to f32 -> (d_far [R], o_seg, d_seg
    [R][G][3]) in f32."""
    c64, r64 = cam.double(), ray.double()
    d_far = sphere_far(c64[0], r64, float(rad))[0].float()
    G = n // seg
    span = (d_far.double() - d0).view(-1, 1, 1)
    g = torch.arange(G, dtype=torch.float64).view(1, G, 1)
    a = d0 + span * (g * seg) / (n - 1)
    o_seg = c64.unsqueeze(1) + r64.unsqueeze(1) * a
    d_seg = (r64.unsqueeze(1) * (span * (seg - 1) / (n - 1))).expand(-1, G, -1)
    return d_far, o_seg.float(), d_seg.float().contiguous()


def segment_points(o_seg, d_seg, seg, dtype):
    """The samples the render kernels take on the pseudo-rays (near 0, far 1, seg samples):
    o + d linspace(0, 1, seg), in dtype -> [R][G * seg][3]."""
    t = torch.linspace(0, 1, steps=seg, dtype=dtype).view(1, 1, seg, 1)
    p = o_seg.to(dtype).unsqueeze(2) + d_seg.to(dtype).unsqueeze(2) * t
    return p.reshape(p.shape[0], -1, 3)


# ---- edge rows of the select rule ---------------------------------------------------------------------------
def select_edge_rows(n):
    """{name: val row [n]} (f32; to be used with tau = 0, so occ = val exactly): the patterns that fit n
    samples, padded by repeating their last value (which adds no change)."""
    tiny, sub = 1e-30, 1e-20       # tiny^2 underflows to -0 in f32; sub^2 = 1e-40 is a subnormal
    pats = {
        "last_pair": [-1.0] * (n - 1) + [1.0],
        "all_negative": [-1.0, -0.5],
        "first_zero_later_change": [0.0, -1.0, 1.0],
        "first_positive_later_change": [1.0, -1.0, 1.0],
        "zero_product": [-1.0, 0.0, 1.0],
        "zero_then_change": [-1.0, 0.0, -1.0, 1.0],
        "first_change_wrong_way": [-1.0, 0.0, 1.0, -1.0],
        "wrong_way_then_right": [-1.0, 0.0, 1.0, -1.0, 1.0],
        "underflow_pair": [-tiny, tiny],
        "underflow_then_change": [-tiny, tiny, -1.0, 1.0],
        "subnormal_product": [-sub, sub],
        "first_pair": [-1.0, 1.0],
        "nan_product": [-1.0, float("nan"), -1.0, 1.0],      # torch.sign(nan) is 0: no change at the pair
    }
    rows = {}
    for name, p in pats.items():
        if len(p) <= n:
            rows[name] = torch.tensor(p + [p[-1]] * (n - len(p)), dtype=torch.float32)
    return rows


def select_case(n, R, tau, seed=0):
    """(occ [R][n] f32, d_far [R] f32, names): tau == 0 puts the edge rows first (row 0 the change in the
    last pair), then generic rows; one bracket row has d_far == 0."""
    g = torch.Generator().manual_seed(seed + 1000 * n + R)
    mag = 0.05 + torch.rand(R, n, generator=g)
    k = torch.randint(0, 2 * n, (R, 1), generator=g)             # k >= n: the row never changes
    sgn = torch.where(torch.arange(n).view(1, n) < k, -1.0, 1.0)
    flip = torch.rand(R, 1, generator=g) < 0.15                  # some rows start occupied
    val = (mag * sgn * torch.where(flip, -1.0, 1.0)).float()
    names = []
    if tau == 0:
        for i, (name, row) in enumerate(select_edge_rows(n).items()):
            if i < R:
                val[i] = row
                names.append(name)
        occ = val
    else:
        occ = (0.45 * val + tau).float()                         # occupancies inside (0, 1)
    d_far = (0.5 + 5.5 * torch.rand(R, generator=g)).float()
    d_far[min(R - 1, 5)] = 0.0                                   # 'zero_then_change' when it is there
    return occ.contiguous(), d_far, names


OCTA_LEVEL_DIST_ALPHA = (3.0 - math.log(math.exp(0.5) - 1.0)) / 5.0   # softplus(3 - 5 s) = 0.5
