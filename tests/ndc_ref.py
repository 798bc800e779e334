"""Staged reference of the NDC ray warp (nerf_ndc_rays / nerf_ndc_rays_bwd, csrc/rays.hip): the
expressions of common.py:632-675 as Renderer.nope_nerf calls them (rendering.py:169-181) plus
d_gt = 1 - 1 / d_src (rendering.py:158-159), evaluated at a dtype with autograd for the gradients, and
the input sets and bars of tests/test_ndc_reference_cpu.py and tests/test_gpu_ndc_fp64.py.

Bars, the rule of tests/test_gpu_pair_fp64.py: per element |got - f64| <= T + 4 E_f32, T = 2^-23 of the
tensor's largest entry (one ulp of it), E_f32 the max-norm error of this reference run in f32 against
its f64 run on the same inputs -- never a number taken from the kernels.  The two reduced focal
gradients get, on top, the room a different summation order of R f32 terms can take:
(R - 1) 2^-24 sum |per-ray term|, the terms from the f64 run."""
from __future__ import annotations

import torch

ULP = 2.0 ** -23
F32_MARGIN = 4.0
EDGE_RAYS = (1, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097)
# which of (g_o, g_d, g_dgt) reach the backward
GRAD_COMBOS = {"all": (True, True, True), "only_g_o": (True, False, False), "only_g_d": (False, True, False),
               "only_g_dgt": (False, False, True)}
WRONG = ("no_shift", "near_not_2near", "plus_fy", "dgt_recip")


def ndc_expr(fx, fy, near, rays_o, rays_d, _wrong=None):
    """common.py:632-675 with fx, fy scalars or one value per ray (the same elementwise operations)."""
    t = -(near + rays_o[..., 2]) / rays_d[..., 2]
    o = rays_o if _wrong == "no_shift" else rays_o + t[..., None] * rays_d
    ox, oy = o[..., 0] / o[..., 2], o[..., 1] / o[..., 2]
    if _wrong == "plus_fy":
        fy = -fy
    o2 = 1.0 + (1.0 if _wrong == "near_not_2near" else 2.0) * near / o[..., 2]
    o_ndc = torch.stack([-1.0 / (1 / fx) * ox, -1.0 / (1 / fy) * oy, o2], -1)
    d_ndc = torch.stack([-1.0 / (1 / fx) * (rays_d[..., 0] / rays_d[..., 2] - ox),
                         -1.0 / (1 / fy) * (rays_d[..., 1] / rays_d[..., 2] - oy),
                         1 - o2], -1)
    return o_ndc, d_ndc


def ndc_inputs(R, seed=0, with_dsrc=True):
    """The generic set: origins within +-0.3, +-0.3, +-0.2; unit directions with |d_z| >= 0.8 and both
    signs of x, y and z; fx = 2.4, fy = -3.2 as camera_mat[1][1] carries it; near = 1; d_src in
    [0.05, 20] (log-uniform); upstream gradients of order one."""
    g = torch.Generator().manual_seed(1000 + 7 * R + seed)
    u = lambda *s: torch.rand(*s, generator=g)      # noqa: E731
    cam = (u(R, 3) * 2 - 1) * torch.tensor([0.3, 0.3, 0.2])
    dz = (0.8 + 0.2 * u(R)) * torch.where(u(R) < 0.5, -1.0, 1.0)
    phi = 2 * torch.pi * u(R)
    s = torch.sqrt(1 - dz * dz)
    ray = torch.stack([s * torch.cos(phi), s * torch.sin(phi), dz], -1)
    K = torch.tensor([[2.4, 0, 0, 0], [0, -3.2, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], dtype=torch.float32)
    d_src = 0.05 * (400.0 ** u(R)) if with_dsrc else None
    return {"cam": cam.float(), "ray": ray.float(), "K": K, "near": 1.0, "d_src": d_src,
            "g_o": torch.randn(R, 3, generator=g), "g_d": torch.randn(R, 3, generator=g),
            "g_dgt": torch.randn(R, generator=g)}


def ndc_ref(inp, dtype, combo="all", _wrong=None):
    """The warp and its gradients at dtype -> dict: o_ndc, d_ndc [R,3], d_gt [R] (with a d_src), and for
    the upstream gradients of GRAD_COMBOS[combo]: g_cam, g_ray [R,3], g_dsrc [R], gK [4,4] (only [0][0]
    and [1][1] non-zero) and fx_terms, fy_terms [R], the per-ray terms the two focal gradients sum."""
    R = inp["cam"].shape[0]
    c = lambda t: t.detach().to(dtype).clone()      # noqa: E731
    cam, ray = c(inp["cam"]).requires_grad_(True), c(inp["ray"]).requires_grad_(True)
    K = c(inp["K"])
    fx = (K[0, 0] * torch.ones(R, dtype=dtype)).requires_grad_(True)      # one leaf per ray: its grad is the term
    fy = (K[1, 1] * torch.ones(R, dtype=dtype)).requires_grad_(True)
    o_ndc, d_ndc = ndc_expr(fx, fy, inp["near"], cam, ray, _wrong)
    out = {"o_ndc": o_ndc.detach(), "d_ndc": d_ndc.detach()}
    d_src = d_gt = None
    if inp["d_src"] is not None:
        d_src = c(inp["d_src"]).requires_grad_(True)
        d_gt = 1 / d_src if _wrong == "dgt_recip" else 1 - 1 / d_src
        out["d_gt"] = d_gt.detach()
    use_o, use_d, use_g = GRAD_COMBOS[combo]
    loss = torch.zeros((), dtype=dtype)
    if use_o:
        loss = loss + (o_ndc * c(inp["g_o"])).sum()
    if use_d:
        loss = loss + (d_ndc * c(inp["g_d"])).sum()
    if use_g and d_gt is not None:
        loss = loss + (d_gt * c(inp["g_dgt"])).sum()
    leaves = [cam, ray, fx, fy] + ([d_src] if d_src is not None else [])
    if loss.requires_grad:
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    else:
        grads = [None] * len(leaves)
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    out["g_cam"], out["g_ray"] = z(grads[0], cam), z(grads[1], ray)
    out["fx_terms"], out["fy_terms"] = z(grads[2], fx), z(grads[3], fy)
    gK = torch.zeros(4, 4, dtype=dtype)
    gK[0, 0], gK[1, 1] = out["fx_terms"].sum(), out["fy_terms"].sum()
    out["gK"] = gK
    if d_src is not None:
        out["g_dsrc"] = z(grads[4], d_src)
    return out


def ndc_refs(inp, combo="all"):
    return ndc_ref(inp, torch.float64, combo), ndc_ref(inp, torch.float32, combo)


def reduce_room(r64, R):
    """[4,4] extra room of gK for the order of an f32 sum of R terms: (R - 1) 2^-24 sum |term| (derived:
    each of the R - 1 additions rounds a partial sum bounded by sum |term| to half an ulp)."""
    room = torch.zeros(4, 4, dtype=torch.float64)
    room[0, 0] = (R - 1) * 2.0 ** -24 * r64["fx_terms"].abs().sum().item()
    room[1, 1] = (R - 1) * 2.0 ** -24 * r64["fy_terms"].abs().sum().item()
    return room


def bar_check(name, got, r64, r32, where="", extra=None):
    """|got - f64| <= 2^-23 max|f64| + 4 max|f32 - f64| (+ extra) per element -> the worst ratio to the bar."""
    got = got.detach().cpu().double().reshape(r64.shape)
    r64, r32 = r64.double(), r32.double()
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), f"{where}: reference {name} not finite"
    assert bool(torch.isfinite(got).all()), f"{where}: {name} not finite"
    e32 = (r32 - r64).abs().max().item() if r64.numel() else 0.0
    T = ULP * (r64.abs().max().item() if r64.numel() else 0.0)
    lim = torch.full_like(r64, T + F32_MARGIN * e32)
    if extra is not None:
        lim = lim + extra
    err = (got - r64).abs()
    ratio = (err / lim.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"{where} {name}: |got-f64| {err.max().item() if err.numel() else 0.0:.3e}  E_f32 {e32:.3e}  T {T:.3e}  "
          f"ratio {ratio:.3f}")
    bad = (err > lim).nonzero()
    assert bad.numel() == 0, (f"{where}: {name}: {bad.shape[0]} elements over the bar, first {bad[:4].tolist()}: "
                              f"|got - f64| up to {err.max().item():.3e} > {T:.3e} + 4 * {e32:.3e}")
    return ratio


FWD_NAMES = ("o_ndc", "d_ndc", "d_gt")
BWD_NAMES = ("g_cam", "g_ray", "g_dsrc", "gK")


def check_all(got, r64, r32, R, where=""):
    """Every tensor of `got` (a dict with names of FWD_NAMES / BWD_NAMES) against the bars."""
    for name, t in got.items():
        if t is None:
            continue
        bar_check(name, t, r64[name], r32[name], where, reduce_room(r64, R) if name == "gK" else None)


def emulate_f32(inp, combo="all", _wrong=None):
    """What a correct f32 implementation returns (the f32 run of the reference, or a wrong variant of
    it), under the names check_all takes."""
    r = ndc_ref(inp, torch.float32, combo, _wrong)
    return {k: r[k] for k in FWD_NAMES + BWD_NAMES if k in r}
