"""The geometry visualisation of a whole frame on the GPU (rendering.py:199-468).

``phong_frame`` is ``Renderer.phong_renderer`` for device tensors without its data-dependent
shapes: every step is dense over the frame's R rays, the per-ray logic runs in the four kernels of
csrc/march.hip and the field evaluations are the launches the colour render already uses.  No
boolean index, no ``.item()`` and no host sync, so a frame is one call (and can be captured as a
graph) instead of a loop of 1024-pixel chunks that each compact three times.

Occupancy of the n_steps samples per ray, two routes:
  * the fused eval render (nerf_render_eval_fused; GEMM precision mode 2, hidden 256) when
    ``dist_alpha`` is off and n_steps is a multiple of 128: a ray becomes n_steps / 128
    pseudo-rays of 128 samples (nerf_march_rays) and the launch's ``alpha`` output, which with
    dist_alpha off is 1 - exp(-sigma), is the [R][n_steps] occupancy array as it lies in memory;
  * otherwise the per-layer forward on the raw head output, in ray chunks of a fixed size,
    followed by ``OfficialStaticNerf._density``.
"""
from __future__ import annotations

import torch

from . import _hip
from .common import unproject_matrix
from .field import F_DIST_ALPHA, F_RELU
from .rays import camera_rays_hip

FUSED_SEG = 128            # samples per pseudo-ray on the fused route (the kernel's row block)
RAW_RAY_CHUNK = 8192       # rays per forward on the raw route: 4.2 M rows at 512 steps, as render_field_eval


def _activation_flags(module) -> int:
    f = 0 if module.occ_activation == "softplus" else F_RELU
    return f | (F_DIST_ALPHA if module.dist_alpha else 0)


def _forward(runner, *args, **kw):
    """runner.forward on weights packed once for the frame (they do not change inside it)."""
    runner.prepacked = True
    return runner.forward(*args, **kw)


def occupancy_samples(module, cam, ray, rad, d0, n_steps):
    """-> (occ [R][n_steps], d_far [R]): the field's occupancy at the n_steps samples of every ray between
    d0 and the far intersection with the sphere of radius rad.  The weights are packed already."""
    runner = module.hip_runner()
    R = cam.shape[0]
    fused = runner.use_fused_eval(FUSED_SEG) and not module.dist_alpha and n_steps % FUSED_SEG == 0
    seg = FUSED_SEG if fused else n_steps
    d_far, o_seg, d_seg = _hip.march_rays(cam, ray, rad, d0, n_steps, seg)
    if fused:
        runner.prepacked = True
        alpha = runner.render_eval_fused(o_seg, d_seg, d_seg, 0.0, 1.0, seg, _activation_flags(module) & F_RELU)[2]
        return alpha.view(R, n_steps), d_far
    occ = torch.empty(R, n_steps, device=cam.device)
    for r0 in range(0, R, RAW_RAY_CHUNK):
        r1 = min(R, r0 + RAW_RAY_CHUNK)
        raw4 = _forward(runner, o_seg[r0:r1], d_seg[r0:r1], d_seg[r0:r1], None, 0.0, 1.0, n_steps, 0, keep=False,
                        composite=False)[0]
        occ[r0:r1] = module._density(raw4[:(r1 - r0) * n_steps, 0]).view(r1 - r0, n_steps)
    return occ, d_far


@torch.no_grad()
def phong_frame(renderer, pixels, camera_mat, world_mat, scale_mat, it, n_steps=512, n_secant_steps=8, tau=0.5):
    """The dict of Renderer.phong_renderer for pixels [1, R, 2] on the GPU, plus 'd_i' [1, R] (the
    surface distance: inf without a surface, 0 when the ray starts inside) and 'mask' [R] (the rays
    that are shaded)."""
    if pixels.shape[0] != 1:
        raise ValueError(f"phong_frame: one image per call, got a batch of {pixels.shape[0]}")
    module = renderer.model
    M = unproject_matrix(camera_mat, world_mat, scale_mat)
    cam, ray, _, _, _, _ = camera_rays_hip(M, pixels, None, True, view_ones=True)
    cam, ray = cam.reshape(-1, 3).contiguous(), ray.reshape(-1, 3).contiguous()
    R = cam.shape[0]
    dev = cam.device
    d0 = 0.0                                      # ray_marching's depth_range[0]
    runner = module.hip_runner()
    act = _activation_flags(module)
    was_training = module.training
    module.eval()
    runner.prepacked = False
    runner.pack()
    try:
        occ, d_far = occupancy_samples(module, cam, ray, renderer.cfg["radius"], d0, n_steps)
        state, *bracket = _hip.march_select(occ, d_far, d0, tau)
        del occ

        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)   # noqa: E731
        d_pred, p_mid, d_i = e(R), e(R, 3), e(R)
        zeros = torch.zeros(R, 3, device=dev)
        raw4 = None
        for k in range(n_secant_steps + 1):
            _hip.secant_step(k == 0, raw4, act, tau, state, cam, ray, bracket, d_pred, p_mid, d_i)
            if k < n_secant_steps:
                raw4 = _forward(runner, p_mid, zeros, zeros, None, 0.0, 0.0, 1, 0, keep=False, composite=False)[0]

        # the normals and the surface colour from one forward and its ray-only backward: sigma_raw does
        # not depend on the view direction, so d sigma_raw / dp is that of the reference's view = 0 call
        raw4, _, _, _, st = _forward(runner, p_mid, zeros, -ray, None, 0.0, 0.0, 1, 0, keep=True, composite=False)
        graw4 = torch.zeros(st["Np"], 4, device=dev)
        graw4[:R, 0] = 1.0
        g_p = runner.backward(st, None, None, True, graw4=graw4, want_weight_grad=False)[1][0]
        rgb, rgb_surf = _hip.phong_shade(-g_p, raw4, state, d_i, cam)
    finally:
        runner.prepacked = False                  # a later call packs again
        module.train(was_training)
    mask = (state == _hip.MARCH_BRACKET) & torch.isfinite(d_i)
    return {"rgb": rgb.view(1, R, 3), "normal": None, "rgb_surf": rgb_surf.view(1, R, 3), "d_i": d_i.view(1, R),
            "mask": mask}
