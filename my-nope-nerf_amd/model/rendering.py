"""Renderer on the MI355X path (drop-in for model/rendering.py).

``Renderer.forward`` / ``nope_nerf`` keep the reference signatures and out-dict keys
(rendering.py:22-168).  Ray generation is a handful of 4x4 / per-ray tensor ops; the
per-sample work (samples, encodings, MLP, heads, compositing) and its backward run as one
fused call into the nerf_hip kernels (field.render_field), so the reference's 64 000-sample
chunk loop (rendering.py:100-111), its ``cat``s and its ``cumprod`` never appear.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .common import get_mask, get_ndc_rays_fxfy, unproject_matrix
from .rays import camera_rays_hip, ndc_rays
from .field import F_DIST_ALPHA, F_RELU, F_WHITE_BKGD, render_field, render_field_eval

epsilon = 1e-6  # rendering.py:9 (applied inside the composite kernel)


def camera_rays(pixels, depth, camera_mat, world_mat, scale_mat, normalise_ray=True):
    """rendering.py:52-80: origin, unit direction, ray-vector norm, guide distance d_src
    (= |P_depth - o|) and the depth-loss mask for pixels [1,R,2] with depth [1,R,1]."""
    M = unproject_matrix(camera_mat, world_mat, scale_mat)          # [1,4,4]
    R = pixels.shape[1]
    origin = M[:, :3, 3]                                            # M @ [0,0,0,1]
    cam = origin.unsqueeze(1).expand(1, R, 3)
    ones = torch.ones_like(pixels[..., :1])
    pix1 = torch.cat([pixels, ones, ones], dim=-1).transpose(1, 2)  # [x, y, 1, 1]
    p_world = (M @ pix1)[:, :3].transpose(1, 2)
    ray = p_world - cam
    ray_norm = ray.norm(2, 2)
    if depth is not None:
        pd = torch.cat([pixels * depth, depth, ones], dim=-1).transpose(1, 2)
        p_depth = (M @ pd)[:, :3].transpose(1, 2)
        d_src = torch.norm(p_depth - cam, p=2, dim=-1)
    else:
        d_src = torch.ones_like(ray_norm)
    if normalise_ray:
        ray = ray / ray_norm.unsqueeze(-1)
    else:
        d_src = d_src / ray_norm
    mask = (get_mask(d_src) & (d_src != 0))[0]                      # rendering.py:69-80
    return cam.reshape(-1, 3), ray.reshape(-1, 3), ray_norm[0], d_src[0], mask


def get_sphere_intersection(cam_loc, ray_directions, r=1.0):
    """rendering.py:447-468: (near, far) distances along the rays to the sphere |x| = r,
    0 without an intersection, clamped at 0; and the intersection mask."""
    n_imgs, n_pix, _ = ray_directions.shape
    cam = cam_loc.unsqueeze(-1)
    ray_cam_dot = torch.bmm(ray_directions, cam).squeeze(-1).reshape(-1)
    under_sqrt = ray_cam_dot ** 2 - (cam.norm(2, 1) ** 2 - r ** 2).reshape(-1).repeat_interleave(n_pix)
    mask = under_sqrt > 0
    root = torch.sqrt(under_sqrt.clamp_min(0)).unsqueeze(-1) * torch.tensor([-1.0, 1.0], device=cam_loc.device)
    inter = torch.where(mask.unsqueeze(-1), root - ray_cam_dot.unsqueeze(-1), torch.zeros_like(root))
    return inter.reshape(n_imgs, n_pix, 2).clamp_min(0.0), mask.reshape(n_imgs, n_pix)


class Renderer(nn.Module):
    def __init__(self, model, cfg, device=None, **kwargs):
        super().__init__()
        self._device = device
        self.depth_range = cfg["depth_range"]
        self.n_max_network_queries = cfg["n_max_network_queries"]
        self.white_background = cfg["white_background"]
        self.cfg = cfg
        self.model = model.to(device) if device is not None else model

    def forward(self, pixels, depth, camera_mat, world_mat, scale_mat, rendering_technique,
                add_noise=True, eval_=False, it=1000000, **kw):
        if rendering_technique == "nope_nerf":
            return self.nope_nerf(pixels, depth, camera_mat, world_mat, scale_mat, it=it,
                                  add_noise=add_noise, eval_=eval_, **kw)
        if rendering_technique == "phong_renderer":
            return self.phong_renderer(pixels, camera_mat, world_mat, scale_mat, it)
        raise NotImplementedError(f"rendering_technique '{rendering_technique}'")

    # ------------------------------------------------------------ geometry visualisation
    def phong_renderer(self, pixels, camera_mat, world_mat, scale_mat, it):
        """rendering.py:199-258: the occupancy surface found by ray marching, shaded with a
        headlight (ambient 0.3 + diffuse 0.7 of the normal -d sigma_raw/dp), background 1;
        'rgb_surf' is the field's colour at the surface.  The field evaluations (512 samples
        per ray, 8 secant steps, the normals) run on the nerf_hip MLP kernels."""
        B, n, _ = pixels.shape
        dev = pixels.device
        rad = self.cfg["radius"]
        M = unproject_matrix(camera_mat, world_mat, scale_mat)
        cam, ray, _, _, _, _ = camera_rays_hip(M, pixels, None, True, view_ones=True)
        cam_w, ray = cam.view(1, n, 3), ray.view(1, n, 3)
        light_src = cam_w[0, 0]
        light = (light_src / light_src.norm(2)).unsqueeze(1)
        diffuse_per = torch.tensor([0.7, 0.7, 0.7], device=dev)
        ambient = torch.tensor([0.3, 0.3, 0.3], device=dev)
        was_training = self.model.training
        self.model.eval()
        with torch.no_grad():
            d_i = self.ray_marching(cam_w, ray, self.model, n_secant_steps=8, n_steps=[512, 513], rad=rad)
            zero_occ = d_i == 0
            mask_pred = get_mask(d_i)
            dists = torch.where(mask_pred, d_i, torch.ones_like(d_i))
            dists = torch.where(zero_occ, torch.zeros_like(dists), dists)
            obj = (mask_pred & ~zero_occ)[0]
            dists = dists[0]
            cam_f, ray_f = cam_w.reshape(-1, 3), ray.reshape(-1, 3)
            points = cam_f + ray_f * dists.unsqueeze(-1)
            view = -ray_f
            rgb = torch.ones_like(points)
            surf, surf_view = points[obj], view[obj]
            rgb_surf = torch.zeros(B * n, 3, device=dev)
            if surf.shape[0] > 0:
                grad = self.model.gradient(surf, it)[:, 0, :].detach()
                normals = grad / grad.norm(2, 1, keepdim=True)
                diffuse = torch.mm(normals, light).clamp_min(0).repeat(1, 3) * diffuse_per.unsqueeze(0)
                rgb[obj] = (ambient.unsqueeze(0) + diffuse).clamp_max(1.0)
                rgb_surf[obj] = self.model(surf, surf_view)
        self.model.train(was_training)
        return {"rgb": rgb.reshape(B, -1, 3), "normal": None, "rgb_surf": rgb_surf.reshape(B, -1, 3)}

    def phong_frame(self, pixels, camera_mat, world_mat, scale_mat, it, n_steps=512, n_secant_steps=8, tau=0.5):
        """phong_renderer for a whole frame of GPU pixels in one call, without its chunk loop, boolean
        indices and host syncs (model/geometry.py, csrc/march.hip); the dict also carries 'd_i' [1, R]
        and 'mask' [R]."""
        from .geometry import phong_frame
        return phong_frame(self, pixels, camera_mat, world_mat, scale_mat, it, n_steps=n_steps,
                           n_secant_steps=n_secant_steps, tau=tau)

    def ray_marching(self, ray0, ray_direction, model, c=None, tau=0.5, n_steps=[128, 129], n_secant_steps=8,
                     depth_range=[0.0, 2.4], max_points=3500000, rad=1.0):
        """rendering.py:262-403: evaluate n_steps samples between depth_range[0] and the far
        intersection with the sphere of radius ``rad``, take the first outside->inside sign
        change of occupancy - tau and refine it with the secant method; inf where there is
        none, 0 where the first sample is already occupied.  All samples are one batched
        field evaluation (max_points chunks)."""
        B, n_pts, _ = ray0.shape
        dev = ray0.device
        n_steps = int(torch.randint(n_steps[0], n_steps[1], (1,)).item())
        d_int, _ = get_sphere_intersection(ray0[:, 0], ray_direction, r=rad)
        d_far = d_int[..., 1]
        t = torch.linspace(0, 1, steps=n_steps, device=dev).view(1, 1, n_steps, 1)
        d_prop = depth_range[0] * (1.0 - t) + d_far.view(1, -1, 1, 1) * t
        p_prop = (ray0.unsqueeze(2) + ray_direction.unsqueeze(2) * d_prop).reshape(-1, 3)
        val = torch.cat([model(ps, only_occupancy=True) - tau for ps in torch.split(p_prop, max_points)])
        val = val.view(B, n_pts, n_steps)
        mask_0_not_occ = val[:, :, 0] < 0
        sign = torch.cat([torch.sign(val[:, :, :-1] * val[:, :, 1:]), torch.ones(B, n_pts, 1, device=dev)], -1)
        cost = sign * torch.arange(n_steps, 0, -1, device=dev).float()
        values, idx = torch.min(cost, -1)
        mask_sign_change = values < 0
        mask_neg_to_pos = torch.gather(val, 2, idx.unsqueeze(-1)).squeeze(-1) < 0
        mask = mask_sign_change & mask_neg_to_pos & mask_0_not_occ
        dp = d_prop.expand(B, n_pts, n_steps, 1)[..., 0]
        take = lambda a, i: torch.gather(a, 2, i.unsqueeze(-1)).squeeze(-1)[mask]
        idx_h = torch.clamp(idx + 1, max=n_steps - 1)
        d_low, f_low, d_high, f_high = take(dp, idx), take(val, idx), take(dp, idx_h), take(val, idx_h)
        d_out = torch.ones(B, n_pts, device=dev)
        if d_low.shape[0] != 0:
            d_out[mask] = self.secant(f_low, f_high, d_low, d_high, n_secant_steps, ray0[mask],
                                      ray_direction[mask], tau, model=model)
        d_out = torch.where(mask, d_out, torch.full_like(d_out, float("inf")))
        d_out = torch.where(mask_0_not_occ, d_out, torch.zeros_like(d_out))
        return d_out

    def secant(self, f_low, f_high, d_low, d_high, n_secant_steps, ray0_masked, ray_direction_masked, tau,
               it=0, model=None):
        """rendering.py:405-436."""
        model = model if model is not None else self.model
        d_pred = -f_low * (d_high - d_low) / (f_high - f_low) + d_low
        for _ in range(n_secant_steps):
            p_mid = ray0_masked + d_pred.unsqueeze(-1) * ray_direction_masked
            f_mid = model(p_mid, only_occupancy=True, it=it)[..., 0] - tau
            low = f_mid < 0
            d_low = torch.where(low, d_pred, d_low)
            f_low = torch.where(low, f_mid, f_low)
            d_high = torch.where(low, d_high, d_pred)
            f_high = torch.where(low, f_high, f_mid)
            d_pred = -f_low * (d_high - d_low) / (f_high - f_low) + d_low
        return d_pred

    def _flags(self) -> int:
        f = 0
        if self.cfg["dist_alpha"]:
            f |= F_DIST_ALPHA
        if self.white_background:
            f |= F_WHITE_BKGD
        if getattr(self.model, "occ_activation", "softplus") != "softplus":
            f |= F_RELU
        return f

    def normal_diff(self, cam, ray, d_src, mask, it, noise=None):
        """rendering.py:127-135 (the ``normal_loss`` branch): at the rays' depth-prior surface
        points and a jittered copy of each (U[-0.005, 0.005) per coordinate), the normals
        -d sigma_raw/dp / (|.| + 1e-5) from the HIP field backward; returns |n - n_jitter| per
        surface point.  ``noise`` injects the U[0,1) jitter (N,3).  The reference builds the
        normals with create_graph=True; here they are first order (OfficialStaticNerf.gradient):
        a loss backpropagated through the result raises in its backward (_FirstOrderOnly)."""
        surface = (cam + ray * d_src.unsqueeze(-1))[mask]
        n = surface.shape[0]
        if noise is None:
            noise = torch.rand_like(surface)
        neighbours = surface + (noise - 0.5) * 0.01
        g = self.model.gradient(torch.cat([surface, neighbours], 0), it)[:, 0, :]
        normals = g / (g.norm(2, dim=1).unsqueeze(-1) + 10 ** (-5))
        return torch.norm(normals[:n] - normals[n:], dim=-1)

    def nope_nerf(self, pixels, depth, camera_mat, world_mat, scale_mat, add_noise=False, it=100000,
                  eval_=False, noise=None, dense_depth=False, normal_noise=None, field_grad=True, rays=None):
        """rendering.py:36-168.  Extra keyword arguments of the MI355X build:
        ``noise`` injects the stratified U[0,1) tensor (1,R,S) instead of torch.rand;
        ``dense_depth`` returns unmasked depth_pred/depth_gt plus 'depth_mask' (R,) so the
        training step never needs the boolean-index host sync (rendering.py:151-153);
        ``normal_noise`` injects the (N,3) jitter of the normal_loss branch;
        ``field_grad=False`` renders a frozen field: gradients reach the camera matrices only
        and no field parameter gets a ``.grad`` (Trainer_pose, eval_pose_one_epoch.py:44-61);
        ``rays`` = (cam, ray, view, ray_norm, d_src, mask) of these pixels, built by the caller
        (the Trainer's step head) instead of the two launches below."""
        cfg = self.cfg
        S = cfg["num_points"] - cfg.get("outside_steps", 0)
        near, far = float(self.depth_range[0]), float(self.depth_range[1])
        if rays is not None:
            cam, ray, view, ray_norm, d_src, mask = rays
        elif pixels.is_cuda:     # two launches: the unprojection matrix, then every ray
            M = unproject_matrix(camera_mat, world_mat, scale_mat)
            cam, ray, view, ray_norm, d_src, mask = camera_rays_hip(
                M, pixels, depth, cfg["normalise_ray"], view_ones=not cfg["use_ray_dir"])
        else:
            cam, ray, ray_norm, d_src, mask = camera_rays(pixels, depth, camera_mat, world_mat, scale_mat,
                                                          cfg["normalise_ray"])
            view = -ray if cfg["use_ray_dir"] else torch.ones_like(ray)
        R = cam.shape[0]
        ndc = cfg["sample_option"] == "ndc"
        ndc_hip = ndc and cam.is_cuda
        if ndc_hip:                              # rendering.py:169-181 and :158-159 in one launch
            if eval_ and cfg["normalise_ray"]:   # rendering.py:144-148 comes before the 1 - 1 / d
                d_src = d_src / ray_norm
            pts_o, pts_d, d_src = ndc_rays(cam, ray, camera_mat, 1.0, d_src)
            near_s, far_s, nz = 0.0, 1.0, None
        elif ndc:                                # rendering.py:169-181 (no jitter)
            fxfy = torch.cat([camera_mat[:, 0, 0], camera_mat[:, 1, 1]])
            pts_o, pts_d = get_ndc_rays_fxfy(fxfy, 1.0, cam, ray)
            near_s, far_s, nz = 0.0, 1.0, None
        else:                                    # rendering.py:183-198
            pts_o, pts_d = cam, ray
            near_s, far_s = near, far
            nz = None
            if add_noise:
                nz = noise if noise is not None else torch.rand(1, R, S, device=cam.device)
                nz = nz.reshape(R, S).float()
        flags = self._flags()
        if torch.is_grad_enabled():
            rgb, dist, alpha, z = render_field(self.model, pts_o, pts_d, view, nz, near_s, far_s, S, flags,
                                               field_grad=field_grad)
        else:
            rgb, dist, alpha, z = render_field_eval(self.model, pts_o, pts_d, view, near_s, far_s, S, flags) \
                if nz is None else render_field(self.model, pts_o, pts_d, view, nz, near_s, far_s, S, flags)
        if eval_ and cfg["normalise_ray"]:       # rendering.py:144-148
            dist = dist / ray_norm
            if not ndc_hip:
                d_src = d_src / ray_norm
        if ndc and not ndc_hip:
            d_src = 1 - 1 / d_src
        normal = None
        if not eval_ and cfg.get("normal_loss", False):          # rendering.py:127-137
            normal = self.normal_diff(cam, ray, d_src, mask, it, normal_noise)
        out = {"rgb": rgb.reshape(1, -1, 3), "z_vals": z, "normal": normal, "alpha": alpha}
        if eval_:
            out["depth_pred"], out["depth_gt"] = dist, d_src
        elif dense_depth:
            out["depth_pred"], out["depth_gt"], out["depth_mask"] = dist, d_src, mask
        else:                                    # rendering.py:151-153
            out["depth_pred"], out["depth_gt"] = dist[mask], d_src[mask]
        return out
