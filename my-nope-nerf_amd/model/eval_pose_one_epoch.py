"""Test-time pose refinement (drop-in for model/eval_pose_one_epoch.py:10-98).

evaluation/eval.py:117-141 optimises the poses of the evaluation images -- which have no
trained pose -- against the trained field before it renders them: ``Trainer_pose.train_step``
renders ``n_points`` random rays of one image in eval mode and steps ``optimizer_pose`` on the
MSE to the image.  Same constructor, ``train_step`` / ``process_data_dict`` / ``compute_loss``
signatures and loss-dict key.

The field is frozen in that step: only ``optimizer_pose`` steps.  The reference still
backpropagates into every field parameter and never uses the result; here the render runs with
``field_grad=False`` (rendering.Renderer.nope_nerf), so the backward stops at the rays -- no
weight gradient is computed and the field's parameters get no ``.grad`` from this step.
"""
from __future__ import annotations

import torch

from .common import arange_pixels, inv
from .losses import Loss_Eval
from .rays import can_sample_on_device
from .rays import sample_rays as sample_rays_dev


class Trainer_pose(object):
    def __init__(self, model, cfg, device=None, optimizer_pose=None, pose_param_net=None, focal_net=None, **kwargs):
        self.model = model
        self.device = device
        self.optimizer_pose = optimizer_pose
        self.pose_param_net = pose_param_net
        self.focal_net = focal_net
        self.n_points = cfg["n_points"]
        self.rendering_technique = cfg["type"]
        self.loss = Loss_Eval()
        self._pix_cache = {}
        # test hook, as Trainer.inject: a ray_idx tensor replaces the next draws of compute_loss
        # (the reference's randperm), so a step can be replayed on the oracle
        self.inject = None
        # False: the render's backward stops at the rays.  True (measurements only,
        # scripts/pose_refine_bench.py) runs the training backward as the reference does: every
        # field parameter then accumulates a .grad that nothing reads
        self.field_grad = False

    def train_step(self, data, it=100000):
        """eval_pose_one_epoch.py:25-41."""
        self.model.eval()
        self.pose_param_net.train()
        self.optimizer_pose.zero_grad()
        if self.focal_net is not None:
            self.focal_net.eval()
        loss_dict = self.compute_loss(data, it=it)
        loss_dict["loss"].backward()
        self.optimizer_pose.step()
        return loss_dict

    def process_data_dict(self, data):
        """eval_pose_one_epoch.py:44-60."""
        dev = self.device
        img = data.get("img").to(dev)
        img_idx = data.get("img.idx")
        B, _, h, w = img.shape
        depth_img = data.get("img.depth", torch.ones(B, h, w)).unsqueeze(1).to(dev)
        camera_mat = data.get("img.camera_mat").to(dev)
        scale_mat = data.get("img.scale_mat").to(dev)
        return (img, depth_img, camera_mat, scale_mat, img_idx)

    def _pixels(self, h, w, device):
        key = (h, w, str(device))
        if key not in self._pix_cache:
            self._pix_cache[key] = arange_pixels((h, w), 1, device=device)[1]
        return self._pix_cache[key]

    def sample_rays(self, img, h, w):
        """eval_pose_one_epoch.py:85-89: ``n_points`` distinct pixels with their coordinates and
        colours -- on the device one launch of the training step's sampler (rays.sample_rays)."""
        B, n_pix, R = img.shape[0], h * w, self.n_points
        if img.is_cuda and B == 1 and can_sample_on_device(n_pix, R):
            return sample_rays_dev(n_pix, R, w, h, img[0])
        ray_idx = torch.randperm(n_pix, device=img.device)[:R]
        return ray_idx, self._pixels(h, w, img.device)[:, ray_idx], img.view(B, 3, n_pix).permute(0, 2, 1)[:, ray_idx]

    def compute_loss(self, data, eval_mode=False, it=100000):
        """eval_pose_one_epoch.py:62-98."""
        img, depth_img, camera_mat, scale_mat, img_idx = self.process_data_dict(data)
        dev = self.device
        B, _, h, w = img.shape
        c2w = self.pose_param_net(img_idx)
        world_mat = inv(c2w).unsqueeze(0)
        if self.focal_net is not None:
            fxfy = self.focal_net(0)
            pad = torch.zeros(4, device=dev)
            one = torch.ones(1, device=dev)
            camera_mat = torch.cat([fxfy[0:1], pad, -fxfy[1:2], pad, -one, pad, one]).view(1, 4, 4)
        if self.inject is not None:
            ray_idx = self.inject.to(dev)
            rgb_gt = img.view(B, 3, h * w).permute(0, 2, 1)[:, ray_idx]
            p = self._pixels(h, w, dev)[:, ray_idx]
        else:
            ray_idx, p, rgb_gt = self.sample_rays(img, h, w)
        out = self.model(p, ray_idx, camera_mat, world_mat, scale_mat, self.rendering_technique, it=it,
                         eval_mode=True, depth_img=depth_img, add_noise=False, img_size=(h, w), field_grad=self.field_grad)
        return self.loss(out["rgb"], rgb_gt)
