"""Eval_Images (drop-in for model/eval_images.py:17-218; imported by evaluation/eval.py:14 and
called per held-out frame at eval.py:146-188).

Same constructor, ``process_data_dict`` and ``eval_images(data, render_dir, fxfy, lpips_vgg_fn,
logger, min_depth, max_depth, it, sc, show_errors)`` signature, output files and returned dict.
The frame is rendered by Extract_Images.render_frame (render_dist.render_image for nope_nerf,
the chunked loop otherwise).  MSE / PSNR / SSIM come from one nerf_image_metrics call on the
renderer's [H,W,3] frame and the loader's [1,3,H,W] image as they lie in memory, with one
device-to-host copy of the two scalars per frame (the reference: three .item() calls, five
convolutions and two permuted copies).  Everything after the metrics is host numpy, as in the
reference.

Additions: ``eval_metrics`` returns the image metrics and the depth metrics (one nerf_depth_metrics
call: resample, masks, confusion counts and compute_errors' seven errors in fp64) of a frame as
device tensors, writing nothing; ``summarise`` turns a list of them into the table of
evaluation/eval.py:190-212 with one device-to-host copy.

Deviations: ``lpips_vgg_fn=None`` gives ``float('nan')`` for 'lpips' (the lpips package is a VGG
network and stays the caller's to provide; the reference would raise).  Images are written with
PIL, the disparity colour map is matplotlib's inferno and the depth resize is
metrics.resize_nearest_exact, since imageio / cv2 are not dependencies of this package.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .common import mse2psnr
from .extracting_images import Extract_Images, _inferno, _to_u8_range, _write_png
from .metrics import DEPTH_METRIC_NAMES, depth_metrics, image_metrics, resize_nearest_exact


class Eval_Images(object):
    def __init__(self, renderer, cfg, points_batch_size=100000, use_learnt_poses=True, use_learnt_focal=True,
                 device=None, render_type=None, c2ws=None, img_list=None):
        self.points_batch_size = points_batch_size
        self.renderer = renderer
        self.resolution = cfg["extract_images"]["resolution"]
        self.device = device
        self.use_learnt_poses = use_learnt_poses
        self.use_learnt_focal = use_learnt_focal
        self.render_type = render_type
        self.c2ws = c2ws
        self.img_list = img_list

    # (rgb [h,w,3], depth [h,w]) of the whole frame: the one render method of both extractors
    render_frame = Extract_Images.render_frame

    def process_data_dict(self, data):
        """eval_images.py:30-45."""
        device = self.device
        img = data.get("img").to(device)
        batch_size, _, h, w = img.shape
        depth_img = data.get("img.depth", torch.ones(batch_size, h, w))
        depth_gt = data.get("img.gt_depths")
        img_idx = data.get("img.idx")
        camera_mat = data.get("img.camera_mat").to(device)
        scale_mat = data.get("img.scale_mat").to(device)
        return (img, depth_img, camera_mat, scale_mat, img_idx, depth_gt)

    def _frame_cameras(self, img_idx, camera_mat, fxfy):
        """(camera_mat, world_mat) of a held-out frame (eval_images.py:59-66): the learnt pose's
        inverse and the learnt focal's camera matrix where the evaluator uses them."""
        world_mat = None
        if self.use_learnt_poses:
            world_mat = torch.inverse(self.c2ws[img_idx]).unsqueeze(0)
        if self.use_learnt_focal:
            camera_mat = torch.tensor([[[fxfy[0], 0, 0, 0], [0, -fxfy[1], 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]]],
                                      dtype=torch.float32, device=self.device)
        return camera_mat, world_mat

    def eval_metrics(self, data, fxfy, min_depth=0.1, max_depth=20, it=0, sc=1):
        """The numbers of eval_images without its files: the same pose / focal handling and the same
        render_frame, then one image_metrics call and one depth_metrics call.  The ground-truth depth
        (img.gt_depths, or img.depth when absent, :53-57) is uploaded once as float32.  Returns
        {"image": [2] float32 (mse, ssim), "depth": [11] float64 (metrics.DEPTH_METRIC_NAMES)} as
        tensors on the renderer's device: no file is written and nothing is copied to the host, so the
        frames of a sequence can be stacked and read back once (summarise)."""
        self.renderer.eval()
        (img_gt, depth, camera_mat, scale_mat, img_idx, depth_gt) = self.process_data_dict(data)
        img_idx = int(img_idx)
        if depth_gt is None:
            depth_gt = depth
        camera_mat, world_mat = self._frame_cameras(img_idx, camera_mat, fxfy)
        with torch.no_grad():
            img_out, depth_pred = self.render_frame(camera_mat, world_mat, scale_mat, it)
            depth_gt = depth_gt.squeeze(0).to(device=depth_pred.device, dtype=torch.float32)
            return {"image": image_metrics(img_out, img_gt),
                    "depth": depth_metrics(depth_pred, depth_gt, min_depth, max_depth, sc=sc)}

    @staticmethod
    def summarise(records):
        """The table of evaluation/eval.py:190-212 from a list of eval_metrics results, with one
        device-to-host copy: the means over the frames of mse, psnr (of each frame's mse) and ssim, of
        the seven depth errors, and of the confusion matrix [[tp, fn], [fp, tn]] divided per frame by
        H*W - 1 -- the reference divides by the last pixel INDEX, not the pixel count
        (eval_images.py:162, 217); kept, so the table matches the reference's."""
        if not records:
            raise ValueError("summarise: no records")
        table = torch.stack([torch.cat([r["image"].double(), r["depth"]]) for r in records]).cpu().numpy()
        image, errors, counts = table[:, :2], table[:, 2:9], table[:, 9:13]
        conf = (counts / (counts.sum(1, keepdims=True) - 1)).mean(0)
        out = {"mse": float(image[:, 0].mean()), "psnr": float(np.mean([mse2psnr(m) for m in image[:, 0]])),
               "ssim": float(image[:, 1].mean())}
        out.update({k: float(v) for k, v in zip(DEPTH_METRIC_NAMES[:7], errors.mean(0))})
        out["conf_mat"] = conf.reshape(2, 2)
        return out

    def eval_images(self, data, render_dir, fxfy, lpips_vgg_fn, logger, min_depth=0.1, max_depth=20, it=0, sc=1,
                    show_errors=False):
        """eval_images.py:47-218."""
        self.renderer.eval()
        (img_gt, depth, camera_mat, scale_mat, img_idx, depth_gt) = self.process_data_dict(data)
        img_idx = int(img_idx)

        if depth_gt is not None:
            depth_gt = depth_gt.squeeze(0).numpy()
        else:
            print("No GT depths available, using input depths")
            depth_gt = depth.squeeze(0).numpy()

        camera_mat, world_mat = self._frame_cameras(img_idx, camera_mat, fxfy)

        with torch.no_grad():
            img_out, depth_pred = self.render_frame(camera_mat, world_mat, scale_mat, it)
            # mse and ssim of the entire image: one library call, one copy of the two scalars
            mse, ssim = image_metrics(img_out, img_gt).tolist()
        psnr = mse2psnr(mse)
        lpips_loss = float("nan")
        if lpips_vgg_fn is not None:
            # the one permuted copy of the path: the VGG wants contiguous [1,3,H,W]
            lpips_loss = lpips_vgg_fn(img_out.permute(2, 0, 1).unsqueeze(0).contiguous(), img_gt.contiguous(),
                                      normalize=True).item()
        print("{0:4d} img: PSNR: {1:.2f}, SSIM: {2:.2f},  LPIPS {3:.2f}".format(img_idx, psnr, ssim, lpips_loss))

        gt_height, gt_width = depth_gt.shape[:2]
        depth_out = depth_pred.cpu().numpy().copy()      # the frame's own depth stays as rendered
        depth_out *= sc
        depth_out = resize_nearest_exact(depth_out, (gt_height, gt_width))

        names = ("img_out", "depth_out", "img_gt_out", "depth_gt_out", "disp_out", "disp_gt_out", "depth_mask")
        dirs = {k: os.path.join(render_dir, k) for k in names}
        for d in dirs.values():
            os.makedirs(d, exist_ok=True)

        depth_img = _to_u8_range(depth_out)
        depth_img_gt = _to_u8_range(depth_gt)
        img_out = (img_out.cpu().numpy() * 255).astype(np.uint8)
        img_gt = (img_gt.squeeze(0).permute(1, 2, 0).cpu().numpy() * 255).astype(np.uint8)

        # disparity frames for better contrast
        disp_img_gt = _inferno(_to_u8_range(1 / depth_gt))
        disp_img = _inferno(_to_u8_range(1 / depth_out))

        name = str(img_idx).zfill(4)
        _write_png(os.path.join(dirs["img_out"], name + ".png"), img_out)
        _write_png(os.path.join(dirs["depth_out"], name + ".png"), depth_img)
        _write_png(os.path.join(dirs["img_gt_out"], name + ".png"), img_gt)
        _write_png(os.path.join(dirs["depth_gt_out"], name + ".png"), depth_img_gt)
        _write_png(os.path.join(dirs["disp_gt_out"], name + ".png"), disp_img_gt)
        _write_png(os.path.join(dirs["disp_out"], name + ".png"), disp_img)

        mask_rendered = (depth_out >= min_depth) & (depth_out <= max_depth)
        mask_gt = (depth_gt >= min_depth) & (depth_gt <= max_depth)
        mask = mask_rendered & mask_gt

        tp = (mask_rendered & mask_gt).reshape(1, -1)
        tn = (np.logical_not(mask_rendered) & np.logical_not(mask_gt)).reshape(1, -1)
        fp = (mask_rendered & np.logical_not(mask_gt)).reshape(1, -1)
        fn = (np.logical_not(mask_rendered) & mask_gt).reshape(1, -1)

        num_pixels = np.arange(depth_gt.shape[0] * depth_gt.shape[1]).reshape(1, -1)

        # show distribution of depth errors if set (eval_images.py:165-178)
        if show_errors:
            import matplotlib.pyplot as plt
            fig = plt.figure()
            x = (depth_gt - depth_out).reshape(1, -1)
            plt.xlim(num_pixels[0, 0], num_pixels[0, -1])
            for sel, colour in ((tp, "r"), (tn, "g"), (fp, "b"), (fn, "k")):
                plt.scatter(num_pixels[sel], x[sel], 1, colour)
            plt.legend(["True Positive", "True Negative", "False Positive", "False Negative"])
            plt.xlabel("Pixel Index")
            plt.ylabel("GT Depth - Predicted Depth (m)")
            plt.title("Classification of Depth Errors")
            plt.savefig(os.path.join(render_dir, name + "_conf.png"))
            plt.close(fig)

        # masked depth images: pixels left out of the evaluation are green, the others keep their grey
        def masked(grey):
            rb, g = grey.copy(), grey.copy()
            rb[mask == 0] = 0
            g[mask == 0] = 255
            return np.stack((rb, g, rb), axis=-1)

        mdir = dirs["depth_mask"]
        _write_png(os.path.join(mdir, name + "_mask_rendered.png"), (255 * mask_rendered).astype(np.uint8))
        _write_png(os.path.join(mdir, name + "_mask_gt.png"), (255 * mask_gt).astype(np.uint8))
        _write_png(os.path.join(mdir, name + "_mask_combined.png"), (255 * mask).astype(np.uint8))
        _write_png(os.path.join(mdir, name + "_gt.png"), masked(depth_img_gt))
        _write_png(os.path.join(mdir, name + ".png"), masked(depth_img))

        # the reference divides by num_pixels[0, -1], the last pixel INDEX = H*W - 1, not the pixel
        # count (eval_images.py:162, 217); kept, so the table matches the reference's
        conf_mat = np.array([[np.sum(tp), np.sum(fn)], [np.sum(fp), np.sum(tn)]]) / num_pixels[0, -1]
        return {"img": img_out,
                "mse": mse,
                "psnr": psnr,
                "ssim": ssim,
                "lpips": lpips_loss,
                "depth_pred": depth_out[mask],
                "depth_gt": depth_gt[mask],
                "conf_mat": conf_mat}
