"""Image metrics of the novel-view evaluation (evaluation/eval.py:146-221 through
model/eval_images.py:94-107): MSE, the 11 x 11 Gaussian SSIM of
third_party/pytorch_ssim/__init__.py:8-46 and the nearest-exact depth resize.

``ssim`` has pytorch_ssim.ssim's signature and return (:76-93).  CUDA float32 tensors of any
strides go through nerf_image_metrics (csrc/metrics.hip): one call, two launches, no permuted
copy, no host synchronisation, repeatable bits.  CPU tensors -- the host-side tests of the
evaluation glue -- use the torch expression below (ssim_map_torch and its mean).  A CUDA tensor of another dtype is an error,
not a fallback.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip

SSIM_C1 = 0.01 ** 2
SSIM_C2 = 0.03 ** 2
SSIM_SIGMA = 1.5


def _check_window(window_size):
    if window_size % 2 != 1 or not 1 <= window_size <= 11:
        raise ValueError(f"ssim: window_size={window_size} must be odd, 1..11")


def gaussian_taps(window_size: int) -> torch.Tensor:
    """The normalised float32 taps exp(-(k - window // 2)^2 / (2 sigma^2)), sigma = 1.5."""
    half = window_size // 2
    taps = torch.tensor([math.exp(-((k - half) ** 2) / (2.0 * SSIM_SIGMA ** 2)) for k in range(window_size)],
                        dtype=torch.float32)
    return taps / taps.sum()


def ssim_map_torch(a, b, use_padding=True, window_size=11):
    """The SSIM map [B,C,H',W'] of two [B,C,H,W] tensors as a torch expression (any device, a's
    dtype): the five windowed moments as depthwise convolutions with the outer product of the
    taps.  The path of CPU tensors; CUDA float32 tensors go through the kernel."""
    c = a.shape[1]
    taps = gaussian_taps(window_size)
    kernel = torch.outer(taps, taps).to(device=a.device, dtype=a.dtype).expand(c, 1, window_size, window_size)
    pad = window_size // 2 if use_padding else 0

    def blur(t):
        return F.conv2d(t, kernel, padding=pad, groups=c)

    mean_a, mean_b = blur(a), blur(b)
    var_a = blur(a * a) - mean_a * mean_a
    var_b = blur(b * b) - mean_b * mean_b
    cov = blur(a * b) - mean_a * mean_b
    luminance = (2 * mean_a * mean_b + SSIM_C1) / (mean_a * mean_a + mean_b * mean_b + SSIM_C1)
    structure = (2 * cov + SSIM_C2) / (var_a + var_b + SSIM_C2)
    return luminance * structure


def _ssim_means_torch(a, b, use_padding, window_size):
    """Per-image mean of ssim_map_torch."""
    return ssim_map_torch(a, b, use_padding, window_size).mean(dim=(1, 2, 3))


def _metrics_hip(a, b, use_padding, window_size):
    """[B][2] = (mse, ssim) per image of two CUDA float32 [B,C,H,W] views."""
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError(f"image metrics: CUDA tensors must be float32, got {a.dtype} and {b.dtype}")
    n, c, h, w = a.shape
    out = torch.empty(n, 2, dtype=torch.float32, device=a.device)
    work = torch.empty(_hip.image_metrics_workspace_bytes(n, c, h, w), dtype=torch.uint8, device=a.device)
    _hip.image_metrics(a, b, window_size, use_padding, out, work)
    return out


def _check_pair(img1, img2):
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError(f"two [B,C,H,W] tensors of one shape expected, got {tuple(img1.shape)} and "
                         f"{tuple(img2.shape)}")
    if img1.device != img2.device:
        raise ValueError(f"both images must live on one device, got {img1.device} and {img2.device}")


def ssim(img1, img2, use_padding=True, window_size=11, size_average=True):
    """pytorch_ssim.ssim (:76-93): the SSIM of two [B,C,H,W] images in [0, 1], averaged over
    everything (a scalar tensor) or, with size_average=False, per image ([B])."""
    _check_window(window_size)
    _check_pair(img1, img2)
    if img1.is_cuda:
        per_image = _metrics_hip(img1, img2, use_padding, window_size)[:, 1]
    else:
        per_image = _ssim_means_torch(img1, img2, use_padding, window_size)
    return per_image.mean() if size_average else per_image


def image_metrics(pred_hwc, gt):
    """(mse, ssim) of one frame as a [2] tensor on the inputs' device: the renderer's [H,W,3]
    prediction against the loader's [1,3,H,W] or [3,H,W] ground truth, both read as they come."""
    if pred_hwc.dim() != 3:
        raise ValueError(f"image_metrics: an [H,W,C] prediction expected, got {tuple(pred_hwc.shape)}")
    pred = pred_hwc.permute(2, 0, 1).unsqueeze(0)          # a view: no copy
    if gt.dim() == 3:
        gt = gt.unsqueeze(0)
    _check_pair(pred, gt)
    if pred.is_cuda:
        return _metrics_hip(pred, gt, True, 11)[0]
    return torch.stack([(pred - gt).square().mean(), _ssim_means_torch(pred, gt, True, 11)[0]])


def resize_nearest_exact(depth, size):
    """Pixel-centre nearest neighbour of a [h,w] array to size = (rows, columns):
    src = min(floor((dst + 0.5) * src_size / dst_size), src_size - 1), in integers -- what
    cv2.INTER_NEAREST_EXACT (eval_images.py:107) and torch's "nearest-exact" pick."""
    depth = np.asarray(depth)
    rows, cols = int(size[0]), int(size[1])
    h, w = depth.shape[:2]
    iy = np.minimum(((2 * np.arange(rows, dtype=np.int64) + 1) * h) // (2 * rows), h - 1)
    ix = np.minimum(((2 * np.arange(cols, dtype=np.int64) + 1) * w) // (2 * cols), w - 1)
    return depth[iy[:, None], ix[None, :]]
