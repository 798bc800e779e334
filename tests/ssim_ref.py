"""The checker of the Gaussian SSIM tests: a restatement of the reference's
third_party/pytorch_ssim/__init__.py:8-46 that runs in any dtype, and the seeded test images.

The window is built as the reference builds it (:8-17): a float32 1-D Gaussian, normalised in
float32, its float32 outer product, and only then the cast to the dtype of the run.  In float64
this is the truth the tests measure against; in float32 it is the reference's own result, whose
distance from the truth sets the bar (tests.helpers.tight_bar).
"""
from __future__ import annotations

import functools
from math import exp

import torch
import torch.nn.functional as F

SHAPES = [(1, 1), (7, 9), (11, 11), (33, 45), (64, 96), (188, 621)]


def ref_window(window_size: int, channel: int, dtype, device="cpu"):
    """create_window (:13-17) on gaussian(window_size, 1.5) (:8-10)."""
    gauss = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)],
                         dtype=torch.float32)
    g1 = (gauss / gauss.sum()).unsqueeze(1)
    w2 = g1.mm(g1.t()).float().unsqueeze(0).unsqueeze(0)
    return w2.expand(channel, 1, window_size, window_size).contiguous().to(device=device, dtype=dtype)


def ssim_map_ref(img1, img2, window_size=11, use_padding=True, dtype=torch.float64):
    """The map of _ssim (:20-41) for [B,C,H,W] images, computed in `dtype` on img1's device."""
    img1, img2 = img1.to(dtype), img2.to(dtype)
    channel = img1.shape[1]
    window = ref_window(window_size, channel, dtype, img1.device)
    pad = window_size // 2 if use_padding else 0                                 # :22-25
    mu1 = F.conv2d(img1, window, padding=pad, groups=channel)                    # :27
    mu2 = F.conv2d(img2, window, padding=pad, groups=channel)                    # :28
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2                  # :30-32
    sigma1_sq = F.conv2d(img1 * img1, window, padding=pad, groups=channel) - mu1_sq    # :34
    sigma2_sq = F.conv2d(img2 * img2, window, padding=pad, groups=channel) - mu2_sq    # :35
    sigma12 = F.conv2d(img1 * img2, window, padding=pad, groups=channel) - mu1_mu2     # :36
    C1, C2 = 0.01 ** 2, 0.03 ** 2                                                # :38-39
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))  # :41


def mean_per_image(ssim_map):
    """size_average=False (:46)."""
    return ssim_map.mean(1).mean(1).mean(1)


@functools.lru_cache(maxsize=None)
def make_pair(h: int, w: int, seed: int = 0):
    """(gt, pred), float32 [1,3,h,w] on the CPU: a smooth channel 0.5 + 0.5 sin(6x + 3y), a ramp
    x y, a constant 0.7, and a saturated flat patch of ones over the top-left third of every
    channel; pred = clamp(gt + 0.05 N(0,1), 0, 1) with the same flat patch.  Flat bright regions
    exercise the E[x^2] - mu^2 cancellation, the border the zero padding, the noise low SSIM."""
    y = torch.linspace(0, 1, h).view(h, 1).expand(h, w)
    x = torch.linspace(0, 1, w).view(1, w).expand(h, w)
    gt = torch.stack([0.5 + 0.5 * torch.sin(6 * x + 3 * y), x * y, torch.full((h, w), 0.7)]).float()
    gt[:, :h // 3, :w // 3] = 1.0
    g = torch.Generator().manual_seed(1000 * seed + 7)
    pred = (gt + 0.05 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    pred[:, :h // 3, :w // 3] = 1.0
    return gt.unsqueeze(0).contiguous(), pred.unsqueeze(0).contiguous()
