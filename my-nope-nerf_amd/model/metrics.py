"""Image metrics of the novel-view evaluation (evaluation/eval.py:146-221 through
model/eval_images.py:94-107): MSE, the 11 x 11 Gaussian SSIM of
third_party/pytorch_ssim/__init__.py:8-46 and the nearest-exact depth resize.

``ssim`` has pytorch_ssim.ssim's signature and return (:76-93).  CUDA float32 tensors of any
strides go through nerf_image_metrics (csrc/metrics.hip): one call, two launches, no permuted
copy, no host synchronisation, repeatable bits.  CPU tensors -- the host-side tests of the
evaluation glue -- use the torch expression below (ssim_map_torch and its mean).  A CUDA tensor of another dtype is an error,
not a fallback.

``depth_metrics`` is the depth half (eval_images.py:105-107, 152-160, 200-201 and compute_errors,
common.py:676-694) on the same terms: nerf_depth_metrics for CUDA float32 tensors, a torch fp64
expression of the same definition for CPU tensors.
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


DEPTH_METRIC_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "tp", "fn", "fp", "tn")


def _depth_metrics_torch(pred, gt, sc, min_depth, max_depth):
    """The definition of nerf_depth_metrics (include/nerf_hip.h) as a torch expression on [B,h,w] /
    [B,H,W] tensors: the selection in float32 as numpy makes it, the sums in float64.  The path of
    CPU tensors -> (out [B,11] float64, depth [B,H,W] float32, mask [B,H,W] uint8)."""
    f32 = dict(dtype=torch.float32, device=pred.device)
    (h, w), (gh, gw) = pred.shape[1:], gt.shape[1:]
    iy = torch.clamp(((2 * torch.arange(gh, device=pred.device) + 1) * h) // (2 * gh), max=h - 1)
    ix = torch.clamp(((2 * torch.arange(gw, device=pred.device) + 1) * w) // (2 * gw), max=w - 1)
    d = (pred.to(torch.float32) * torch.tensor(sc, **f32))[:, iy[:, None], ix[None, :]]
    g = gt.to(torch.float32)
    lo, hi = torch.tensor(min_depth, **f32), torch.tensor(max_depth, **f32)
    mr, mg = (d >= lo) & (d <= hi), (g >= lo) & (g <= hi)
    rows = []
    for b in range(pred.shape[0]):
        sel = mr[b] & mg[b]
        g64, d64 = g[b][sel].double(), d[b][sel].double()
        ratio = torch.maximum(g64 / d64, d64 / g64)
        tp = sel.sum().double()
        diff = g64 - d64
        sums = torch.stack([(diff.abs() / g64).sum(), (diff * diff / g64).sum(), (diff * diff).sum(),
                            (g64.log() - d64.log()).square().sum()] +
                           [(ratio < 1.25 ** k).sum().double() for k in (1, 2, 3)])
        means = sums / tp                                       # 0 / 0 = NaN without a selected pixel
        means[2:4] = means[2:4].sqrt()
        counts = torch.stack([sel.sum(), (~mr[b] & mg[b]).sum(), (mr[b] & ~mg[b]).sum(), (~mr[b] & ~mg[b]).sum()])
        rows.append(torch.cat([means, counts.double()]))
    return torch.stack(rows), d.contiguous(), mr.to(torch.uint8) | (mg.to(torch.uint8) << 1)


def depth_metrics(pred, gt, min_depth, max_depth, sc=1.0, planes=False):
    """The depth half of the evaluation (eval_images.py:105-107, 152-160, 200-201 and compute_errors,
    common.py:676-694) for a rendered depth [h,w] or [B,h,w] against a ground truth [H,W] or [B,H,W]:
    pred * sc resampled to the ground truth's grid by pixel-centre nearest neighbour, both
    [min_depth, max_depth] masks, and over the pixels in range in both the seven errors.  Returns a
    float64 [11] (both inputs 2-D) or [B,11] tensor on the inputs' device, DEPTH_METRIC_NAMES in order:
    means over the tp pixels (NaN without one) and the four confusion counts.  planes=True also
    returns (depth_out float32, mask uint8: bit 0 the rendered depth in range, bit 1 the ground truth),
    shaped as gt.  CUDA float32 tensors of any strides go through nerf_depth_metrics: one call, two
    launches, no resized copy, no host synchronisation, repeatable bits.  CPU tensors use the torch
    expression above; a CUDA tensor of another dtype is an error."""
    single = pred.dim() == 2 and gt.dim() == 2
    p3 = pred.unsqueeze(0) if pred.dim() == 2 else pred
    g3 = gt.unsqueeze(0) if gt.dim() == 2 else gt
    if p3.dim() != 3 or g3.dim() != 3 or p3.shape[0] != g3.shape[0] or 0 in p3.shape or 0 in g3.shape:
        raise ValueError(f"depth_metrics: [h,w] or [B,h,w] against [H,W] or [B,H,W] expected, got {tuple(pred.shape)} "
                         f"and {tuple(gt.shape)}")
    if p3.device != g3.device:
        raise ValueError(f"both depths must live on one device, got {p3.device} and {g3.device}")
    if not (math.isfinite(sc) and min_depth > 0 and max_depth >= min_depth):
        raise ValueError(f"depth_metrics: a finite sc and 0 < min_depth <= max_depth expected, got sc={sc}, "
                         f"min_depth={min_depth}, max_depth={max_depth}")
    if p3.is_cuda:
        if p3.dtype != torch.float32 or g3.dtype != torch.float32:
            raise RuntimeError(f"depth metrics: CUDA tensors must be float32, got {p3.dtype} and {g3.dtype}")
        n, gh, gw = g3.shape
        out = torch.empty(n, 11, dtype=torch.float64, device=p3.device)
        work = torch.empty(_hip.depth_metrics_workspace_bytes(n, gh, gw), dtype=torch.uint8, device=p3.device)
        depth = torch.empty(n, gh, gw, dtype=torch.float32, device=p3.device) if planes else None
        mask = torch.empty(n, gh, gw, dtype=torch.uint8, device=p3.device) if planes else None
        _hip.depth_metrics(p3, g3, sc, min_depth, max_depth, out, work, depth, mask)
    else:
        out, depth, mask = _depth_metrics_torch(p3, g3, float(sc), float(min_depth), float(max_depth))
    if gt.dim() == 2:
        depth, mask = (None, None) if depth is None else (depth[0], mask[0])
    out = out[0] if single else out
    return (out, depth, mask) if planes else out


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
