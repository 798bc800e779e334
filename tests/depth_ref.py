"""The checker of the depth-metric tests: a numpy restatement of the reference's depth evaluation
(model/eval_images.py:105-107, 152-160, 200-201 and compute_errors, model/common.py:676-694) that
sums in any dtype, and the seeded and crafted inputs.

The selection is made in float32 exactly as the reference makes it: the rendered depth scaled by
a float32 multiply, resampled by pixel-centre nearest neighbour, both masks by float32 comparisons.
The sums run through the unchanged model.common.compute_errors on the selected values cast to
`dtype`: float64 is the truth the tests measure against, float32 the reference's own arithmetic.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from model.common import compute_errors
from model.metrics import resize_nearest_exact

# (h, w, H, W): one pixel, non-integer up- and down-sampling, identity, large upsampling, the evaluation's own
SHAPES = [(1, 1, 1, 1), (5, 7, 11, 13), (47, 155, 23, 61), (33, 45, 33, 45), (7, 9, 64, 96), (188, 621, 375, 1242)]
SCALES = (1.0, 1.7)
LO, HI = 0.1, 20.0
THRESHOLDS = (1.25, 1.5625, 1.953125)
RATIO_GAP = 1e-6                       # no selected pixel has max(g/d, d/g) this close (relative) to a threshold
# a shape whose default seed (1000 h + w) breaks a condition of assert_conditions has another one here
DEPTH_SEEDS = {(188, 621, 375, 1242): 4188621}     # 188621: a ratio 5.1e-7 from a threshold at sc = 1


def select(pred, gt, sc, lo, hi):
    """(d, g, mr, mg): the scaled, resampled rendered depth [H,W] f32, the ground truth f32 and the
    two range masks, as eval_images.py:105-107, 152-153 forms them."""
    d = np.array(pred, dtype=np.float32, copy=True)
    d *= np.float32(sc)                                       # depth_out *= sc on a float32 array
    g = np.asarray(gt, dtype=np.float32)
    d = resize_nearest_exact(d, g.shape)
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        mr, mg = (d >= lo) & (d <= hi), (g >= lo) & (g <= hi)
    return d, g, mr, mg


def errors(g_sel, d_sel, dtype):
    """compute_errors on the selected values in `dtype`; seven NaNs for an empty selection (numpy's
    mean of nothing, without its warning)."""
    if g_sel.size == 0:
        return np.full(7, np.nan)
    return np.array([float(v) for v in compute_errors(g_sel.astype(dtype), d_sel.astype(dtype))], dtype=np.float64)


def depth_metrics_ref(pred, gt, sc, lo, hi, dtype=np.float64):
    """{"out": [11] float64 (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, tp, fn, fp, tn), "depth": d,
    "mask": uint8 (bit 0 = rendered in range, bit 1 = ground truth in range), "sel": tp mask}."""
    d, g, mr, mg = select(pred, gt, sc, lo, hi)
    sel = mr & mg
    counts = [sel.sum(), (~mr & mg).sum(), (mr & ~mg).sum(), (~mr & ~mg).sum()]
    out = np.concatenate([errors(g[sel], d[sel], dtype), np.array(counts, dtype=np.float64)])
    return {"out": out, "depth": d, "mask": mr.astype(np.uint8) | (mg.astype(np.uint8) << 1), "sel": sel}


@functools.lru_cache(maxsize=None)
def make_depth_pair(h, w, H, W, seed=None):
    """(pred [h,w], gt [H,W]) float32 CPU tensors: gt = 0.05 + 30 U^2 (a share below 0.1, a share above
    20), pred = gt resampled bilinearly to h x w times exp(0.25 N(0,1)); for h w >= 8 the pixels 1, 3,
    5, 7 of pred (row-major) hold 0, NaN, +inf and -1."""
    seed = DEPTH_SEEDS.get((h, w, H, W), 1000 * h + w) if seed is None else seed
    gen = torch.Generator().manual_seed(seed)
    gt = (0.05 + 30.0 * torch.rand(H, W, generator=gen) ** 2).float()
    pred = F.interpolate(gt[None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
    pred = (pred * torch.exp(0.25 * torch.randn(h, w, generator=gen))).float().contiguous()
    if h * w >= 8:
        flat = pred.view(-1)
        flat[1], flat[3], flat[5], flat[7] = 0.0, float("nan"), float("inf"), -1.0
    return pred, gt.contiguous()


def threshold_gap(g_sel, d_sel):
    """The smallest relative distance of max(g/d, d/g) (fp64) to one of the three thresholds."""
    g, d = g_sel.astype(np.float64), d_sel.astype(np.float64)
    r = np.maximum(g / d, d / g)
    return min(float(np.abs(r / t - 1.0).min()) for t in THRESHOLDS) if r.size else float("inf")


def assert_conditions(pair, scales=SCALES, lo=LO, hi=HI):
    """The conditions under which an fp64 evaluation in any order decides every pixel as the truth
    does: a non-empty selection, all four confusion cells populated for h w >= 35, and no selected
    ratio within RATIO_GAP of a threshold."""
    pred, gt = pair
    for sc in scales:
        ref = depth_metrics_ref(pred.numpy(), gt.numpy(), sc, lo, hi)
        tp, fn, fp, tn = ref["out"][7:]
        assert tp >= 1, ("empty selection", tuple(pred.shape), sc)
        if pred.numel() >= 35:
            assert min(tp, fn, fp, tn) >= 1, ("empty confusion cell", tuple(pred.shape), sc, (tp, fn, fp, tn))
        gap = threshold_gap(gt.numpy()[ref["sel"]], ref["depth"][ref["sel"]])
        assert gap >= RATIO_GAP, ("ratio at a threshold", tuple(pred.shape), sc, gap)


def crafted_pair():
    """(pred, gt) [4,4] with exact boundary values (sc = 1, bounds LO / HI, identity resample):
    both depths exactly at fl32(0.1) and exactly at 20 (in range); one f32 step below and above, on
    either side (out of range); ratios of exactly 1.25 (both ways round), 1.5625 and 1.953125, which
    the strict < does not count; a ratio of exactly 1; 0, NaN, -1 and 25 out of range in both."""
    lo, hi = np.float32(LO), np.float32(HI)
    below, above = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
    nan = np.float32("nan")
    gd = [(lo, lo), (hi, hi), (below, 1), (above, 1),            # tp, tp, fp, fp
          (1, below), (1, above), (4, 5), (5, 4),                 # fn, fn, ratio 1.25, ratio 1.25
          (4, 6.25), (8, 15.625), (2, 2), (3, 7),                 # 1.5625, 1.953125, 1, 2.33
          (0, nan), (25, -1), (10, 11), (0.5, 0.45)]              # tn, tn, 1.1, 1.11
    gt = torch.tensor([float(g) for g, _ in gd], dtype=torch.float32).view(4, 4)
    pred = torch.tensor([float(d) for _, d in gd], dtype=torch.float32).view(4, 4)
    assert gt[0, 0].item() == float(lo) and gt[0, 2].item() == float(below) and gt[0, 3].item() == float(above)
    return pred, gt


# at sc = 1: ten selected pixels, five of them below 1.25, seven below 1.5625, eight below 1.953125
CRAFTED_COUNTS = dict(tp=10, fn=2, fp=2, tn=2, a1=0.5, a2=0.7, a3=0.8)


def check_against_ref(out, ref_out, where=""):
    """The pass condition of both modules: counts and a1..a3 exactly the fp64 restatement's, the four
    continuous metrics within 2^-30 max(1, |ref|) (at most 2^20 non-negative fp64 summands, each a few
    ulp off: within about n 2^-53 + 2^-50 < 2^-33 relative in any order; the bar leaves 8 x over that).
    NaNs must sit where the restatement's are.  -> the largest |got - ref| of the four."""
    out, ref_out = np.asarray(out, dtype=np.float64), np.asarray(ref_out, dtype=np.float64)
    assert out.shape == ref_out.shape == (11,), (where, out.shape)
    assert np.array_equal(out[7:], ref_out[7:]), (where, "counts", out[7:], ref_out[7:])
    assert np.array_equal(np.isnan(out), np.isnan(ref_out)), (where, "NaN pattern", out, ref_out)
    if np.isnan(ref_out[:7]).any():
        return 0.0
    assert np.array_equal(out[4:7], ref_out[4:7]), (where, "a1..a3", out[4:7], ref_out[4:7])
    err = np.abs(out[:4] - ref_out[:4])
    bar = 2.0 ** -30 * np.maximum(1.0, np.abs(ref_out[:4]))
    assert (err <= bar).all(), (where, "continuous metrics", out[:4], ref_out[:4], err, bar)
    return float(err.max())
