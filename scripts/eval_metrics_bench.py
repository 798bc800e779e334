"""Per-frame image metrics of the novel-view evaluation at the V_KITTI frame (188 x 621), in the
layouts Eval_Images.eval_images receives -- the renderer's [H,W,3] prediction and the loader's
[1,3,H,W] ground truth:

  (a) model.metrics.image_metrics: one nerf_image_metrics call (two launches);
  (b) what the reference runs (eval_images.py:95-97): F.mse_loss plus the five-convolution torch
      expression of pytorch_ssim (:27-41) on permuted views in float32, once with the window
      built and uploaded per call as pytorch_ssim.ssim does (:86-91) and once with it cached.

Neither side reads a result back.  Each round times `--calls` warm calls of one variant between
one pair of hipEvents; the variants are interleaved over `--rounds` rounds and the medians of the
per-call times go to a JSON file, with the kernel launches per call counted by torch.profiler.
Not part of the suite or of bench.py.

With --depth the same scheme measures the depth half instead, a 188 x 621 rendered depth against a
375 x 1242 ground truth, both on the device: model.metrics.depth_metrics (one nerf_depth_metrics
call), the same with the two planes, and the host path Eval_Images.eval_images runs (.cpu(),
resize_nearest_exact, the masks, the counts, compute_errors), timed by the wall clock because its
copy synchronises.

    python scripts/eval_metrics_bench.py [--calls 100 --rounds 7 --out profiles/eval_metrics/bench.json]
    python scripts/eval_metrics_bench.py --depth [--out profiles/eval_metrics/depth_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "my-nope-nerf_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H, W = 188, 621


def launches(fn):
    """Device kernels of one call (None when the profiler gives no device events)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as exc:  # noqa: BLE001  (a count, not a measurement: report why it is missing)
        print(f"launch count unavailable: {exc!r}", file=sys.stderr)
        return None


def frame_pair(h, w, seed=0):
    """(gt [1,3,h,w], pred [h,w,3]) on the CPU: a smooth image with a saturated flat patch and a
    noisy copy of it -- the values do not matter to the time, only that the metrics are ordinary."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, h).view(h, 1).expand(h, w)
    x = torch.linspace(0, 1, w).view(1, w).expand(h, w)
    gt = torch.stack([0.5 + 0.5 * torch.sin(6 * x + 3 * y), x * y, torch.full((h, w), 0.7)]).float()
    gt[:, :h // 3, :w // 3] = 1.0
    pred = (gt + 0.05 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    return gt.unsqueeze(0).contiguous(), pred.permute(1, 2, 0).contiguous()


def gaussian_window(channels, device):
    """The 11 x 11 window as pytorch_ssim.create_window builds it (:8-17): on the CPU, then uploaded."""
    from model.metrics import gaussian_taps
    taps = gaussian_taps(11).unsqueeze(1)
    return taps.mm(taps.t()).expand(channels, 1, 11, 11).contiguous().to(device)


def torch_metrics(hwc, gt, window=None):
    """(mse, ssim) as eval_images.py:95-97 computes them; window=None builds and uploads it per call."""
    img_gt = gt.squeeze(0).permute(1, 2, 0)                  # eval_images.py:51
    mse = F.mse_loss(hwc, img_gt)
    a, b = hwc.permute(2, 0, 1).unsqueeze(0), img_gt.permute(2, 0, 1).unsqueeze(0)
    c = a.shape[1]
    if window is None:
        window = gaussian_window(c, a.device)
    mu1, mu2 = F.conv2d(a, window, padding=5, groups=c), F.conv2d(b, window, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11 = F.conv2d(a * a, window, padding=5, groups=c) - mu1_sq
    s22 = F.conv2d(b * b, window, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(a * b, window, padding=5, groups=c) - mu1_mu2
    m = ((2 * mu1_mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1_sq + mu2_sq + 1e-4) * (s11 + s22 + 9e-4))
    return mse, m.mean()


def depth_pair(h, w, gh, gw, seed=0):
    """(pred [h,w], gt [gh,gw]) on the CPU: depths 0.05 + 30 U^2, a share outside [0.1, 20], and a
    noisy bilinear copy at the render's resolution."""
    g = torch.Generator().manual_seed(seed)
    gt = (0.05 + 30.0 * torch.rand(gh, gw, generator=g) ** 2).float()
    pred = F.interpolate(gt[None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
    return (pred * torch.exp(0.25 * torch.randn(h, w, generator=g))).float().contiguous(), gt.contiguous()


def host_depth_metrics(depth_pred, depth_gt, sc, lo, hi):
    """What Eval_Images.eval_images and evaluation/eval.py:200-209 do for the depth of one frame: the
    rendered depth copied to the host, scaled, resized, both masks, the four counts and
    compute_errors in float32 (the ground truth is on the host already, as the loader leaves it)."""
    import numpy as np
    from model.common import compute_errors
    from model.metrics import resize_nearest_exact
    d = depth_pred.cpu().numpy().copy()
    d *= sc
    d = resize_nearest_exact(d, depth_gt.shape)
    mr, mg = (d >= lo) & (d <= hi), (depth_gt >= lo) & (depth_gt <= hi)
    m = mr & mg
    counts = [np.sum(m), np.sum(~mr & mg), np.sum(mr & ~mg), np.sum(~mr & ~mg)]
    return [float(v) for v in compute_errors(depth_gt[m], d[m])] + [float(c) for c in counts]


def depth_main(args):
    """--depth: (a) metrics.depth_metrics, (b) the same with the planes, (c) the host path, for a
    188 x 621 rendered depth against a 375 x 1242 ground truth, both on the device."""
    import time
    from model import _hip, metrics
    _hip.load_library()
    dev = torch.device("cuda", 0)
    gh, gw, sc, lo, hi = 375, 1242, 1.7, 0.1, 20.0
    pred_cpu, gt_cpu = depth_pair(H, W, gh, gw)
    pred, gt, gt_np = pred_cpu.to(dev), gt_cpu.to(dev), gt_cpu.numpy()
    device_variants = {"hip_depth_metrics": lambda: metrics.depth_metrics(pred, gt, lo, hi, sc=sc),
                       "hip_depth_metrics_planes": lambda: metrics.depth_metrics(pred, gt, lo, hi, sc=sc, planes=True)}
    got = metrics.depth_metrics(pred, gt, lo, hi, sc=sc).tolist()
    host = host_depth_metrics(pred, gt_np, sc, lo, hi)
    if got[7:] != host[7:] or max(abs(a - b) for a, b in zip(got[:7], host[:7])) > 1e-3:
        raise RuntimeError(f"depth metrics disagree: hip {got}, host {host}")
    for fn in device_variants.values():
        for _ in range(args.warmup):
            fn()
    for _ in range(3):
        host_depth_metrics(pred, gt_np, sc, lo, hi)
    torch.cuda.synchronize()
    times = {k: [] for k in list(device_variants) + ["host_numpy_f32"]}
    host_calls = max(1, args.calls // 20)              # milliseconds each: fewer calls per round
    for _ in range(args.rounds):
        for name, fn in device_variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            times[name].append(1e3 * a.elapsed_time(b) / args.calls)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(host_calls):
            host_depth_metrics(pred, gt_np, sc, lo, hi)      # its .cpu() waits for the device: wall clock
        times["host_numpy_f32"].append(1e6 * (time.perf_counter() - t0) / host_calls)
    res = {"shape": {"height": H, "width": W, "gt_height": gh, "gt_width": gw, "sc": sc, "min_depth": lo,
                     "max_depth": hi},
           "method": f"{args.rounds} interleaved rounds; device variants: {args.calls} warm calls between one hipEvent "
                     f"pair, no result read back; host path: {host_calls} calls by the wall clock, its device-to-host "
                     "copy included; us per call",
           "values": {"hip": dict(zip(metrics.DEPTH_METRIC_NAMES, got)),
                      "host_numpy_f32": dict(zip(metrics.DEPTH_METRIC_NAMES, host))}}
    for name, v in times.items():
        res[name] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "rounds": len(v),
                     "launches_per_call": None}
    for name, fn in device_variants.items():
        res[name]["launches_per_call"] = launches(fn)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--depth", action="store_true", help="measure the depth metrics instead (depth_bench.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.calls < 100:
        raise SystemExit("--calls: at least 100 warm calls per round")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "eval_metrics", "depth_bench.json" if args.depth else "bench.json")
    if args.depth:
        return depth_main(args)
    from model import _hip, metrics
    _hip.load_library()
    dev = torch.device("cuda", 0)
    gt, hwc = (t.to(dev) for t in frame_pair(H, W))          # [1,3,H,W] as the loader, [H,W,3] as the renderer
    window = gaussian_window(3, dev)

    variants = {"hip_image_metrics": lambda: metrics.image_metrics(hwc, gt),
                "torch_window_per_call": lambda: torch_metrics(hwc, gt),
                "torch_window_cached": lambda: torch_metrics(hwc, gt, window)}
    # the three agree before anything is timed
    ref = [float(v) for v in torch_metrics(hwc, gt, window)]
    got = metrics.image_metrics(hwc, gt).tolist()
    if abs(got[0] - ref[0]) > 1e-6 or abs(got[1] - ref[1]) > 1e-3:
        raise RuntimeError(f"metrics disagree: hip {got}, torch {ref}")
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            times[name].append(1e3 * a.elapsed_time(b) / args.calls)
    res = {"shape": {"height": H, "width": W, "channels": 3, "window": 11, "use_padding": True,
                     "prediction_layout": "[H,W,3]", "ground_truth_layout": "[1,3,H,W]"},
           "method": f"{args.rounds} interleaved rounds of {args.calls} warm calls between one hipEvent pair; "
                     "us per call, no result read back",
           "values": {"hip": {"mse": got[0], "ssim": got[1]}, "torch_f32": {"mse": ref[0], "ssim": ref[1]}}}
    for name in variants:
        v = times[name]
        res[name] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "rounds": len(v),
                     "launches_per_call": None}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    write()                                   # the times first: the profiler pass below is the fragile part
    for name, fn in variants.items():
        res[name]["launches_per_call"] = launches(fn)
    write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
