"""The geometry visualisation of one 188 x 621 frame (cfg4's size) two ways in one process:

* frame:  Renderer.phong_frame, the whole frame in one call (model/geometry.py, csrc/march.hip);
* chunks: the path before it, Renderer.forward(..., "phong_renderer") over 1024-pixel chunks, as
          Trainer.render_visdata and Extract_Images.generate_images drove it.

The field is the hand-built octahedron of tests/test_gpu_geometry.py (sigma_raw = 3 - 5 |x|_1) at hidden
256, GEMM mode f16x3, seen by the V_KITTI camera matrix from (0.15, -0.1, 2).  Both paths are warmed once,
then alternate for `--rounds` rounds; per frame: the device-synchronised wall time and the peak of
torch.cuda.memory_allocated above its level before the frame.  The two images are compared: hit-mask
flips (bar: at most 0.5 % of the pixels) and the largest rgb difference on agreeing pixels (bar: 1e-4).
`--launches` instead counts the kernel launches of one frame each way with torch.profiler, in a run of
its own (the profiler slows the host: no time is taken from it).

Not measured: graph replay of the frame, more than one GPU, trained fields.  Not part of the suite or of
bench.py.

    python scripts/geometry_frame_ab.py [--rounds 5] [--out profiles/geometry/frame_ab.json] [--launches]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FOCAL, HIDDEN = 188, 621, 362.5, 256


def octahedron_field(mdl, cfg, torch):
    """The trunk passes |x|, |y|, |z| through identity layers; the density head gives 3 - 5 |x|_1."""
    torch.manual_seed(3)
    net = mdl.OfficialStaticNerf(cfg)
    with torch.no_grad():
        for lin in list(net.layers0)[::2] + list(net.layers1)[::2]:
            lin.weight.zero_()
            lin.bias.zero_()
        w0 = net.layers0[0].weight
        for c in range(3):
            w0[2 * c, c], w0[2 * c + 1, c] = 1.0, -1.0
        for lin in list(net.layers0)[2::2] + list(net.layers1)[::2]:
            for i in range(6):
                lin.weight[i, i] = 1.0
        net.fc_density.weight.zero_()
        net.fc_density.weight[0, :6] = -5.0
        net.fc_density.bias.fill_(3.0)
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "my-nope-nerf_amd"))
    import torch
    import model as mdl
    from model import _hip
    from model.common import arange_pixels
    from model.synthetic import camera_K, make_cfg
    _hip.load_library()
    _hip.gemm_set_precision(2)
    dev = torch.device("cuda", 0)
    cfg = make_cfg(hidden=HIDDEN, S=128)
    rnd = mdl.Renderer(octahedron_field(mdl, cfg, torch), cfg["rendering"], device=dev)
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.15, -0.1, 2.0])
    K, w2c, S = camera_K(H, W, FOCAL, FOCAL).to(dev), torch.inverse(c2w).unsqueeze(0).to(dev), torch.eye(4).unsqueeze(0).to(dev)
    pix = arange_pixels(resolution=(H, W), device=dev)[1]

    def frame():
        return rnd.phong_frame(pix, K, w2c, S, 0)["rgb"]

    def chunks():
        with torch.no_grad():
            return torch.cat([rnd(p, None, K, w2c, S, "phong_renderer", eval_=True, it=0, add_noise=False)["rgb"]
                              for p in torch.split(pix, 1024, dim=1)], dim=1)

    paths = {"frame": frame, "chunks": chunks}
    res = {"frame_hw": [H, W], "hidden": HIDDEN, "gemm_precision": 2, "field": "octahedron 3 - 5 |x|_1",
           "device": torch.cuda.get_device_name(0), "not_measured": ["graph replay", "multi-GPU", "trained fields"]}
    if args.launches:
        from torch.profiler import ProfilerActivity, profile
        for name, fn in paths.items():
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                    and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
            res[f"launches_per_frame_{name}"] = n or None
            print(f"{name}: {n} kernel launches per frame", flush=True)
    else:
        imgs = {}
        for name, fn in paths.items():                      # warm-up of both
            imgs[name] = fn()
            torch.cuda.synchronize()
            print(f"warm-up {name} done", flush=True)
        ms = {n: [] for n in paths}
        peak = {n: [] for n in paths}
        for r in range(args.rounds):
            for name, fn in paths.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                ms[name].append(1e3 * (time.perf_counter() - t0))
                peak[name].append(torch.cuda.max_memory_allocated() - base)
                del out
            print(f"round {r}: frame {ms['frame'][-1]:.1f} ms, chunks {ms['chunks'][-1]:.1f} ms", flush=True)
        a, b = imgs["frame"][0], imgs["chunks"][0]
        hit_a, hit_b = ~(a == 1).all(-1), ~(b == 1).all(-1)
        same = hit_a == hit_b
        res.update({
            "rounds": args.rounds,
            "ms_per_frame": {n: [round(v, 2) for v in ms[n]] for n in paths},
            "ms_per_frame_median": {n: round(statistics.median(ms[n]), 2) for n in paths},
            "frame_faster_in_every_round": all(x < y for x, y in zip(ms["frame"], ms["chunks"])),
            "peak_bytes_above_start": {n: max(peak[n]) for n in paths},
            "pixels": H * W, "hits_frame": int(hit_a.sum()), "hits_chunks": int(hit_b.sum()),
            "mask_flips": int((~same).sum()), "mask_flip_cap": int(0.005 * H * W),
            "max_rgb_diff_on_agreeing_pixels": float((a[same] - b[same]).abs().max()), "rgb_bar": 1e-4})
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        old = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
        old.update(res)
        with open(args.out, "w") as f:
            json.dump(old, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
