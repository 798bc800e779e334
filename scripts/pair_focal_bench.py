"""The config-3 training step (Trainer.train_step on the two-view synthetic V_KITTI scene: 188 x 621,
1024 rays x 128 samples, D = 256, pose + distortion learning, 47 x 155 pair grid) with a learned focal
length (LearnFocal and its Adam, pose.learn_focal) and with a fixed one, in one tree or in two.

With a learned focal a tree that has nerf_pair_backward_cam runs the pair terms on csrc/pair.hip (4 + 4
launches, the camera-matrix gradient from the same backward launches); a tree without it (the commit
before) keeps the torch expressions for that setting: ATen point clouds and reprojection and the (3, P, P)
chamfer differences with their autograd.

Each measurement is a fresh process (its own Trainer, warmed), timing `--steps` steps between one pair of
hipEvents, the two cameras alternating; the settings (and trees) are interleaved over `--rounds` rounds
and the medians of the per-step times go to a JSON file, with the device kernels of one step counted by
torch.profiler in the last round.  Not measured: graph replay, more than one GPU, real frames.  Not part
of the suite or of bench.py.

    python scripts/pair_focal_bench.py [--steps 50 --rounds 5 --out profiles/pair_focal/bench.json]
                                       [--tree parent=/path/to/other/checkout ...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FOCAL, RAYS, SAMPLES, HIDDEN = 188, 621, 362.5, 1024, 128, 256


def child(args):
    """One setting in this process: build, warm, time; print one JSON line."""
    sys.path.insert(0, os.path.join(args.child, "my-nope-nerf_amd"))
    import torch
    import model as mdl
    from model import _hip
    from model.optim import HipAdam
    from model.synthetic import make_cfg, vkitti_pair_scene
    _hip.load_library()
    dev = torch.device("cuda", 0)
    cfg = make_cfg(hidden=HIDDEN, S=SAMPLES)
    t = cfg["training"]
    t["n_training_points"] = RAYS
    t["annealing_epochs"], t["scheduling_start"] = 2000, 0
    datas, c2w = vkitti_pair_scene(dev, H, W, FOCAL)
    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    nn_model = mdl.get_model(mdl.Renderer(net, cfg["rendering"], device=dev), cfg, device=dev)
    pose = mdl.LearnPose(2, True, True, cfg, init_c2w=c2w.clone()).to(dev)
    distn = mdl.Learn_Distortion(2, True, True, cfg).to(dev)
    kw = {}
    if args.learn_focal:
        K = datas[0]["img.camera_mat"]
        focal = mdl.LearnFocal(True, False, order=2, init_focal=[K[0, 0, 0].item(), -K[0, 1, 1].item()]).to(dev)
        kw = dict(focal_net=focal, optimizer_focal=torch.optim.Adam(focal.parameters(), lr=1e-3, fused=True))
    tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), t, device=dev,
                     optimizer_pose=torch.optim.Adam(pose.parameters(), lr=5e-4, fused=True), pose_param_net=pose,
                     optimizer_distortion=torch.optim.Adam(distn.parameters(), lr=5e-4, fused=True),
                     distortion_net=distn, **kw)
    routed = []
    inner = tr._reference_terms

    def spy(*a, **k):                         # did the step take the pair kernels?
        o = inner(*a, **k)
        routed.append("pair_losses" in o)
        return o

    tr._reference_terms = spy

    def one(i):
        return tr.train_step(datas[i % 2], it=i + 1, epoch=0, scheduling_start=0)

    for i in range(args.warmup):
        out = one(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(args.steps):
        out = one(args.warmup + i)
    b.record()
    b.synchronize()
    res = {"step_ms": a.elapsed_time(b) / args.steps, "pair_kernels": all(routed) and bool(routed),
           "loss_rgb_s": float(out["loss_rgb_s"]), "loss_pc": float(out["loss_pc"]),
           "focalx": float(out["focalx"].detach()) if "focalx" in out else None, "launches_per_step": None}
    if args.count_launches:
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                one(args.warmup + args.steps)
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                    and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
            res["launches_per_step"] = n or None
        except Exception as exc:  # noqa: BLE001  (a count, not a measurement: report why it is missing)
            print(f"launch count unavailable: {exc!r}", file=sys.stderr)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tree", action="append", default=[], metavar="NAME=DIR",
                    help="another checkout (built) to measure beside this one, learned focal only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_focal", "bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--learn-focal", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--count-launches", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = [("this_tree", ROOT, True), ("this_tree", ROOT, False)]
    for spec in args.tree:
        name, path = spec.split("=", 1)
        runs.append((name, os.path.abspath(path), True))
    times = {(n, s): [] for n, _, s in runs}
    last = {}
    for r in range(args.rounds):
        for name, path, s in runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--learn-focal", str(int(s)),
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            if r == args.rounds - 1:
                cmd.append("--count-launches")
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                raise SystemExit(f"{name} learn_focal={s}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            last[name, s] = json.loads(line[-1][7:])
            times[name, s].append(last[name, s]["step_ms"])
            print(f"round {r} {name} learn_focal={s}: {times[name, s][-1]:.3f} ms/step", flush=True)
    res = {"shape": {"height": H, "width": W, "rays": RAYS, "samples": SAMPLES, "hidden": HIDDEN, "pair_grid": [47, 155]},
           "method": f"fresh process per measurement, {args.warmup} warm-up steps, {args.steps} steps between one "
                     f"hipEvent pair, {args.rounds} interleaved rounds; median ms per Trainer.train_step",
           "not_measured": ["graph replay", "more than one GPU", "real frames"]}
    for name, _, s in runs:
        v = times[name, s]
        res.setdefault(name, {})[f"learn_focal_{s}"] = {
            "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "per_round_ms": v,
            "pair_kernels": last[name, s]["pair_kernels"], "launches_per_step": last[name, s]["launches_per_step"],
            "loss_rgb_s": last[name, s]["loss_rgb_s"], "loss_pc": last[name, s]["loss_pc"],
            "focalx": last[name, s]["focalx"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
