"""The config-3 training step (Trainer.train_step on the two-view synthetic V_KITTI scene: 188 x 621,
1024 rays x 128 samples, D = 256, pose + distortion learning, 47 x 155 pair grid) with
training.with_ssim True and False, in one tree or in two.

With with_ssim True a tree that has nerf_pair_forward_ssim runs the pair terms on csrc/pair.hip
(5 + 4 launches); a tree without it (the commit before) keeps the torch expressions for that setting:
ATen point clouds and reprojection, the (3, P, P) chamfer differences, five AvgPool2d and their autograd.

Each measurement is a fresh process (its own Trainer, warmed), timing `--steps` steps between one pair of
hipEvents, the two cameras alternating; the settings (and trees) are interleaved over `--rounds` rounds
and the medians of the per-step times go to a JSON file, with the device kernels of one step counted by
torch.profiler in the last round and, from the last round too, the time of pair_losses alone (forward +
backward at 47 x 155).  Not part of the suite or of bench.py.

    python scripts/pair_ssim_bench.py [--steps 50 --rounds 5 --out profiles/pair_ssim/bench.json]
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
    t["with_ssim"] = bool(args.with_ssim)
    datas, c2w = vkitti_pair_scene(dev, H, W, FOCAL)
    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    nn_model = mdl.get_model(mdl.Renderer(net, cfg["rendering"], device=dev), cfg, device=dev)
    pose = mdl.LearnPose(2, True, True, cfg, init_c2w=c2w.clone()).to(dev)
    distn = mdl.Learn_Distortion(2, True, True, cfg).to(dev)
    tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), t, device=dev,
                     optimizer_pose=torch.optim.Adam(pose.parameters(), lr=5e-4, fused=True), pose_param_net=pose,
                     optimizer_distortion=torch.optim.Adam(distn.parameters(), lr=5e-4, fused=True),
                     distortion_net=distn)
    routed = []
    inner = tr._reference_terms

    def spy(*a, **kw):                        # did the step take the pair kernels?
        o = inner(*a, **kw)
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
           "loss_rgb_s": float(out["loss_rgb_s"]), "loss_pc": float(out["loss_pc"]), "launches_per_step": None}
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
    res["pair_losses_us"] = pair_alone(dev, bool(args.with_ssim))
    print("RESULT " + json.dumps(res))


def pair_alone(dev, with_ssim, calls=200):
    """us per pair_losses forward + backward at the 47 x 155 grid on random inputs, one hipEvent pair around
    `calls` warm calls; None where the tree's pair_losses has no with_ssim."""
    import inspect
    import torch
    from model.pair import pair_losses
    kw = {}
    if with_ssim:
        if "with_ssim" not in inspect.signature(pair_losses).parameters:
            return None
        kw["with_ssim"] = True
    h, w = 47, 155
    g = torch.Generator().manual_seed(0)
    d1, d2 = (2.0 + 3.0 * torch.rand(1, 1, h, w, generator=g) for _ in range(2))
    i1, i2 = (torch.rand(1, 3, h, w, generator=g).to(dev) for _ in range(2))
    K = torch.diag(torch.tensor([1.5, -1.5, -1.0, 1.0])).view(1, 4, 4).to(dev)
    Rt = torch.eye(4)
    Rt[:3, 3] = torch.tensor([0.05, -0.02, 0.3])
    leaves = [t.to(dev).requires_grad_(True) for t in (d1, d2, Rt.view(1, 4, 4))]

    def one():
        l_pc, l_rgbs = pair_losses(leaves[0], leaves[1], K, leaves[2], None, i1, i2, (h, w), 0.01, **kw)
        (l_pc + l_rgbs).backward()

    for _ in range(20):
        one()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        one()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tree", action="append", default=[], metavar="NAME=DIR",
                    help="another checkout (built) to measure beside this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_ssim", "bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--with-ssim", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--count-launches", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    trees = {"this_tree": ROOT}
    for spec in args.tree:
        name, path = spec.split("=", 1)
        trees[name] = os.path.abspath(path)
    runs = [(name, path, s) for name, path in trees.items() for s in (True, False)]
    times = {(n, s): [] for n, _, s in runs}
    last = {}
    for r in range(args.rounds):
        for name, path, s in runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--with-ssim", str(int(s)),
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            if r == args.rounds - 1:
                cmd.append("--count-launches")
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                raise SystemExit(f"{name} with_ssim={s}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            last[name, s] = json.loads(line[-1][7:])
            times[name, s].append(last[name, s]["step_ms"])
            print(f"round {r} {name} with_ssim={s}: {times[name, s][-1]:.3f} ms/step", flush=True)
    res = {"shape": {"height": H, "width": W, "rays": RAYS, "samples": SAMPLES, "hidden": HIDDEN, "pair_grid": [47, 155]},
           "method": f"fresh process per measurement, {args.warmup} warm-up steps, {args.steps} steps between one "
                     f"hipEvent pair, {args.rounds} interleaved rounds; median ms per Trainer.train_step"}
    for name, _, s in runs:
        v = times[name, s]
        res.setdefault(name, {})[f"with_ssim_{s}"] = {
            "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rounds": len(v),
            "pair_kernels": last[name, s]["pair_kernels"], "launches_per_step": last[name, s]["launches_per_step"],
            "loss_rgb_s": last[name, s]["loss_rgb_s"], "pair_losses_us": last[name, s]["pair_losses_us"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
