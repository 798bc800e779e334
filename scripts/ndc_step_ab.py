"""The LLFF-style training step (sample_option ndc, dist_alpha, depth_range [0, 1]: configs/LLFF/fern.yaml:6-8)
on this tree and on a built checkout of the commit before nerf_ndc_rays, whose NDC warp is ~20 ATen
launches forward and their autograd backward (model/common.py get_ndc_rays_fxfy in Renderer.nope_nerf).

The step: Trainer.train_step on the one-view synthetic scene, 188 x 621, 1024 rays x 128 samples, D = 256,
pose learning (LearnPose with its Adam), GEMM mode f16x3, eager; the image-pair terms are off, so this is
the render path the warp sits in.  Reported:

* ms / step: a fresh process per measurement (its own Trainer, warmed), `--steps` steps between one pair
  of hipEvents, the trees interleaved over `--rounds` rounds, medians;
* launches per step between the step head (k_step_head*) and k_encode_samples, and in the whole step,
  from a rocprofv3 kernel trace of a few steps in a run of its own (tracing slows the host: no time is
  taken from it).

Not measured: graph replay, more than one GPU, real frames.  Not part of the suite or of bench.py.

    python scripts/ndc_step_ab.py --tree parent=/path/to/built/checkout [--steps 50 --rounds 3]
                                  [--out profiles/ndc/ndc_step_ab.txt] [--no-trace]
"""
from __future__ import annotations

import argparse
import collections
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FOCAL, RAYS, SAMPLES, HIDDEN = 188, 621, 362.5, 1024, 128, 256


def child(args):
    """One tree in this process: build the trainer, warm, time (or just step, under the profiler)."""
    sys.path.insert(0, os.path.join(args.child, "my-nope-nerf_amd"))
    import torch
    import model as mdl
    from model import _hip
    from model.optim import HipAdam
    from model.synthetic import make_cfg, vkitti_scene
    _hip.load_library()
    _hip.gemm_set_precision(2)
    dev = torch.device("cuda", 0)
    cfg = make_cfg(hidden=HIDDEN, S=SAMPLES, sample_option="ndc", dist_alpha=True, depth_range=[0.0, 1.0])
    t = cfg["training"]
    t["n_training_points"] = RAYS
    t["pc_weight"], t["rgb_s_weight"] = [0.0, 0.0], [0.0, 0.0]
    data, c2w = vkitti_scene(dev, 0, H, W, FOCAL)
    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    nn_model = mdl.get_model(mdl.Renderer(net, cfg["rendering"], device=dev), cfg, device=dev)
    pose = mdl.LearnPose(1, True, True, cfg, init_c2w=c2w.unsqueeze(0).to(dev)).to(dev)
    tr = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), t, device=dev,
                     optimizer_pose=torch.optim.Adam(pose.parameters(), lr=5e-4, fused=True), pose_param_net=pose)

    def one(i):
        return tr.train_step(data, it=i + 1, epoch=0, scheduling_start=0)

    for i in range(args.warmup):
        out = one(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(args.steps):
        out = one(args.warmup + i)
    b.record()
    b.synchronize()
    loss = float(out["loss"])
    if loss != loss or abs(loss) == float("inf"):
        raise SystemExit(f"non-finite loss {loss}")
    print("RESULT " + json.dumps({"step_ms": a.elapsed_time(b) / args.steps, "loss": loss,
                                  "hip_ndc": hasattr(_hip, "ndc_rays"), "pose_moved": bool((pose.r.detach() != 0).any())}))


def short(name):
    return name.replace("void ", "").replace("nerf::", "").split("(")[0].split("<")[0]


def summarise_trace(path):
    """Kernel-trace CSV -> launches per step between k_step_head* and the next k_encode_samples, the names of
    those launches, and launches per whole step (head to head)."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    names = [n for _, n in rows]
    heads = [i for i, n in enumerate(names) if n.startswith("k_step_head")]
    between, whole, seen = [], [], collections.Counter()
    for k, i in enumerate(heads):
        j = next((j for j in range(i + 1, len(names)) if names[j].startswith("k_encode_samples")), None)
        if j is None:
            break
        between.append(j - i - 1)
        if k + 1 < len(heads):
            whole.append(heads[k + 1] - i)
        if k == len(heads) - 2 or len(heads) == 1:      # the names of one warmed step
            seen = collections.Counter(names[i + 1:j])
    return {"steps_traced": len(between), "launches_head_to_encode": between, "launches_per_step": whole,
            "between_names": dict(seen)}


def run_child(tree, steps, warmup, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", tree, "--steps", str(steps),
                          "--warmup", str(warmup)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        raise SystemExit(f"{tree}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tree", action="append", default=[], metavar="NAME=DIR",
                    help="another checkout (built) to measure beside this one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ndc", "ndc_step_ab.txt"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "prof_out", "ndc_step_ab"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--summarise", metavar="CSV", help="only summarise this kernel-trace CSV")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.summarise:
        print(json.dumps(summarise_trace(args.summarise)))
        return
    trees = [("this_tree", ROOT)] + [(s.split("=", 1)[0], os.path.abspath(s.split("=", 1)[1])) for s in args.tree]
    times = {n: [] for n, _ in trees}
    last = {}
    for r in range(args.rounds):
        for name, path in trees:
            last[name] = run_child(path, args.steps, args.warmup)
            times[name].append(last[name]["step_ms"])
            print(f"round {r} {name}: {times[name][-1]:.3f} ms/step", flush=True)
    res = {"shape": {"height": H, "width": W, "rays": RAYS, "samples": SAMPLES, "hidden": HIDDEN, "gemm": "f16x3",
                     "learned": "pose", "pair_terms": False, "exec": "eager"},
           "method": f"fresh process per measurement, {args.warmup} warm-up steps, {args.steps} steps between one "
                     f"hipEvent pair, {args.rounds} interleaved rounds; median ms per Trainer.train_step; launch counts "
                     "from a rocprofv3 --kernel-trace run of 4 steps after 3 warm-up steps, in a run of its own",
           "not_measured": ["graph replay", "more than one GPU", "real frames"]}
    for name, path in trees:
        v = times[name]
        res[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "per_round_ms": v,
                     "hip_ndc": last[name]["hip_ndc"], "loss": last[name]["loss"], "pose_moved": last[name]["pose_moved"]}
        if args.no_trace or shutil.which("rocprofv3") is None:
            res[name]["trace"] = "not measured"
            continue
        d = os.path.join(args.trace_dir, name)
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d, exist_ok=True)
        run_child(path, 4, 3, prefix=["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "run", "--"])
        found = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        res[name]["trace"] = summarise_trace(found[-1]) if found else "no kernel trace written"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
