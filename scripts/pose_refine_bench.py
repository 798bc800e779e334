"""Test-time pose refinement step at the cfg2 shape (1024 rays x 128 samples, D = 256, GEMM
precision mode 2): Trainer_pose.train_step on the frozen-field path (field_grad=False) against
the same step through the training backward (field_grad=True: every weight gradient computed
and dropped, what a wrapper around the training path would run).

The two variants are interleaved step by step, each step timed by a pair of hipEvents, after a
warm-up; the medians, the spread and the peak allocated bytes of each go to a JSON file, with
the chain kernels' own times (nerf_prof_read_kinds) from a second, profiled pass.  Not part of
the suite or of bench.py.

    python scripts/pose_refine_bench.py [--steps 40 --warmup 10 --out profiles/pose_refine/bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "my-nope-nerf_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

RAYS, SAMPLES, HIDDEN = 1024, 128, 256


def build(dev, field_grad):
    import model as mdl
    from model.synthetic import VKITTI_FOCAL, VKITTI_H, VKITTI_W, make_cfg, vkitti_scene
    cfg = make_cfg(hidden=HIDDEN, S=SAMPLES)
    data, c2w = vkitti_scene(dev, 0, VKITTI_H, VKITTI_W, VKITTI_FOCAL)
    torch.manual_seed(42)
    net = mdl.OfficialStaticNerf(cfg)
    renderer = mdl.Renderer(net, cfg["rendering"], device=dev)
    nn_model = mdl.get_model(renderer, cfg, device=dev)
    pose = mdl.LearnPose(1, True, True, cfg, init_c2w=c2w.unsqueeze(0).to(dev)).to(dev)
    opt = torch.optim.Adam(pose.parameters(), lr=1e-3)
    tr = mdl.Trainer_pose(nn_model, {"n_points": RAYS, "type": "nope_nerf"}, dev, opt, pose, None)
    tr.field_grad = field_grad
    return tr, net, data


def step(tr, net, data):
    if tr.field_grad:
        net.zero_grad(set_to_none=True)     # the unused gradients are dropped, not accumulated
    return tr.train_step(data)["loss"]


def spread(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "q1_ms": q[0], "q3_ms": q[2],
            "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--prof-steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_refine", "bench.json"))
    args = ap.parse_args()
    if args.steps < 20:
        raise SystemExit("--steps: a median of at least 20 per variant")
    from model import _hip
    _hip.load_library()
    _hip.gemm_set_precision(2)
    dev = torch.device("cuda", 0)
    variants = {"frozen": build(dev, False), "full": build(dev, True)}
    times = {k: [] for k in variants}
    peak = {}
    for name, v in variants.items():        # warm-up, and each variant's peak memory on its own
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        for _ in range(args.warmup):
            loss = step(*v)
        torch.cuda.synchronize()
        peak[name] = {"peak_allocated_bytes": torch.cuda.max_memory_allocated(dev),
                      "allocated_before_bytes": base}
        if not torch.isfinite(loss).item():
            raise RuntimeError(f"{name}: non-finite loss")
    for _ in range(args.steps):
        for name, v in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(*v)
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    kernels = {}
    _hip.prof_enable(True)
    try:
        for name, v in variants.items():
            _hip.prof_read()                 # reset
            for _ in range(args.prof_steps):
                step(*v)
            torch.cuda.synchronize()
            kinds = _hip.prof_read_kinds()
            _hip.prof_read()
            kernels[name] = {k: {"us_per_launch": 1e3 * r["ms"] / r["launches"], "launches": r["launches"]}
                             for k, r in kinds.items() if r["launches"]}
    finally:
        _hip.prof_enable(False)
    res = {"shape": {"rays": RAYS, "samples": SAMPLES, "hidden": HIDDEN, "gemm_precision": 2, "scene": "synthetic"},
           "method": "interleaved steps, one hipEvent pair per step, medians",
           "frozen": {**spread(times["frozen"]), **peak["frozen"]},
           "full": {**spread(times["full"]), **peak["full"]},
           "gain_ms": statistics.median(times["full"]) - statistics.median(times["frozen"]),
           # chain_fwd: k_mlp_chain_frozen (frozen) / k_mlp_chain_train2 (full); chain_bwd:
           # k_mlp_chain_bwd_rays / k_mlp_chain_bwd; dx: the 64-wide encoding-gradient GEMMs
           "kernels": kernels}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
