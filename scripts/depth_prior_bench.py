"""ms/step of the cfg2-shaped training step under the two depth-prior settings that used to leave the
sync-free path: a sparse device depth mask (1 valid pixel in 400, the fork's *_d6 configs) with the l1
depth term, and depth_loss_type 'invariant'.  One JSON line per run; run it in the tree under test and in a
checkout of the commit to compare with, a fresh process per side and round, interleaved:

    python scripts/depth_prior_bench.py --case sparse|invariant|dense [--steps 200] [--warmup 20]

Uses the public Trainer only, so it runs unchanged on a tree without the device-side redraw.  "head_calls"
counts the C-ABI launches of the step's head per step (the draw, the 4x4 chain, the camera rays, the weight
pack); "draw_launches" the launches that draw rays per step (the sampler or the step head: more than one
means the host loop looked at the draw, a sync, and drew again).  The comparison is scripts/lib_ab.py's: one
child process per side and round, sides interleaved; lib_ab.py itself swaps only the library under one tree's
Python, and here the Python side differs too, so each side runs this script in its own tree."""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "my-nope-nerf_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HEAD = ("nerf_step_head", "nerf_step_head_valid", "nerf_sample_rays", "nerf_sample_rays_valid", "nerf_pose_c2w",
        "nerf_mat4_inv", "nerf_unproject_matrix", "nerf_depth_affine", "nerf_camera_rays", "nerf_pack_weights")
LOSS = ("nerf_ray_loss", "nerf_ray_loss_bwd", "nerf_ray_loss_invariant", "nerf_ray_loss_invariant_bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["sparse", "invariant", "dense"], default="sparse")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import bench
    from model import _hip
    dev = torch.device("cuda:0")
    _hip.gemm_set_precision(2)
    cfg = bench.make_cfg()
    if args.case == "invariant":
        cfg["training"]["depth_loss_type"] = "invariant"
    data, c2w = bench.synthetic_scene(dev)
    if args.case == "sparse":
        mask = torch.zeros(1, bench.H, bench.W, dtype=torch.bool)
        mask[:, ::20, ::20] = True                                    # 1 valid pixel in 400
        data["img.depth"] = torch.where(mask.to(dev), data["img.depth"].clamp_min(1.0), 0.0)
        data["img.depth_mask"] = mask.to(dev)
    trainer, _ = bench.build_trainer(dev, c2w, cfg)
    torch.manual_seed(0)
    calls = collections.Counter()
    call = _hip._call

    def counted(name, *a):
        calls[name] += 1
        return call(name, *a)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            ld = trainer.train_step(data, it=i, epoch=0, scheduling_start=0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, ld
    run(args.warmup)
    el, ld = run(args.steps)
    _hip._call = counted                  # the launch census: a few more steps, outside the timed ones
    n_census = 20
    run(n_census)
    _hip._call = call
    head = {k: calls[k] / n_census for k in HEAD if calls[k]}
    out = {"case": args.case, "ms_per_step": 1e3 * el / args.steps, "steps": args.steps,
           "final_loss": ld["loss"].item(), "head_calls": head, "head_calls_per_step": sum(head.values()),
           "loss_calls": {k: calls[k] / n_census for k in LOSS if calls[k]},
           "draw_launches": (calls["nerf_sample_rays"] + calls["nerf_sample_rays_valid"] + calls["nerf_step_head"]
                          + calls["nerf_step_head_valid"]) / n_census,
           "draw_attempts": int(trainer.draw_attempts.item()) if getattr(trainer, "draw_attempts", None) is not None
           else None}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
