"""Writes tests/golden/eval_ssim.pt: the (33, 45) test images of tests/ssim_ref.py and what the
reference's own third_party/pytorch_ssim.ssim returns for them in float32 on the CPU.  It pins the
restatement in tests/ssim_ref.py to the real module (tests/test_eval_images_cpu.py).

    python tests/golden/make_eval_ssim_golden.py <path to the reference checkout>

Only third_party.pytorch_ssim is imported from the reference tree; the file holds data it wrote.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main(reference_root):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, reference_root)
    from third_party import pytorch_ssim
    from tests import ssim_ref
    gt, pred = ssim_ref.make_pair(33, 45)
    out = {"gt": gt, "pred": pred,
           "pad_w11": pytorch_ssim.ssim(pred, gt).detach().clone(),
           "nopad_w11": pytorch_ssim.ssim(pred, gt, use_padding=False).detach().clone(),
           "pad_w7": pytorch_ssim.ssim(pred, gt, window_size=7).detach().clone()}
    path = os.path.join(HERE, "eval_ssim.pt")
    torch.save(out, path)
    print({k: (v.item() if v.dim() == 0 else tuple(v.shape)) for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])
