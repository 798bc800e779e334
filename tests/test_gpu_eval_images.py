"""Eval_Images.eval_images (eval_images.py:47-218, the caller of evaluation/eval.py:146-188) end to
end on the GPU for one small frame: the render is Extract_Images.render_frame's, the metrics are
nerf_image_metrics' and as accurate as the reference's own float32 (tests/ssim_ref.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from model.common import mse2psnr
from model.official_nerf import OfficialStaticNerf
from model.rendering import Renderer
from tests import ssim_ref
from tests.helpers import camera_K, make_cfg, report_err, rigid_c2w, tight_bar

pytestmark = pytest.mark.gpu


def test_eval_images_one_frame(dev, tmp_path, monkeypatch):
    from model.eval_images import Eval_Images
    from model.extracting_images import Extract_Images
    h, w, S, hidden = 24, 40, 32, 64
    cfg = make_cfg(hidden=hidden, S=S)
    cfg["extract_images"] = {"resolution": [h, w]}
    torch.manual_seed(3)
    rnd = Renderer(OfficialStaticNerf(cfg).to(dev), cfg["rendering"], device=dev)
    K = camera_K(h, w, 30.0, 30.0)
    c2ws = torch.stack([rigid_c2w(5, 0.2), rigid_c2w(6, 0.2)]).to(dev)
    scale = torch.eye(4).unsqueeze(0)

    # the frame the evaluation must see: Extract_Images' render of the same camera
    ex = Extract_Images(rnd, cfg, use_learnt_poses=True, use_learnt_focal=False, device=dev, render_type="nope_nerf")
    with torch.no_grad():
        frame, _ = ex.render_frame(K.to(dev), torch.inverse(c2ws[1]).unsqueeze(0), scale.to(dev), 1000)
    frame = frame.clone()

    g = torch.Generator().manual_seed(11)
    gt = (frame.cpu().permute(2, 0, 1) + 0.1 * torch.randn(3, h, w, generator=g)).clamp(0, 1).unsqueeze(0).contiguous()
    data = {"img": gt, "img.gt_depths": 0.05 + 25.0 * torch.rand(1, 48, 80, generator=g), "img.idx": torch.tensor([1]),
            "img.camera_mat": K, "img.scale_mat": scale}
    ev = Eval_Images(rnd, cfg, use_learnt_poses=True, use_learnt_focal=False, device=dev, render_type="nope_nerf",
                     c2ws=c2ws)
    # record the float frame eval_images scores: the metrics below are checked on that very tensor
    scored = {}
    render = Eval_Images.render_frame

    def recording(self, *args):
        scored["frame"], scored["depth"] = render(self, *args)
        return scored["frame"], scored["depth"]

    monkeypatch.setattr(Eval_Images, "render_frame", recording)
    rnd.train()
    out = ev.eval_images(data, str(tmp_path), None, lambda a, b, normalize: torch.tensor([[0.25]], device=a.device),
                         None, it=1000)
    assert rnd.training is False                                           # eval_images.py:48
    assert np.array_equal(out["img"], (frame.cpu().numpy() * 255).astype(np.uint8))
    assert np.array_equal(out["img"], (scored["frame"].cpu().numpy() * 255).astype(np.uint8))

    # mse / ssim against fp64 on the returned float frame, no worse than the reference's own f32 on this GPU
    pred = scored["frame"].permute(2, 0, 1).unsqueeze(0)
    gtd = gt.to(dev)
    map64 = ssim_ref.ssim_map_ref(pred.cpu(), gt)
    mse64 = F.mse_loss(pred.cpu().double(), gt.double()).item()
    e_ref_ssim = abs(ssim_ref.ssim_map_ref(pred, gtd, dtype=torch.float32).mean().item() - map64.mean().item())
    e_ref_mse = abs(F.mse_loss(pred, gtd).item() - mse64)
    e_ssim, e_mse = abs(out["ssim"] - map64.mean().item()), abs(out["mse"] - mse64)
    for name, e in (("ssim_ref_f32", e_ref_ssim), ("ssim_hip", e_ssim), ("mse_ref_f32", e_ref_mse), ("mse_hip", e_mse)):
        report_err("eval_images", name, e)
        print(f"eval_images {name}: {e:.3e}")
    assert e_ssim <= tight_bar(e_ref_ssim) and e_mse <= tight_bar(e_ref_mse)
    assert out["psnr"] == mse2psnr(out["mse"])
    assert out["lpips"] == 0.25
    assert out["conf_mat"].shape == (2, 2) and out["depth_pred"].shape == out["depth_gt"].shape

    for sub in ("img_out/0001.png", "depth_out/0001.png", "img_gt_out/0001.png", "depth_gt_out/0001.png",
                "disp_out/0001.png", "disp_gt_out/0001.png", "depth_mask/0001.png", "depth_mask/0001_gt.png",
                "depth_mask/0001_mask_rendered.png", "depth_mask/0001_mask_gt.png",
                "depth_mask/0001_mask_combined.png"):
        assert (tmp_path / sub).exists(), sub
