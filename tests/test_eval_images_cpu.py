"""Novel-view evaluation, the parts that need no GPU: the names evaluation/eval.py:14 imports
resolve, nerf_image_metrics refuses bad arguments on the host before any HIP call, the
nearest-exact resize, the CPU path of metrics.ssim, and the host part of Eval_Images.eval_images
(eval_images.py:94-218) on a fixed frame."""
import importlib
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from model import _hip
from tests import ssim_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_ssim.pt")


def test_names():
    """eval.py:14 `from model.eval_images import Eval_Images`; the constructor stores what
    eval_images.py:19-28 stores."""
    cls = importlib.import_module("model.eval_images").Eval_Images
    e = cls("rnd", {"extract_images": {"resolution": [12, 20]}}, points_batch_size=77, use_learnt_poses=False,
            use_learnt_focal=False, device="cpu", render_type="nope_nerf", c2ws="poses", img_list=["a"])
    assert (e.points_batch_size, e.renderer, e.resolution, e.device) == (77, "rnd", [12, 20], "cpu")
    assert (e.use_learnt_poses, e.use_learnt_focal, e.render_type, e.c2ws, e.img_list) == \
        (False, False, "nope_nerf", "poses", ["a"])
    assert cls("rnd", {"extract_images": {"resolution": [1, 1]}}).points_batch_size == 100000
    for name in ("eval_images", "process_data_dict", "render_frame"):
        assert callable(getattr(cls, name))
    # one render method for both extractors
    from model.extracting_images import Extract_Images
    assert cls.render_frame is Extract_Images.render_frame


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_hip.LIB_PATH):
        pytest.fail(f"library not built at {_hip.LIB_PATH}; run __graft_entry__.build()")
    return _hip.load_library()


def test_abi(lib):
    assert lib.nerf_hip_abi_version() == 15
    for n in ("nerf_image_metrics", "nerf_image_metrics_workspace_bytes"):
        assert n in _hip.EXPORTED_SYMBOLS and hasattr(lib, n)
    # one (sum of squares, sum of SSIM) pair of doubles per 32 x 32 tile, channel and image
    assert lib.nerf_image_metrics_workspace_bytes(1, 3, 188, 621) == 3 * 6 * 20 * 16
    assert lib.nerf_image_metrics_workspace_bytes(2, 3, 32, 33) == 2 * 3 * 1 * 2 * 16
    assert lib.nerf_image_metrics_workspace_bytes(1, 3, 0, 621) == 0


P = 4096   # a non-NULL, aligned stand-in for a device pointer (never dereferenced on the host)


def _call(lib, img1=P, img2=P, batch=1, channels=3, height=33, width=45, window=11, use_padding=1, out=P, ssim_map=None,
          workspace=P):
    return lib.nerf_image_metrics(img1, 3 * height * width, height * width, width, 1, img2, 3 * height * width,
                                  height * width, width, 1, batch, channels, height, width, window, use_padding, out,
                                  ssim_map, workspace, None)


@pytest.mark.parametrize("kw,word", [
    ({"img1": None}, b"img1"), ({"img2": None}, b"img2"), ({"out": None}, b"out"),
    ({"window": 4}, b"window"), ({"window": 0}, b"window"), ({"window": 13}, b"window"), ({"window": -3}, b"window"),
    ({"batch": 0}, b"batch"), ({"channels": 0}, b"channels"), ({"height": 0}, b"height"), ({"width": -1}, b"width"),
    ({"use_padding": 0, "height": 10}, b"use_padding"), ({"use_padding": 0, "width": 7, "window": 9}, b"use_padding"),
    ({"workspace": None}, b"workspace"),
])
def test_refusals(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.nerf_hip_last_error()
    assert b"nerf_image_metrics" in msg and word in msg, msg


@pytest.mark.parametrize("src,dst", [((5, 5), (7, 7)), ((7, 7), (5, 5)), ((47, 155), (188, 621)),
                                     ((188, 621), (375, 1242)), ((12, 20), (12, 20))])
def test_resize_nearest_exact(src, dst):
    from model.metrics import resize_nearest_exact
    a = torch.arange(src[0] * src[1], dtype=torch.float32).reshape(src)
    want = F.interpolate(a[None, None], size=dst, mode="nearest-exact")[0, 0].numpy()
    got = resize_nearest_exact(a.numpy(), dst)
    assert got.shape == tuple(dst) and got.dtype == np.float32
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape,window,padding", [((33, 45), 11, True), ((33, 45), 11, False), ((7, 9), 11, True),
                                                  ((33, 45), 7, True), ((1, 1), 11, True)])
def test_ssim_cpu_path_has_the_formula(shape, window, padding):
    """The CPU path of metrics.ssim against the fp64 restatement, on the MAP: atol 1e-3, whose only
    job is to catch a wrong formula, tap or border (the reference's own f32 map is within 7.7e-4
    of fp64 on these inputs; a mean would average a local error away).  metrics.ssim is the mean
    of that map."""
    from model import metrics
    gt, pred = ssim_ref.make_pair(*shape)
    truth = ssim_ref.ssim_map_ref(pred, gt, window, padding)
    got_map = metrics.ssim_map_torch(pred, gt, use_padding=padding, window_size=window)
    assert got_map.shape == truth.shape and got_map.dtype == torch.float32
    assert (got_map.double() - truth).abs().max().item() <= 1e-3
    # an image against itself: the map is 1 everywhere
    self_map = metrics.ssim_map_torch(gt, gt.clone(), use_padding=padding, window_size=window)
    assert (self_map.double() - ssim_ref.ssim_map_ref(gt, gt, window, padding)).abs().max().item() <= 1e-3
    assert (self_map - 1.0).abs().max().item() <= 1e-3
    # the scalar and per-image returns of pytorch_ssim.ssim (:43-46) are means of that map
    got = metrics.ssim(pred, gt, use_padding=padding, window_size=window)
    assert got.dim() == 0 and got.dtype == torch.float32
    assert abs(got.item() - got_map.double().mean().item()) <= 1e-6
    per = metrics.ssim(torch.cat([pred, gt]), torch.cat([gt, gt]), use_padding=padding, window_size=window,
                       size_average=False)
    assert per.shape == (2,)
    assert abs(per[0].item() - got_map.double().mean().item()) <= 1e-6
    assert abs(per[1].item() - self_map.double().mean().item()) <= 1e-6
    # the strided views the evaluation passes give the same numbers as their contiguous copies
    if (window, padding) == (11, True):
        hwc = pred[0].permute(1, 2, 0).contiguous()
        m = metrics.image_metrics(hwc, gt)
        assert abs(m[1].item() - got_map.double().mean().item()) <= 1e-6
        assert abs(m[0].item() - F.mse_loss(pred.double(), gt.double()).item()) <= 1e-6
    with pytest.raises(ValueError, match="window_size"):
        metrics.ssim(pred, gt, window_size=4)


def test_restatement_matches_the_reference_outputs():
    """tests/golden/eval_ssim.pt (make_eval_ssim_golden.py): the (33, 45) inputs and what the
    reference's pytorch_ssim.ssim returned for them in float32; the f32 restatement equals it."""
    gold = torch.load(GOLDEN, weights_only=True)
    gt, pred = ssim_ref.make_pair(33, 45)
    assert torch.equal(gold["gt"], gt) and torch.equal(gold["pred"], pred)
    for key, window, padding in (("pad_w11", 11, True), ("nopad_w11", 11, False), ("pad_w7", 7, True)):
        mine = ssim_ref.ssim_map_ref(pred, gt, window, padding, dtype=torch.float32).mean().item()
        assert abs(mine - gold[key].item()) <= 1e-6, (key, mine, gold[key].item())


class _StubRenderer:
    training = True

    def eval(self):
        self.training = False


def _host_case():
    g = torch.Generator().manual_seed(5)
    h, w, gh, gw = 12, 20, 24, 40
    frame = torch.rand(h, w, 3, generator=g)
    depth = 0.02 + 14.0 * torch.rand(h, w, generator=g)          # x sc=2: both range limits are crossed
    gt = (frame.permute(2, 0, 1) + 0.1 * torch.randn(3, h, w, generator=g)).clamp(0, 1).unsqueeze(0).contiguous()
    depth_gt = 0.05 + 25.0 * torch.rand(1, gh, gw, generator=g)
    data = {"img": gt, "img.gt_depths": depth_gt, "img.idx": torch.tensor([3]),
            "img.camera_mat": torch.eye(4).unsqueeze(0), "img.scale_mat": torch.eye(4).unsqueeze(0)}
    return frame, depth, gt, depth_gt, data


def _evaluator(monkeypatch, frame, depth):
    from model.eval_images import Eval_Images
    seen = {}

    def fixed(self, camera_mat, world_mat, scale_mat, it):
        seen.update(camera_mat=camera_mat, world_mat=world_mat, it=it)
        return frame, depth

    monkeypatch.setattr(Eval_Images, "render_frame", fixed)
    rnd = _StubRenderer()
    ev = Eval_Images(rnd, {"extract_images": {"resolution": [12, 20]}}, use_learnt_poses=True, use_learnt_focal=True,
                     device=None, render_type="nope_nerf", c2ws=torch.eye(4).repeat(5, 1, 1))
    return ev, rnd, seen


def test_eval_images_host_part(monkeypatch, tmp_path):
    from model.common import mse2psnr
    frame, depth, gt, depth_gt, data = _host_case()
    depth_before = depth.clone()
    ev, rnd, seen = _evaluator(monkeypatch, frame, depth)
    out = ev.eval_images(data, str(tmp_path), (30.0, 31.0), lambda a, b, normalize: torch.tensor([[0.25]]), None,
                         min_depth=0.1, max_depth=20, it=9, sc=2, show_errors=True)
    assert rnd.training is False and seen["it"] == 9
    assert torch.equal(depth, depth_before)                      # sc scales a copy, not the frame
    assert seen["camera_mat"].tolist() == [[[30.0, 0, 0, 0], [0, -31.0, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]]]
    assert torch.equal(seen["world_mat"], torch.eye(4).unsqueeze(0))

    assert set(out) == {"img", "mse", "psnr", "ssim", "lpips", "depth_pred", "depth_gt", "conf_mat"}
    assert out["img"].dtype == np.uint8 and out["img"].shape == (12, 20, 3)
    assert np.array_equal(out["img"], (frame.numpy() * 255).astype(np.uint8))
    assert isinstance(out["mse"], float) and isinstance(out["ssim"], float)
    assert abs(out["mse"] - F.mse_loss(frame.permute(2, 0, 1)[None].double(), gt.double()).item()) <= 1e-6
    truth = ssim_ref.ssim_map_ref(frame.permute(2, 0, 1)[None], gt).mean().item()
    assert abs(out["ssim"] - truth) <= 1e-3
    assert out["psnr"] == mse2psnr(out["mse"])
    assert out["lpips"] == 0.25

    # numpy restatement of eval_images.py:105-107, 152-162, 200-217
    d = F.interpolate((depth * 2)[None, None], size=(24, 40), mode="nearest-exact")[0, 0].numpy()
    dg = depth_gt[0].numpy()
    mr, mg = (d >= 0.1) & (d <= 20), (dg >= 0.1) & (dg <= 20)
    conf = np.array([[np.sum(mr & mg), np.sum(~mr & mg)], [np.sum(mr & ~mg), np.sum(~mr & ~mg)]]) / (24 * 40 - 1)
    assert mr.any() and (~mr).any() and mg.any() and (~mg).any()
    assert out["conf_mat"].shape == (2, 2) and np.array_equal(out["conf_mat"], conf)
    assert out["conf_mat"].sum() > 1.0                          # the H*W - 1 divisor, kept
    assert np.array_equal(out["depth_pred"], d[mr & mg]) and out["depth_pred"].dtype == np.float32
    assert np.array_equal(out["depth_gt"], dg[mr & mg])

    from PIL import Image
    shapes = {"img_out/0003.png": (12, 20, 3), "depth_out/0003.png": (24, 40), "img_gt_out/0003.png": (12, 20, 3),
              "depth_gt_out/0003.png": (24, 40), "disp_gt_out/0003.png": (24, 40, 3), "disp_out/0003.png": (24, 40, 3),
              "depth_mask/0003_mask_rendered.png": (24, 40), "depth_mask/0003_mask_gt.png": (24, 40),
              "depth_mask/0003_mask_combined.png": (24, 40), "depth_mask/0003_gt.png": (24, 40, 3),
              "depth_mask/0003.png": (24, 40, 3)}
    for rel, shape in shapes.items():
        assert (tmp_path / rel).exists(), rel
        assert np.asarray(Image.open(tmp_path / rel)).shape == shape, rel
    assert np.array_equal(np.asarray(Image.open(tmp_path / "img_out/0003.png")), out["img"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "depth_mask/0003_mask_combined.png")) > 0, mr & mg)
    green = np.asarray(Image.open(tmp_path / "depth_mask/0003.png"))
    assert (green[~(mr & mg)] == [0, 255, 0]).all()
    assert (tmp_path / "0003_conf.png").exists()


def test_eval_images_without_lpips_and_gt_depths(monkeypatch, tmp_path):
    """lpips_vgg_fn=None gives NaN (the documented deviation); a missing img.gt_depths falls back
    to img.depth (eval_images.py:53-57); show_errors=False writes no plot."""
    frame, depth, gt, depth_gt, data = _host_case()
    del data["img.gt_depths"]
    data["img.depth"] = depth_gt
    ev, _, _ = _evaluator(monkeypatch, frame, depth)
    out = ev.eval_images(data, str(tmp_path), (30.0, 31.0), None, None, sc=2)
    assert math.isnan(out["lpips"])
    dg = depth_gt[0].numpy()
    d = F.interpolate((depth * 2)[None, None], size=(24, 40), mode="nearest-exact")[0, 0].numpy()
    m = (d >= 0.1) & (d <= 20) & (dg >= 0.1) & (dg <= 20)
    assert np.array_equal(out["depth_gt"], dg[m])
    assert not (tmp_path / "0003_conf.png").exists()
