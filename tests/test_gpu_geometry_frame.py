"""Renderer.phong_frame -- the whole-frame geometry render (model/geometry.py, csrc/march.hip) --
against the oracle's phong_renderer and against the chunked Renderer.phong_renderer, on the
octahedron field and camera of tests/test_gpu_geometry.py with that file's bars (GPU only):
the hit mask differs in at most 2 of 384 pixels, colours within 1e-4 where the masks agree,
distances within 1e-4 on hits and within 1e-4 of the analytic surface.  Three routes: hidden 64
(per-layer forwards), hidden 256 in precision mode 2 (the fused eval render's alpha), hidden 256
with dist_alpha (the raw head output).  Then: the frame is captured as a graph and replays the
same bits (no host sync inside it), and the two callers write what the chunk loop wrote."""
import math

import numpy as np
import pytest
import torch

import model as mdl
from model import _hip
from oracle import nerf_oracle as orc
from tests import march_ref as MR
from tests.helpers import make_cfg
from tests.helpers_depth_prior import capture_graph
from tests.test_gpu_geometry import _camera, _octahedron_field

pytestmark = pytest.mark.gpu

H, W = 16, 24
CAM = torch.tensor([0.15, -0.1, 2.0])
_ORACLE = {}


def _oracle(D, dist_alpha):
    """The oracle's frame, computed once per field."""
    key = (D, dist_alpha)
    if key not in _ORACLE:
        cfg = make_cfg(hidden=D, S=32, dist_alpha=dist_alpha)
        ref = orc.OracleNerf(hidden_dim=D, dist_alpha=dist_alpha)
        ref.load_state_dict(_octahedron_field(cfg).state_dict())
        pix = orc.arange_pixels(H, W)[1]
        K, w2c, S = _camera(H, W)
        out = orc.phong_renderer(ref, pix, K, w2c, S, rad=cfg["rendering"]["radius"])
        ray = orc.image_points_to_world(pix, K, w2c, S)[0] - CAM
        _ORACLE[key] = (out, ray / ray.norm(dim=-1, keepdim=True))
    return _ORACLE[key]


def _setup(dev, D, dist_alpha=False, h=H, w=W):
    cfg = make_cfg(hidden=D, S=32, dist_alpha=dist_alpha)
    rnd = mdl.Renderer(_octahedron_field(cfg), cfg["rendering"], device=dev)
    pix = orc.arange_pixels(h, w)[1].to(dev)
    return rnd, pix, [t.to(dev) for t in _camera(h, w)]


def _compare(got, want_rgb, want_surf, want_mask, what):
    """The bars of tests/test_gpu_geometry.py between a frame and a reference -> the agreeing pixels."""
    rgb, surf, mask = got["rgb"].cpu()[0], got["rgb_surf"].cpu()[0], got["mask"].cpu()
    assert torch.equal((rgb == 1).all(-1), ~mask), what          # background is exactly 1, and only there
    flips = int((mask != want_mask).sum())
    same = mask == want_mask
    e_rgb = (rgb[same] - want_rgb[same]).abs().max().item()
    e_surf = (surf[same & mask] - want_surf[same & mask]).abs().max().item()
    print(f"{what}: flips {flips}, rgb {e_rgb:.3g}, rgb_surf {e_surf:.3g}")
    assert flips <= 2, what
    assert e_rgb < 1e-4 and e_surf < 1e-4, what
    return same


@pytest.mark.parametrize("D,dist_alpha", [(64, False), (256, False), (256, True)], ids=["d64", "d256_fused", "d256_raw"])
def test_phong_frame_matches_oracle_and_chunks(dev, monkeypatch, D, dist_alpha):
    _hip.gemm_set_precision(2)
    out_o, ray = _oracle(D, dist_alpha)
    mask_o = out_o["mask"]
    assert 0.2 * H * W < mask_o.sum() < 0.9 * H * W
    rnd, pix, mats = _setup(dev, D, dist_alpha)
    fused_calls = []
    real = _hip.render_eval_fused
    monkeypatch.setattr(_hip, "render_eval_fused", lambda *a, **k: (fused_calls.append(a[3:5]), real(*a, **k))[1])
    out = rnd.phong_frame(pix, *mats, it=0)
    # the occupancy route: one fused launch over R * 4 pseudo-rays of 128 samples, or none
    assert fused_calls == ([(H * W * 4, 128)] if (D == 256 and not dist_alpha) else [])
    assert out["rgb"].shape == (1, H * W, 3) and out["rgb_surf"].shape == (1, H * W, 3) and out["normal"] is None
    assert out["d_i"].shape == (1, H * W) and out["mask"].shape == (H * W,) and out["mask"].dtype == torch.bool
    same = _compare(out, out_o["rgb"][0], out_o["rgb_surf"][0], mask_o, "frame vs oracle")
    d_h, d_o = out["d_i"].cpu()[0], out_o["d_i"][0]
    hits = same & mask_o
    assert (d_h[hits] - d_o[hits]).abs().max().item() < 1e-4
    assert torch.equal(d_h[same & ~mask_o], d_o[same & ~mask_o])             # inf where nothing is hit
    level = MR.OCTA_LEVEL_DIST_ALPHA if dist_alpha else 0.6
    m_h = out["mask"].cpu()
    hit = CAM + ray[m_h] * d_h[m_h].unsqueeze(-1)
    assert (hit.abs().sum(-1) - level).abs().max().item() < 1e-4
    # the chunked path of the same renderer on the same frame
    out_c = rnd.phong_renderer(pix, *mats, it=0)
    rgb_c = out_c["rgb"].cpu()[0]
    _compare(out, rgb_c, out_c["rgb_surf"].cpu()[0], ~(rgb_c == 1).all(-1), "frame vs chunked")


@pytest.mark.parametrize("D", [64, 256])
def test_phong_frame_special_rays(dev, D):
    """The rays of test_sphere_intersection_and_ray_marching_edges through 'd_i': a hit at 2.4, a miss
    (inf), and a camera inside the surface (0 for every pixel, drawn as background)."""
    _hip.gemm_set_precision(2)
    rnd, _, (K, _, S) = _setup(dev, D)
    pix = torch.tensor([[[0.0, 0.0], [1.0, 1.0]]], device=dev)      # directions (0, 0, -1) and (1, -1, -4) / |.|
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.0, 0.0, 3.0])
    out = rnd.phong_frame(pix, K, torch.inverse(c2w).unsqueeze(0).to(dev), S, it=0)
    d = out["d_i"].cpu()[0]
    assert abs(d[0].item() - 2.4) < 1e-4 and math.isinf(d[1].item())
    assert out["mask"].cpu().tolist() == [True, False]
    c2w[:3, 3] = torch.tensor([0.1, 0.0, 0.0])
    out = rnd.phong_frame(pix, K, torch.inverse(c2w).unsqueeze(0).to(dev), S, it=0)
    assert out["d_i"].cpu()[0].tolist() == [0.0, 0.0]
    assert (out["rgb"] == 1).all() and (out["rgb_surf"] == 0).all() and not out["mask"].any()


def test_phong_frame_is_graph_capturable(dev):
    """No host sync, no data-dependent shape: the 9 x 13 frame at hidden 256 is captured after one
    eager warm-up and the replay gives the eager bits."""
    _hip.gemm_set_precision(2)
    rnd, pix, mats = _setup(dev, 256, h=9, w=13)
    keys = ("rgb", "rgb_surf", "d_i", "mask")
    eager = {k: v.clone() for k, v in rnd.phong_frame(pix, *mats, it=0).items() if k in keys}
    assert 0 < int(eager["mask"].sum()) < 9 * 13
    g, out = capture_graph(lambda: rnd.phong_frame(pix, *mats, it=0), warm=1)
    for k in keys:
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(out[k], eager[k]), k


def _grey_levels_agree(a, b):
    """Within 1 grey level in at least 99.5 % of the pixels (the 2-in-384 cap as a share)."""
    close = (np.abs(a.astype(int) - b.astype(int)) <= 1).all(-1)
    return close.mean() >= 0.995


def _count_chunks(monkeypatch):
    calls = []
    real = mdl.Renderer.phong_renderer
    monkeypatch.setattr(mdl.Renderer, "phong_renderer", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    return calls, real


def test_render_visdata_uses_the_frame(dev, monkeypatch, tmp_path):
    from PIL import Image
    from model.optim import HipAdam
    h, w = 9, 13
    cfg = make_cfg(hidden=64, S=32)
    cfg["training"]["vis_geo"] = True
    rnd = mdl.Renderer(_octahedron_field(cfg), cfg["rendering"], device=dev)
    nn_model = mdl.get_model(rnd, cfg, device=dev)
    K, w2c, S = _camera(h, w)
    c2w = torch.inverse(w2c[0])
    pose = mdl.LearnPose(1, False, False, cfg, init_c2w=c2w.unsqueeze(0).to(dev)).to(dev)
    trainer = mdl.Trainer(nn_model, HipAdam(nn_model.parameters(), lr=1e-3), cfg["training"], device=dev,
                          pose_param_net=pose)
    data = {"img": torch.rand(1, 3, h, w), "img.idx": torch.tensor([0]), "img.depth": torch.ones(1, h, w),
            "img.depth_mask": torch.ones(1, h, w, dtype=torch.bool), "img.camera_mat": K, "img.scale_mat": S,
            "img.pose_gt": c2w.unsqueeze(0)}
    calls, real = _count_chunks(monkeypatch)
    geo = trainer.render_visdata(data, (h, w), 0, str(tmp_path))
    assert calls == []                                            # the chunk loop was not entered
    for name in ("0000_depth.png", "0000_img.png", "0000_geo.png"):
        assert (tmp_path / name).exists()
    assert geo.shape == (h, w, 3) and geo.dtype == np.uint8
    assert np.array_equal(np.asarray(Image.open(tmp_path / "0000_geo.png")), geo)
    pix = orc.arange_pixels(h, w)[1].to(dev)
    ref = real(rnd, pix, K.to(dev), w2c.to(dev), S.to(dev), 0)["rgb"]
    ref = (ref.view(h, w, 3).cpu().numpy() * 255).astype(np.uint8)
    assert 0 < (ref != 255).all(-1).sum() < h * w
    assert _grey_levels_agree(geo, ref)


def test_extract_images_uses_the_frame(dev, monkeypatch, tmp_path):
    from PIL import Image
    from model.extracting_images import Extract_Images
    h, w = 9, 13
    cfg = make_cfg(hidden=64, S=32)
    cfg["extract_images"] = {"resolution": [h, w]}
    rnd = mdl.Renderer(_octahedron_field(cfg), cfg["rendering"], device=dev)
    K, w2c, S = _camera(h, w)
    c2ws = torch.inverse(w2c[0]).unsqueeze(0)
    ex = Extract_Images(rnd, cfg, use_learnt_poses=True, use_learnt_focal=False, device=dev, render_type="nope_nerf")
    data = {"img.idx": torch.tensor([0]), "img.camera_mat": K, "img.scale_mat": S}
    calls, real = _count_chunks(monkeypatch)
    out = ex.generate_images(data, str(tmp_path), c2ws.to(dev), None, 0, True)
    assert calls == []
    for sub in ("img_out/0000.png", "depth_out/0000.png", "depth_out/0.npy", "disp_out/0000.png", "geo_out/0000.png"):
        assert (tmp_path / sub).exists()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "geo_out" / "0000.png")), out["geo"])
    pix = orc.arange_pixels(h, w)[1].to(dev)
    ref = real(rnd, pix, K.to(dev), w2c.to(dev), S.to(dev), 0)["rgb"]
    ref = (ref.view(h, w, 3).cpu().numpy() * 255).astype(np.uint8)
    assert 0 < (ref != 255).all(-1).sum() < h * w
    assert _grey_levels_agree(out["geo"], ref)
