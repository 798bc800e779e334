"""nerf_image_metrics (csrc/metrics.hip) on the GPU: MSE, mean SSIM and the SSIM map against the
fp64 restatement of the reference's pytorch_ssim (tests/ssim_ref.py).

The bar is "as accurate as the reference": e_ref = max |f32 restatement run on the GPU - fp64| on
the same inputs, e_hip the same for the kernel, and e_hip <= tests.helpers.tight_bar(e_ref) =
1.5 e_ref + 4 ulp -- the 1.5 covers another summation order and leaves no room for a wrong tap
or a wrong border.  The fp64 truth is computed once per case on the CPU and shared."""
import functools

import pytest
import torch
import torch.nn.functional as F

from model import _hip, metrics
from tests import ssim_ref
from tests.helpers import U24, report_err, tight_bar

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _truth(h, w, window, padding, seed=0):
    """(gt, pred, fp64 map, fp64 per-image mean, fp64 mse), all on the CPU."""
    gt, pred = ssim_ref.make_pair(h, w, seed)
    m = ssim_ref.ssim_map_ref(pred, gt, window, padding)
    return gt, pred, m, ssim_ref.mean_per_image(m), F.mse_loss(pred.double(), gt.double())


def _run(a, b, window=11, padding=True, want_map=True):
    """One nerf_image_metrics call on [B,C,H,W] views -> (out [B,2], map or None)."""
    n, c, h, w = a.shape
    out = torch.empty(n, 2, device=a.device)
    work = torch.empty(_hip.image_metrics_workspace_bytes(n, c, h, w), dtype=torch.uint8, device=a.device)
    cut = 0 if padding else window - 1
    smap = torch.empty(n, c, h - cut, w - cut, device=a.device) if want_map else None
    _hip.image_metrics(a, b, window, padding, out, work, smap)
    return out, smap


def _check_against_fp64(dev, name, h, w, window, padding):
    gt, pred, map64, mean64, mse64 = _truth(h, w, window, padding)
    g, p = gt.to(dev), pred.to(dev)
    # the reference's own arithmetic on this GPU
    map32 = ssim_ref.ssim_map_ref(p, g, window, padding, dtype=torch.float32)
    ref = {"map": (map32.double().cpu() - map64).abs().max().item(),
           "mean": (ssim_ref.mean_per_image(map32).double().cpu() - mean64).abs().max().item(),
           "mse": abs(F.mse_loss(p, g).double().item() - mse64.item())}
    out, smap = _run(p, g, window, padding)
    assert smap.shape == map64.shape
    hip = {"map": (smap.double().cpu() - map64).abs().max().item(),
           "mean": abs(out[0, 1].double().item() - mean64.item()),
           "mse": abs(out[0, 0].double().item() - mse64.item())}
    for k in ("map", "mean", "mse"):
        report_err(name, f"{k}_ref_f32", ref[k])
        report_err(name, f"{k}_hip", hip[k])
        print(f"{name} {h}x{w} w={window} pad={padding} {k}: e_hip={hip[k]:.3e} e_ref={ref[k]:.3e}")
    for k in ("map", "mean", "mse"):
        assert hip[k] <= tight_bar(ref[k]), (k, hip[k], ref[k])
    # the public surface returns the same scalars
    assert metrics.ssim(p, g, use_padding=padding, window_size=window).item() == out[0, 1].item()


@pytest.mark.parametrize("h,w", ssim_ref.SHAPES)
def test_mean_and_map_match_fp64(dev, h, w):
    _check_against_fp64(dev, "image_metrics", h, w, 11, True)


@pytest.mark.parametrize("h,w,window,padding", [(11, 11, 11, False), (33, 45, 11, False), (33, 45, 1, True),
                                                (33, 45, 3, True), (33, 45, 7, True), (33, 45, 7, False)])
def test_borders_and_windows(dev, h, w, window, padding):
    _check_against_fp64(dev, "image_metrics_window", h, w, window, padding)
    if (h, w, padding) == (11, 11, False):
        assert _truth(h, w, window, padding)[2].shape == (1, 3, 1, 1)     # exactly one valid position


def test_batch_of_two_equals_single_calls(dev):
    pairs = [ssim_ref.make_pair(33, 45, seed) for seed in (1, 2)]
    gt2 = torch.cat([pairs[0][0], pairs[1][0].flip(-1)]).to(dev)          # two different image pairs
    pr2 = torch.cat([pairs[0][1], pairs[1][1].flip(-1)]).to(dev)
    out2, map2 = _run(pr2, gt2)
    assert not torch.equal(out2[0], out2[1])
    for i in range(2):
        out1, map1 = _run(pr2[i:i + 1], gt2[i:i + 1])
        assert torch.equal(out1[0], out2[i]) and torch.equal(map1[0], map2[i])
    per = metrics.ssim(pr2, gt2, size_average=False)
    assert torch.equal(per, out2[:, 1]) and metrics.ssim(pr2, gt2).item() == out2[:, 1].mean().item()


def test_layouts_give_identical_bits(dev):
    gt, pred = (t.to(dev) for t in ssim_ref.make_pair(33, 45))
    base, base_map = _run(pred, gt)                                        # both contiguous [B,C,H,W]
    # the evaluation's layouts: the renderer's [H,W,3] frame against the loader's [1,3,H,W]
    hwc = pred[0].permute(1, 2, 0).contiguous()
    assert torch.equal(metrics.image_metrics(hwc, gt), base[0])
    assert torch.equal(metrics.image_metrics(hwc, gt[0]), base[0])
    out, smap = _run(hwc.permute(2, 0, 1).unsqueeze(0), gt)
    assert torch.equal(out, base) and torch.equal(smap, base_map)
    # a non-contiguous crop of a larger tensor against its contiguous copy
    big = torch.rand(1, 3, 33 + 7, 45 + 9, device=dev)
    big[:, :, 3:36, 5:50] = pred
    crop = big[:, :, 3:36, 5:50]
    assert not crop.is_contiguous()
    out, smap = _run(crop, gt)
    assert torch.equal(out, base) and torch.equal(smap, base_map)
    out, smap = _run(gt, crop)                                             # and as the second image
    swapped, swapped_map = _run(gt, pred)
    assert torch.equal(out, swapped) and torch.equal(smap, swapped_map)


@pytest.mark.parametrize("h,w", [(7, 9), (33, 45)])
def test_identity(dev, h, w):
    gt = ssim_ref.make_pair(h, w)[0].to(dev)
    out, smap = _run(gt, gt.clone())
    assert out[0, 0].item() == 0.0
    assert abs(out[0, 1].item() - 1.0) <= 4 * U24
    assert (smap - 1.0).abs().max().item() <= 4 * U24


def test_deterministic_bits(dev):
    gt, pred = (t.to(dev) for t in ssim_ref.make_pair(188, 621))
    hwc = pred[0].permute(1, 2, 0).contiguous()
    a, a_map = _run(hwc.permute(2, 0, 1).unsqueeze(0), gt)
    b, b_map = _run(hwc.permute(2, 0, 1).unsqueeze(0), gt)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(a_map.view(torch.int32), b_map.view(torch.int32))


@pytest.mark.parametrize("h,w", [(7, 9), (33, 45)])
def test_no_stray_writes(dev, h, w):
    """Outputs, map and workspace sit between guard bands of a sentinel; the guards are intact after
    the call and every output element was written."""
    gt, pred = (t.to(dev) for t in ssim_ref.make_pair(h, w))
    G, S = 256, -777.0
    n_map = 3 * h * w
    out_buf = torch.full((G + 2 + G,), S, device=dev)
    map_buf = torch.full((G + n_map + G,), S, device=dev)
    n_work = _hip.image_metrics_workspace_bytes(1, 3, h, w)
    work_buf = torch.full((G + n_work + G,), 0xA5, dtype=torch.uint8, device=dev)
    out = out_buf[G:G + 2].view(1, 2)
    smap = map_buf[G:G + n_map].view(1, 3, h, w)
    _hip.image_metrics(pred, gt, 11, True, out, work_buf[G:G + n_work], smap)
    for buf, n in ((out_buf, 2), (map_buf, n_map)):
        assert (buf[:G] == S).all() and (buf[G + n:] == S).all()
        assert (buf[G:G + n] != S).all()
    assert (work_buf[:G] == 0xA5).all() and (work_buf[G + n_work:] == 0xA5).all()
    want, want_map = _run(pred, gt)
    assert torch.equal(out, want) and torch.equal(smap, want_map)
