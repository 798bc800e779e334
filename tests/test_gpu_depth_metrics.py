"""nerf_depth_metrics (csrc/metrics.hip) on the GPU against the fp64 restatement of the reference's
depth evaluation (tests/depth_ref.py).

The bar is derived, not measured (depth_ref.check_against_ref): the counts and a1..a3 equal the
restatement exactly, the four continuous metrics lie within 2^-30 max(1, |ref|).  e_ref, the error
of the reference's own float32 compute_errors on the same selection, is printed and reported next
to e_hip; it is the DESIGN table's content, not the pass condition.  The restatement is computed
once per case on the CPU and shared."""
import functools
import os

import numpy as np
import pytest
import torch

from model import _hip, metrics
from tests import depth_ref
from tests.depth_ref import HI, LO, SCALES, SHAPES
from tests.helpers import SENT, Guarded, report_err

pytestmark = pytest.mark.gpu

CASES = [pytest.param(s, id="x".join(map(str, s))) for s in SHAPES] + [pytest.param("crafted", id="crafted")]
BIG = (188, 621, 375, 1242)


def _pair(case):
    return depth_ref.crafted_pair() if case == "crafted" else depth_ref.make_depth_pair(*case)


@functools.lru_cache(maxsize=None)
def _truth(case, sc):
    """(pred, gt, the fp64 restatement, the float32 restatement's seven errors), all on the CPU."""
    pred, gt = _pair(case)
    if case != "crafted":
        depth_ref.assert_conditions((pred, gt), scales=(sc,))
    ref = depth_ref.depth_metrics_ref(pred.numpy(), gt.numpy(), sc, LO, HI)
    e32 = depth_ref.depth_metrics_ref(pred.numpy(), gt.numpy(), sc, LO, HI, dtype=np.float32)["out"][:7]
    return pred, gt, ref, e32


def _run(pred, gt, sc=1.0, lo=LO, hi=HI, planes=True):
    """One nerf_depth_metrics call on [B,h,w] / [B,H,W] views -> (out [B,11], depth or None, mask or None)."""
    n, gh, gw = gt.shape
    out = torch.empty(n, 11, dtype=torch.float64, device=gt.device)
    work = torch.empty(_hip.depth_metrics_workspace_bytes(n, gh, gw), dtype=torch.uint8, device=gt.device)
    depth = torch.empty(n, gh, gw, device=gt.device) if planes else None
    mask = torch.empty(n, gh, gw, dtype=torch.uint8, device=gt.device) if planes else None
    _hip.depth_metrics(pred, gt, sc, lo, hi, out, work, depth, mask)
    return out, depth, mask


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("sc", SCALES)
@pytest.mark.parametrize("case", CASES)
def test_accuracy_and_planes(dev, case, sc):
    pred, gt, ref, e32 = _truth(case, sc)
    out, depth, mask = _run(pred.to(dev)[None], gt.to(dev)[None], sc)
    got = out[0].cpu().numpy()
    name = "depth_metrics_" + ("crafted" if case == "crafted" else "x".join(map(str, case)))
    for k, metric in enumerate(metrics.DEPTH_METRIC_NAMES[:4]):
        e_hip, e_ref = abs(got[k] - ref["out"][k]), abs(e32[k] - ref["out"][k])
        report_err(name, f"{metric}_ref_f32", e_ref)
        report_err(name, f"{metric}_hip", e_hip)
        print(f"{name} sc={sc} {metric}: e_hip={e_hip:.3e} e_ref={e_ref:.3e} ref={ref['out'][k]:.9g}")
    depth_ref.check_against_ref(got, ref["out"], (case, sc))
    if case == "crafted" and sc == 1.0:
        named = dict(zip(metrics.DEPTH_METRIC_NAMES, got.tolist()))
        for k, v in depth_ref.CRAFTED_COUNTS.items():
            assert named[k] == v, (k, named[k], v)
    # the planes, bitwise the CPU restatement's
    assert np.array_equal(depth[0].cpu().numpy().view(np.int32), ref["depth"].view(np.int32))
    assert np.array_equal(mask[0].cpu().numpy(), ref["mask"])
    # the public surface returns the same bits, with and without planes
    pub, pub_depth, pub_mask = metrics.depth_metrics(pred.to(dev), gt.to(dev), LO, HI, sc=sc, planes=True)
    assert pub.shape == (11,) and _same((pub, pub_depth, pub_mask), (out[0], depth[0], mask[0]))
    assert _same((metrics.depth_metrics(pred.to(dev), gt.to(dev), LO, HI, sc=sc),), (out[0],))


def test_layouts_give_identical_bits(dev):
    pred, gt = (t.to(dev) for t in depth_ref.make_depth_pair(47, 155, 23, 61))
    base = _run(pred[None], gt[None], 1.7)
    # a non-contiguous crop of a larger tensor
    big = torch.rand(1, 47 + 7, 155 + 9, device=dev)
    big[:, 3:50, 5:160] = pred
    crop = big[:, 3:50, 5:160]
    assert not crop.is_contiguous()
    assert _same(_run(crop, gt[None], 1.7), base)
    # a column-strided ground-truth view
    wide = torch.rand(1, 23, 2 * 61, device=dev)
    wide[:, :, ::2] = gt
    cols = wide[:, :, ::2]
    assert cols.stride(2) == 2
    assert _same(_run(pred[None], cols, 1.7), base)
    assert _same(_run(crop, cols, 1.7), base)
    # a transposed prediction (row stride 1)
    assert _same(_run(pred.t().contiguous().t()[None], gt[None], 1.7), base)
    # the [h,w] / [1,h,w] forms of the public surface
    one = metrics.depth_metrics(pred, gt, LO, HI, sc=1.7, planes=True)
    assert one[0].shape == (11,) and one[1].shape == gt.shape and _same(one, [t[0] for t in base])
    three = metrics.depth_metrics(crop, cols, LO, HI, sc=1.7, planes=True)
    assert three[0].shape == (1, 11) and _same(three, base)
    mixed = metrics.depth_metrics(pred, cols, LO, HI, sc=1.7)
    assert mixed.shape == (1, 11) and _same((mixed,), base[:1])
    with pytest.raises(RuntimeError):
        metrics.depth_metrics(pred.double(), gt.double(), LO, HI)


def test_batch_of_three_equals_single_calls(dev):
    pairs = [depth_ref.make_depth_pair(33, 45, 50, 70, seed) for seed in (1, 2, 3)]
    pr3 = torch.stack([p for p, _ in pairs]).to(dev)
    gt3 = torch.stack([g for _, g in pairs]).to(dev)
    out3, depth3, mask3 = _run(pr3, gt3, 1.7)
    assert not torch.equal(out3[0], out3[1]) and not torch.equal(out3[1], out3[2]) and not torch.equal(out3[0], out3[2])
    for i in range(3):
        assert _same(_run(pr3[i:i + 1], gt3[i:i + 1], 1.7), (out3[i:i + 1], depth3[i:i + 1], mask3[i:i + 1]))
        ref = depth_ref.depth_metrics_ref(pairs[i][0].numpy(), pairs[i][1].numpy(), 1.7, LO, HI)
        depth_ref.check_against_ref(out3[i].cpu().numpy(), ref["out"], i)
    assert _same((metrics.depth_metrics(pr3, gt3, LO, HI, sc=1.7),), (out3,))


def test_deterministic_bits(dev):
    pred, gt = (t.to(dev)[None] for t in depth_ref.make_depth_pair(*BIG))
    assert _hip.depth_metrics_workspace_bytes(1, BIG[2], BIG[3]) > 64 * 11 * 8     # the final kernel's strided loop
    a, b = _run(pred, gt, 1.7), _run(pred, gt, 1.7)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
    assert _same(a, b)


def test_no_valid_pixel(dev):
    pred, gt = (t.to(dev)[None] for t in depth_ref.make_depth_pair(5, 7, 11, 13))
    want = depth_ref.depth_metrics_ref(pred[0].cpu().numpy(), np.full((11, 13), 50.0, np.float32), 1.0, LO, HI)["out"]
    for bad in (50.0, 0.0, float("nan"), float("inf"), -3.0):
        out, _, mask = _run(pred, torch.full_like(gt, bad))
        got = out[0].cpu().numpy()
        assert np.isnan(got[:7]).all() and got[7] == 0 and got[8] == 0
        assert np.array_equal(got[7:], want[7:]) and got[9] > 0 and got[10] > 0
        assert int((mask & 2).sum()) == 0
    # every rendered pixel out of range as well: everything is a true negative
    out, _, _ = _run(torch.full_like(pred, 100.0), torch.full_like(gt, 50.0))
    assert out[0, 7:].tolist() == [0.0, 0.0, 0.0, 11.0 * 13.0] and torch.isnan(out[0, :7]).all()


@pytest.mark.parametrize("shape", [(5, 7, 11, 13), (33, 45, 33, 45)])
def test_no_stray_writes(dev, shape):
    """out, both planes and the workspace sit between guard bands of a sentinel; the guards are intact
    after the call and every output element was written."""
    pred, gt = (t.to(dev)[None] for t in depth_ref.make_depth_pair(*shape))
    H, W = shape[2:]
    out = Guarded((1, 11), dev, dtype=torch.float64)
    depth = Guarded((1, H, W), dev)
    mask = Guarded((1, H, W), dev, dtype=torch.uint8, fill=0xA5)
    work = Guarded((_hip.depth_metrics_workspace_bytes(1, H, W),), dev, dtype=torch.uint8, fill=0xA5)
    _hip.depth_metrics(pred, gt, 1.7, LO, HI, out.t, work.t, depth.t, mask.t)
    for g in (out, depth, mask, work):
        assert g.intact()
    assert (out.t != SENT).all() and (depth.t != SENT).all() and (mask.t != 0xA5).all()
    assert _same((out.t, depth.t, mask.t), _run(pred, gt, 1.7))
    # without planes: the same numbers, nothing else written
    out2 = Guarded((1, 11), dev, dtype=torch.float64)
    _hip.depth_metrics(pred, gt, 1.7, LO, HI, out2.t, work.t)
    assert out2.intact() and work.intact() and _same((out2.t,), (out.t,))


def test_eval_metrics_one_frame(dev, tmp_path, monkeypatch):
    """Eval_Images.eval_metrics on a small seeded field: the counts of eval_images' confusion matrix,
    the very depths eval_images selects, and no file."""
    from model.eval_images import Eval_Images
    from model.official_nerf import OfficialStaticNerf
    from model.rendering import Renderer
    from tests.helpers import camera_K, make_cfg, rigid_c2w
    h, w, H, W, S, hidden = 12, 20, 25, 41, 32, 64
    cfg = make_cfg(hidden=hidden, S=S)
    cfg["extract_images"] = {"resolution": [h, w]}
    torch.manual_seed(3)
    rnd = Renderer(OfficialStaticNerf(cfg).to(dev), cfg["rendering"], device=dev)
    K = camera_K(h, w, 30.0, 30.0)
    c2ws = torch.stack([rigid_c2w(5, 0.2), rigid_c2w(6, 0.2)]).to(dev)
    g = torch.Generator().manual_seed(11)
    data = {"img": torch.rand(1, 3, h, w, generator=g), "img.gt_depths": 0.05 + 25.0 * torch.rand(1, H, W, generator=g),
            "img.idx": torch.tensor([1]), "img.camera_mat": K, "img.scale_mat": torch.eye(4).unsqueeze(0)}
    ev = Eval_Images(rnd, cfg, use_learnt_poses=True, use_learnt_focal=False, device=dev, render_type="nope_nerf",
                     c2ws=c2ws)
    renders = []
    render = Eval_Images.render_frame

    def recording(self, *args):
        renders.append(render(self, *args))
        return renders[-1]

    monkeypatch.setattr(Eval_Images, "render_frame", recording)
    # the rendered depth's median lands mid-range, so that the selection is not empty
    with torch.no_grad():
        probe = ev.render_frame(K.to(dev), torch.inverse(c2ws[1]).unsqueeze(0), data["img.scale_mat"].to(dev), 1000)[1]
    sc = 5.0 / float(probe.median())
    renders.clear()

    empty = tmp_path / "cwd"
    empty.mkdir()
    cwd = os.getcwd()
    os.chdir(empty)
    try:
        rec = ev.eval_metrics(data, None, it=1000, sc=sc)
    finally:
        os.chdir(cwd)
    assert list(empty.iterdir()) == []
    assert rec["image"].is_cuda and rec["depth"].is_cuda and rec["depth"].dtype == torch.float64
    out = ev.eval_images(data, str(tmp_path / "render"), None, None, None, it=1000, sc=sc)
    assert len(renders) == 2 and torch.equal(renders[0][1], renders[1][1])

    counts = rec["depth"][7:].cpu().numpy()
    print("eval_metrics counts tp, fn, fp, tn:", counts.tolist())
    assert counts.sum() == H * W and counts[0] >= 1
    assert np.array_equal(counts.reshape(2, 2), np.rint(out["conf_mat"] * (H * W - 1)))
    assert np.array_equal(Eval_Images.summarise([rec])["conf_mat"], out["conf_mat"])
    assert rec["image"].tolist() == [out["mse"], out["ssim"]]
    # the planes' selected values are the depths eval_images hands to compute_errors, bit for bit
    gt = data["img.gt_depths"][0].to(dev)
    again, depth, mask = metrics.depth_metrics(renders[0][1], gt, 0.1, 20, sc=sc, planes=True)
    assert torch.equal(again.view(torch.int64), rec["depth"].view(torch.int64))
    sel = (mask == 3).cpu().numpy()
    assert np.array_equal(depth.cpu().numpy()[sel].view(np.int32), out["depth_pred"].view(np.int32))
    assert np.array_equal(gt.cpu().numpy()[sel], out["depth_gt"])
    ref = depth_ref.errors(out["depth_gt"], out["depth_pred"], np.float64)
    depth_ref.check_against_ref(rec["depth"].cpu().numpy(), np.concatenate([ref, counts]))
