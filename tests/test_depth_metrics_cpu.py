"""Depth metrics of the novel-view evaluation, the parts that need no GPU: the two C-ABI entries
resolve and refuse bad arguments on the host before any HIP call, the CPU path of
metrics.depth_metrics equals the fp64 restatement (tests/depth_ref.py), the restatement's checker
rejects three wrong variants, and Eval_Images.eval_metrics / summarise give the numbers of
eval_images on a fixed frame."""
import os

import numpy as np
import pytest
import torch

from model import _hip, metrics
from model.common import compute_errors
from model.metrics import resize_nearest_exact
from tests import depth_ref
from tests.depth_ref import HI, LO, SCALES, SHAPES

CASES = [pytest.param(s, id="x".join(map(str, s))) for s in SHAPES] + [pytest.param("crafted", id="crafted")]


def _pair(case):
    if case == "crafted":
        return depth_ref.crafted_pair()
    pair = depth_ref.make_depth_pair(*case)
    depth_ref.assert_conditions(pair)
    return pair


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_hip.LIB_PATH):
        pytest.fail(f"library not built at {_hip.LIB_PATH}; run __graft_entry__.build()")
    return _hip.load_library()


def test_abi(lib):
    assert lib.nerf_hip_abi_version() == 15
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "nerf_hip.h")).read()
    for n in ("nerf_depth_metrics", "nerf_depth_metrics_workspace_bytes"):
        assert n in _hip.EXPORTED_SYMBOLS and hasattr(lib, n) and n + "(" in header
    ws = lib.nerf_depth_metrics_workspace_bytes
    for zero in ((0, 375, 1242), (1, 0, 1242), (1, 375, 0), (-1, 375, 1242), (1, -3, 5)):
        assert ws(*zero) == 0
    assert ws(1, 1, 1) == 11 * 8                                   # eleven doubles per block of pixels
    assert ws(1, 375, 1242) > 64 * 11 * 8                          # the final kernel's strided loop runs
    assert ws(1, 375, 1242) < ws(2, 375, 1242) < ws(3, 375, 1242) and ws(3, 33, 45) == 3 * ws(1, 33, 45)
    assert _hip.depth_metrics_workspace_bytes(2, 33, 45) == ws(2, 33, 45)


P = 4096   # a non-NULL, aligned stand-in for a device pointer (never dereferenced on the host)


def _call(lib, pred=P, gt=P, h=12, w=20, H=25, W=41, batch=1, sc=1.0, min_depth=0.1, max_depth=20.0, out=P,
          workspace=P):
    return lib.nerf_depth_metrics(pred, h * w, w, 1, h, w, gt, H * W, W, 1, H, W, batch, sc, min_depth, max_depth, out,
                                  None, None, workspace, None)


@pytest.mark.parametrize("kw,word", [
    ({"pred": None}, b"pred"), ({"gt": None}, b"gt"), ({"out": None}, b"out"), ({"workspace": None}, b"workspace"),
    ({"h": 0}, b"h="), ({"w": -1}, b"w="), ({"H": 0}, b"H="), ({"W": 0}, b"W="), ({"batch": 0}, b"batch"),
    ({"H": 65536, "W": 32768}, b"H * W"), ({"H": 46341, "W": 46341}, b"H * W"),
    ({"sc": float("nan")}, b"sc"), ({"sc": float("inf")}, b"sc"), ({"sc": float("-inf")}, b"sc"),
    ({"min_depth": 0.0}, b"min_depth"), ({"min_depth": -1.0}, b"min_depth"), ({"min_depth": float("nan")}, b"min_depth"),
    ({"max_depth": 0.05}, b"max_depth"), ({"max_depth": float("nan")}, b"max_depth"),
])
def test_refusals(lib, kw, word):
    assert _call(lib, **kw) == -1
    msg = lib.nerf_hip_last_error()
    assert b"nerf_depth_metrics" in msg and word in msg, msg


def test_binding_refuses_cpu_tensors():
    pred, gt = torch.ones(1, 3, 4), torch.ones(1, 5, 6)
    out, work = torch.empty(1, 11, dtype=torch.float64), torch.empty(88, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        _hip.depth_metrics(pred, gt, 1.0, LO, HI, out, work)


@pytest.mark.parametrize("sc", SCALES)
@pytest.mark.parametrize("case", CASES)
def test_cpu_path_equals_the_restatement(case, sc):
    pred, gt = _pair(case)
    ref = depth_ref.depth_metrics_ref(pred.numpy(), gt.numpy(), sc, LO, HI)
    out, depth, mask = metrics.depth_metrics(pred, gt, LO, HI, sc=sc, planes=True)
    assert out.dtype == torch.float64 and out.shape == (11,)
    depth_ref.check_against_ref(out.numpy(), ref["out"], (case, sc))
    # the planes: resize_nearest_exact(pred * f32(sc)) and the two masks, bitwise
    want = resize_nearest_exact(pred.numpy() * np.float32(sc), tuple(gt.shape))
    assert depth.dtype == torch.float32 and mask.dtype == torch.uint8 and depth.shape == mask.shape == gt.shape
    assert np.array_equal(depth.numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(depth.numpy().view(np.int32), ref["depth"].view(np.int32))
    assert np.array_equal(mask.numpy(), ref["mask"])
    # the batched forms return the same row
    assert torch.equal(metrics.depth_metrics(pred[None], gt[None], LO, HI, sc=sc)[0].view(torch.int64),
                       out.view(torch.int64))
    assert torch.equal(metrics.depth_metrics(pred, gt, LO, HI, sc=sc).view(torch.int64), out.view(torch.int64))


def test_crafted_set_counts():
    """The boundary pixels fall where the definition puts them: both bounds inclusive, one f32 step
    outside is out, a ratio exactly at a threshold is not counted by the strict <."""
    pred, gt = depth_ref.crafted_pair()
    out = dict(zip(metrics.DEPTH_METRIC_NAMES, metrics.depth_metrics(pred, gt, LO, HI).tolist()))
    for k, v in depth_ref.CRAFTED_COUNTS.items():
        assert out[k] == v, (k, out[k], v)
    ref = dict(zip(metrics.DEPTH_METRIC_NAMES, depth_ref.depth_metrics_ref(pred.numpy(), gt.numpy(), 1.0, LO, HI)["out"]))
    for k, v in depth_ref.CRAFTED_COUNTS.items():
        assert ref[k] == v, (k, ref[k], v)


def test_no_valid_pixel_and_bad_arguments():
    pred, gt = depth_ref.make_depth_pair(5, 7, 11, 13)
    out = metrics.depth_metrics(pred, torch.full_like(gt, 50.0), LO, HI)
    assert torch.isnan(out[:7]).all() and out[7].item() == 0 and out[7:].sum().item() == 11 * 13
    assert out[8].item() == 0 and out[9].item() > 0 and out[10].item() > 0
    assert len(metrics.DEPTH_METRIC_NAMES) == 11 and metrics.DEPTH_METRIC_NAMES[7:] == ("tp", "fn", "fp", "tn")
    for kw in ({"min_depth": 0.0}, {"max_depth": 0.01}, {"sc": float("nan")}):
        args = dict(min_depth=LO, max_depth=HI, sc=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            metrics.depth_metrics(pred, gt, **args)
    with pytest.raises(ValueError):
        metrics.depth_metrics(pred[None].expand(2, -1, -1), gt[None], LO, HI)


# ---- the checker has teeth: three wrong variants of the definition ------------------------------------
def _variant(pred, gt, sc, lo, hi, wrong):
    """The definition of depth_ref.depth_metrics_ref in fp64 with one thing wrong."""
    g = np.asarray(gt, dtype=np.float32)
    d = np.asarray(pred, dtype=np.float32) * np.float32(sc)
    H, W = g.shape
    h, w = d.shape
    if wrong == "floor_index":                                   # floor(Y h / H) instead of the pixel centre
        iy, ix = (np.arange(H) * h) // H, (np.arange(W) * w) // W
        d = d[iy[:, None], ix[None, :]]
    else:
        d = resize_nearest_exact(d, (H, W))
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        if wrong == "exclusive_upper":
            mr, mg = (d >= lo) & (d < hi), (g >= lo) & (g < hi)
        else:
            mr, mg = (d >= lo) & (d <= hi), (g >= lo) & (g <= hi)
    sel = mr & mg
    e = depth_ref.errors(g[sel], d[sel], np.float64)
    if wrong == "mean_over_all":                                 # means over every pixel, not the selection
        n, tp = g.size, sel.sum()
        e = np.array([e[0] * tp / n, e[1] * tp / n, np.sqrt(e[2] ** 2 * tp / n), np.sqrt(e[3] ** 2 * tp / n),
                      e[4] * tp / n, e[5] * tp / n, e[6] * tp / n])
    counts = [sel.sum(), (~mr & mg).sum(), (mr & ~mg).sum(), (~mr & ~mg).sum()]
    return np.concatenate([e, np.array(counts, dtype=np.float64)])


def _upper_bound_on_a_pixel(pred, gt):
    """An upper bound that a selected ground-truth pixel sits on exactly (the largest selected value
    below the median of the selection), so that an exclusive bound shows."""
    ref = depth_ref.depth_metrics_ref(pred.numpy(), gt.numpy(), 1.0, LO, HI)
    vals = np.sort(gt.numpy()[ref["sel"]])
    return float(vals[len(vals) // 2])


@pytest.mark.parametrize("wrong", [None, "floor_index", "exclusive_upper", "mean_over_all"])
def test_the_checker_has_teeth(wrong):
    failed = []
    for shape in SHAPES:
        pred, gt = depth_ref.make_depth_pair(*shape)
        hi = _upper_bound_on_a_pixel(pred, gt) if wrong in (None, "exclusive_upper") else HI
        for sc in SCALES:
            ref = depth_ref.depth_metrics_ref(pred.numpy(), gt.numpy(), sc, LO, hi)["out"]
            try:
                depth_ref.check_against_ref(_variant(pred.numpy(), gt.numpy(), sc, LO, hi, wrong), ref)
            except AssertionError:
                failed.append((shape, sc))
    if wrong is None:
        assert not failed, failed                                # the right definition passes everywhere
    else:
        assert failed, f"the checker accepts the wrong variant {wrong} on every shape"
        print(f"{wrong}: rejected on {len(failed)} of {2 * len(SHAPES)} cases")


def test_crafted_set_rejects_an_exclusive_bound():
    pred, gt = depth_ref.crafted_pair()
    ref = depth_ref.depth_metrics_ref(pred.numpy(), gt.numpy(), 1.0, LO, HI)["out"]
    depth_ref.check_against_ref(_variant(pred.numpy(), gt.numpy(), 1.0, LO, HI, None), ref)
    with pytest.raises(AssertionError):
        depth_ref.check_against_ref(_variant(pred.numpy(), gt.numpy(), 1.0, LO, HI, "exclusive_upper"), ref)


# ---- Eval_Images.eval_metrics / summarise on a stub renderer ------------------------------------------
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
    return frame, depth, data


def _evaluator(monkeypatch, frame, depth):
    from model.eval_images import Eval_Images
    seen = []

    def fixed(self, camera_mat, world_mat, scale_mat, it):
        seen.append(dict(camera_mat=camera_mat, world_mat=world_mat, it=it))
        return frame, depth

    monkeypatch.setattr(Eval_Images, "render_frame", fixed)
    rnd = _StubRenderer()
    ev = Eval_Images(rnd, {"extract_images": {"resolution": [12, 20]}}, use_learnt_poses=True, use_learnt_focal=True,
                     device=None, render_type="nope_nerf", c2ws=torch.eye(4).repeat(5, 1, 1))
    return ev, rnd, seen


def test_eval_metrics_and_summarise(monkeypatch, tmp_path):
    from model.eval_images import Eval_Images
    frame, depth, data = _host_case()
    depth_before = depth.clone()
    ev, rnd, seen = _evaluator(monkeypatch, frame, depth)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        rec = ev.eval_metrics(data, (30.0, 31.0), min_depth=0.1, max_depth=20, it=9, sc=2)
    finally:
        os.chdir(cwd)
    assert list(tmp_path.iterdir()) == []                        # no file
    assert rnd.training is False and torch.equal(depth, depth_before)
    assert set(rec) == {"image", "depth"}
    assert rec["image"].shape == (2,) and rec["image"].dtype == torch.float32
    assert rec["depth"].shape == (11,) and rec["depth"].dtype == torch.float64

    out = ev.eval_images(data, str(tmp_path), (30.0, 31.0), None, None, min_depth=0.1, max_depth=20, it=9, sc=2)
    assert set(out) == {"img", "mse", "psnr", "ssim", "lpips", "depth_pred", "depth_gt", "conf_mat"}
    # the same pose, focal and iteration reached the renderer both times
    assert seen[0]["it"] == seen[1]["it"] == 9
    assert torch.equal(seen[0]["camera_mat"], seen[1]["camera_mat"]) and torch.equal(seen[0]["world_mat"], seen[1]["world_mat"])
    assert rec["image"].tolist() == [out["mse"], out["ssim"]]

    # the confusion matrix: the same integers, and summarise's quirky divisor gives eval_images' matrix
    n = 24 * 40
    counts = rec["depth"][7:].numpy()
    assert counts.sum() == n and counts.min() >= 1
    assert np.array_equal(counts.reshape(2, 2), np.rint(out["conf_mat"] * (n - 1)))
    table = Eval_Images.summarise([rec])
    assert np.array_equal(table["conf_mat"], out["conf_mat"])
    assert table["mse"] == out["mse"] and table["ssim"] == out["ssim"] and table["psnr"] == float(out["psnr"])

    # the seven errors: fp64 of the very values eval_images returns, so within the float32
    # compute_errors' own distance from fp64 of what the reference would print
    assert out["depth_gt"].dtype == np.float32 and out["depth_pred"].dtype == np.float32
    e64 = np.array(compute_errors(out["depth_gt"].astype(np.float64), out["depth_pred"].astype(np.float64)))
    e32 = np.array([float(v) for v in compute_errors(out["depth_gt"], out["depth_pred"])])
    got = rec["depth"][:7].numpy()
    depth_ref.check_against_ref(rec["depth"].numpy(), np.concatenate([e64, counts]))
    for k, name in enumerate(metrics.DEPTH_METRIC_NAMES[:7]):
        own = abs(e32[k] - e64[k])
        assert abs(got[k] - e32[k]) <= own + 2.0 ** -30 * max(1.0, abs(e64[k])), (name, got[k], e32[k], e64[k])
        assert table[name] == got[k]

    # two frames: the means of the rows
    rec2 = {"image": rec["image"] * 2, "depth": torch.cat([rec["depth"][:7] * 3, rec["depth"][7:]])}
    two = Eval_Images.summarise([rec, rec2])
    assert two["mse"] == pytest.approx(1.5 * out["mse"], rel=1e-12) and two["abs_rel"] == pytest.approx(2 * got[0], rel=1e-12)
    assert np.array_equal(two["conf_mat"], out["conf_mat"])
    with pytest.raises(ValueError):
        Eval_Images.summarise([])


def test_eval_metrics_without_gt_depths(monkeypatch):
    """A missing img.gt_depths falls back to img.depth (eval_images.py:53-57)."""
    frame, depth, data = _host_case()
    ev, _, _ = _evaluator(monkeypatch, frame, depth)
    want = ev.eval_metrics(data, (30.0, 31.0), sc=2)["depth"]
    data["img.depth"] = data.pop("img.gt_depths")
    got = ev.eval_metrics(data, (30.0, 31.0), sc=2)["depth"]
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
