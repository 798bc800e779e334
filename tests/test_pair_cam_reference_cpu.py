"""The staged reference of the camera-matrix gradient (tests/pair_cam_ref.py) checked on the CPU: the sum of
the per-point K leaf's gradients is fp64 autograd of one shared K leaf; a torch-f32 emulation of the
kernel's per-point accumulation passes the bars of the GPU module; each of four wrong kernels fails them on
the "full" camera; nerf_pair_backward_cam is declared, exported and refuses NULL pointers before any HIP
call."""
import ctypes
import os

import pytest
import torch

from model import _hip
from tests import helpers as H
from tests import pair_cam_ref as C

SETS = ((2, 2, "diag"), (19, 27, "principal"), (19, 27, "full"), (47, 155, "skew"))


def _nn_and_dec(inp):
    return C.emulation_nn(inp), H.pair_decisions(inp)


@pytest.mark.parametrize("h,w,cam", SETS[:3])
def test_per_point_leaf_sums_to_the_shared_leaf(h, w, cam):
    """The same function of K: the per-point leaf's summed gradient against one shared leaf, fp64 rounding
    (1e-12 of the condition sum), every combo, detach and both rgb_s terms."""
    inp = H.pair_generic_inputs(h, w, cam)
    nn, dec = _nn_and_dec(inp)
    for combo, detach, ssim in C.cam_runs(True):
        go_pc, go_rgbs = H.PAIR_COMBOS[combo]
        r = C.pair_cam_loss_ref(inp, nn, dec["valid"], dec["bad"], go_pc, go_rgbs, bool(detach), torch.float64, ssim)
        want = C.shared_leaf_gK(inp, nn, dec["valid"], dec["bad"], go_pc, go_rgbs, bool(detach), ssim)
        assert bool(((r["gK"] - want).abs() <= 1e-12 * r["cond16"]).all()), (combo, detach, ssim)
        assert bool((r["cond16"] >= r["gK"].abs() * (1 - 1e-12)).all())
    r = C.pair_cam_loss_ref(inp, nn, dec["valid"], dec["bad"], 1.0, 0.7, False, torch.float64)
    if cam == "full":
        assert bool((r["cond16"].view(4, 4)[3] > 0).all()), "row 3 of gK has terms under the full camera"
    if cam == "diag":
        assert bool((r["cond16"].view(4, 4)[3] == 0).all()), "inv(K) without a translation column: row 3 is 0"


def test_identity_of_the_inverse_term():
    """-a b^T with a = inv(K)^T[:, :3] g and b = inv(K) v is d/dK of g . (inv(K) v)[:3], fp64 autograd."""
    g = torch.Generator().manual_seed(3)
    K = H.pair_camera("full", 19, 27).double().requires_grad_(True)
    v = torch.rand(4, generator=g, dtype=torch.float64)
    gp = torch.randn(3, generator=g, dtype=torch.float64)
    (gp * (torch.linalg.inv(K) @ v)[:3]).sum().backward()
    Ki = torch.linalg.inv(K.detach())
    want = -torch.outer(Ki[:3].t() @ gp, Ki @ v)
    assert (K.grad - want).abs().max().item() <= 1e-14 * want.abs().max().item()
    assert K.grad[3].abs().min().item() > 0


def test_reference_without_a_live_term():
    """No valid point and go_pc absent: the total carries no grad, the reference returns zeros; a clamped but
    valid point still gives the projection's term."""
    inp = H.pair_no_valid_inputs()
    nn, dec = _nn_and_dec(inp)
    assert not bool(dec["valid"].any())
    for ssim in (False, True):
        r = C.pair_cam_loss_ref(inp, nn, dec["valid"], dec["bad"], None, 0.7, False, torch.float64, ssim)
        assert bool((r["gK"] == 0).all()) and bool((r["cond16"] == 0).all())
    inp = H.pair_generic_inputs(19, 27, "diag", with_img=False)
    nn, dec = _nn_and_dec(inp)
    r = C.pair_cam_loss_ref(inp, nn, dec["valid"], dec["bad"], None, None, False, torch.float64)
    assert bool((r["gK"] == 0).all())
    inp, clamped = H.pair_clamped_inputs()
    nn, dec = _nn_and_dec(inp)
    only = torch.zeros_like(dec["valid"])
    only[clamped] = dec["valid"][clamped]
    assert bool(only.any()) and bool(dec["bad"][clamped].all())
    r = C.pair_cam_loss_ref(inp, nn, only, dec["bad"], None, 0.7, False, torch.float64)
    assert r["cond16"].view(4, 4)[:2].max().item() > 0, "a clamped, valid point projects through K"


@pytest.mark.parametrize("h,w,cam", SETS)
def test_emulation_passes_the_bars(h, w, cam):
    ref = C.check_emulation(H.pair_generic_inputs(h, w, cam))
    for name, r in ref.worst.items():
        H.report_err(f"pair_cam_emulation_{h}x{w}_{cam}", name, r)


def test_emulation_passes_on_the_crafted_sets():
    C.check_emulation(H.pair_clamped_inputs()[0])
    C.check_emulation(H.pair_no_valid_inputs())
    C.check_emulation(H.pair_coincident_inputs()[0])


@pytest.mark.parametrize("wrong", C.CAM_WRONG)
def test_bars_reject_a_wrong_kernel(wrong):
    """The inverse's contribution dropped, only the diagonal entries kept, rgbs_detach_scale ignored for the
    reprojection's pc1, pc2's contribution dropped: the unmodified emulation passes on the full camera, the
    wrong one fails (detach_ignored can only show with detach = 1)."""
    inp = H.pair_generic_inputs(19, 27, "full")
    runs = [("both", 1, False), ("both", 1, True)] if wrong == "detach_ignored" else [("both", 0, False), ("both", 0, True)]
    C.check_emulation(inp, None, runs)
    for run in runs:
        with pytest.raises(AssertionError):
            C.check_emulation(inp, wrong, [run])


def test_backward_cam_is_declared_exported_and_checks_its_pointers():
    """ABI: the header declares it, the library exports it, the binding lists it; NULL pointers and a NULL
    gK16 alone return -1 with a "null" message before any HIP call."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int nerf_pair_backward_cam(" in open(os.path.join(root, "include", "nerf_hip.h")).read()
    assert "nerf_pair_backward_cam" in _hip.EXPORTED_SYMBOLS
    lib = _hip.load_library()
    assert lib.nerf_hip_abi_version() == 15
    fn = lib.nerf_pair_backward_cam
    rc = fn(None, None, 3, 5, None, None, None, 0.01, None, None, 0, None, None, None, *([None] * 10))
    assert rc == -1 and b"null" in lib.nerf_hip_last_error()
    p = ctypes.c_void_p(16)
    rc = fn(p, p, 3, 5, p, p, p, 0.01, p, p, 0, p, p, None, p, p, p, p, p, p, p, None, p, None)
    assert rc == -1
    msg = lib.nerf_hip_last_error()
    assert b"null" in msg and b"gK16" in msg, msg
    rc = fn(p, p, 3, 1, p, p, p, 0.01, p, p, 0, p, p, None, p, p, p, p, p, p, p, p, p, None)
    assert rc == -1 and b"resolution" in lib.nerf_hip_last_error()
