"""Test-time pose refinement, the parts that need no GPU: the names evaluation/eval.py:117-141
imports resolve, and the three frozen-field entry points refuse bad arguments on the host,
before any HIP call."""
import ctypes
import importlib
import os

import pytest

from model import _hip


def test_trainer_pose_resolves():
    """evaluation/eval.py:125 builds mdl.Trainer_pose; the class lives in
    model/eval_pose_one_epoch.py as in the reference."""
    import model as mdl
    cls = importlib.import_module("model.eval_pose_one_epoch").Trainer_pose
    assert mdl.Trainer_pose is cls
    t = cls(None, {"n_points": 96, "type": "nope_nerf"}, None, None, None, None)
    assert t.n_points == 96 and t.rendering_technique == "nope_nerf" and t.inject is None
    for name in ("train_step", "compute_loss", "process_data_dict"):
        assert callable(getattr(cls, name))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_hip.LIB_PATH):
        pytest.fail(f"library not built at {_hip.LIB_PATH}; run __graft_entry__.build()")
    return _hip.load_library()


def test_new_symbols_are_bound_within_abi_15(lib):
    assert lib.nerf_hip_abi_version() == 15
    for n in ("nerf_mlp_chain_frozen", "nerf_mlp_chain_bwd_rays", "nerf_field_backward_rays",
              "nerf_field_bwd_rays_workspace_bytes"):
        assert n in _hip.EXPORTED_SYMBOLS and hasattr(lib, n)
    # graw4, three D_i with row maxima, three encoding gradients: far below ten D_i
    rays, full = lib.nerf_field_bwd_rays_workspace_bytes(384), lib.nerf_field_bwd_workspace_bytes(384, 1)
    assert 384 * 4 * (4 + 128 + 2 * 256 + 3 + 3 * 64) <= rays < full // 2
    assert lib.nerf_field_bwd_rays_workspace_bytes(100) == 0


P = 4096   # a non-NULL, 16-byte aligned stand-in for a device pointer (never dereferenced on the host)


def _layers(out=None, cmax=None, at=3):
    ls = []
    for l in range(10):
        ls.append(_hip.ChainLayer(P, 128 if l == 9 else 256, P, out if l == at else None, 256,
                                  None if l == 8 else P, 8, cmax if l == at else None))
    return (_hip.ChainLayer * 10)(*ls)


def test_chain_frozen_refuses_saves(lib):
    for kw, word in (({"out": P}, b"out"), ({"cmax": P}, b"cmax")):
        rc = lib.nerf_mlp_chain_frozen(P, P, P, P, 384, _layers(**kw), P, P, P, P, P, None)
        assert rc == -1
        msg = lib.nerf_hip_last_error()
        assert b"nerf_mlp_chain_frozen" in msg and b"layer 3" in msg and word in msg, msg
    assert lib.nerf_mlp_chain_frozen(P, P, P, P, 100, _layers(), P, P, P, P, P, None) == -1
    assert b"n_pad" in lib.nerf_hip_last_error()
    assert lib.nerf_mlp_chain_frozen(P, P, P, P, 384, None, P, P, P, P, P, None) == -1


def _chain_bwd(extra=None):
    c = _hip.ChainBwd()
    c.graw4 = c.hr_mask = c.wd = c.wc = P
    c.ld_hr_mask = 4
    c.n_pad = 384
    for i in range(9):
        c.wt_img[i] = P
        c.wt_img_rows[i] = 320 if i in (0, 5) else 256
        c.in_mask[i] = P
        c.ld_in_mask[i] = 8
    for i in (0, 5, 9):
        c.dy[i] = P
        c.lddy[i] = 128 if i == 0 else 256
        c.dy_rmax[i] = P
    if extra:
        getattr(c, extra[0])[extra[1]] = P
    return c


def test_chain_bwd_rays_refuses_other_outputs(lib):
    for field, i in (("dy", 1), ("dy_rmax", 4), ("dy_cmax", 6), ("dy_cmax", 5)):
        c = _chain_bwd((field, i))
        assert lib.nerf_mlp_chain_bwd_rays(ctypes.addressof(c), None) == -1, (field, i)
        msg = lib.nerf_hip_last_error()
        assert b"nerf_mlp_chain_bwd_rays" in msg and f"D_{i}".encode() in msg, msg
    c = _chain_bwd()
    c.dy[5] = None
    assert lib.nerf_mlp_chain_bwd_rays(ctypes.addressof(c), None) == -1 and b"D_5" in lib.nerf_hip_last_error()
    assert lib.nerf_mlp_chain_bwd_rays(None, None) == -1


def test_field_backward_rays_refuses_missing_workspace(lib):
    a = _hip.FieldBwdRays()
    a.n_pad, a.n_rays, a.n_samples = 384, 12, 32
    for f in ("z", "raw4", "pts_o", "pts_d", "view", "wd", "wc", "g_rgb", "g_dist", "g_pts_o", "g_pts_d", "g_view"):
        setattr(a, f, P)
    for l in range(10):
        a.mask[l] = None if l == 8 else P
        a.wt[l] = a.wt_img[l] = a.wt_cimg[l] = P
    assert lib.nerf_field_backward_rays(ctypes.addressof(a), None) == -1
    assert b"workspace" in lib.nerf_hip_last_error()
    a.workspace = P
    a.g_view = None
    assert lib.nerf_field_backward_rays(ctypes.addressof(a), None) == -1
    assert b"gradient outputs" in lib.nerf_hip_last_error()
    assert lib.nerf_field_backward_rays(None, None) == -1
