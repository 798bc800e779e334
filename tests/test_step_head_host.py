"""nerf_step_head's argument checks (include/nerf_hip.h): each returns NERF_EINVAL with a telling
message before any HIP call, so none of this needs a GPU."""
import ctypes
import os

import pytest

from model import _hip

P = ctypes.c_void_p(16)     # a non-null pointer the entry never dereferences on these paths


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_hip.LIB_PATH):
        pytest.fail(f"library not built at {_hip.LIB_PATH}; run __graft_entry__.build()")
    return _hip.load_library()


def _rays(**over):
    kw = dict(r=P, t=P, init_c2w=P, K=P, scale=P, img=P, depth_map=P, aff_scale=P, aff_shift=P, seed=7,
              n_pix=32 * 64, n_rays=1024, width=64, height=32, shift_first=0, flags=1, lo=float("-inf"),
              c2w=P, world=P, M=P, inverses=P, idx=P, pixels=P, rgb=P, status=P, depth_g=P, depth_d=P,
              cam=P, ray=P, view=P, ray_norm=P, d_src=P, mask=P)
    kw.update(over)
    return _hip.StepHeadRays(**{k: v for k, v in kw.items() if v is not None})


def _desc():
    return _hip.PackDesc(P, P, None, 4, 4, 4, 0, 0)


def _fails(lib, rays, descs, n, word):
    arr = (_hip.PackDesc * max(len(descs), 1))(*descs)
    rc = lib.nerf_step_head(None if rays is None else ctypes.byref(rays), arr if descs else None, n, None)
    msg = lib.nerf_hip_last_error()
    assert rc == -1, (rc, msg)
    assert b"nerf_step_head" in msg and word in msg, msg


def test_both_parts_absent(lib):
    _fails(lib, None, [], 0, b"neither")


def test_too_many_rays(lib):
    _fails(lib, _rays(n_rays=_hip.SAMPLE_MAX_RAYS + 1, n_pix=128 * 128, width=128, height=128), [], 0, b"n_rays=4097")


def test_too_few_pixels(lib):
    _fails(lib, _rays(n_rays=1025), [], 0, b"2*n_rays")


def test_too_many_descriptors(lib):
    _fails(lib, None, [_desc()] * 25, 25, b"n_desc=25")
    _fails(lib, _rays(), [_desc()] * 25, 25, b"n_desc=25")


@pytest.mark.parametrize("name", ["c2w", "world", "M", "inverses", "idx", "pixels", "rgb", "cam", "ray", "ray_norm",
                                  "d_src", "depth_g", "depth_d"])
def test_null_required_output(lib, name):
    _fails(lib, _rays(**{name: None}), [], 0, b"'" + name.encode() + b"'")


def test_optional_outputs_need_their_inputs(lib):
    # without a depth map neither depth output is required; an affine needs the map and its shift
    _fails(lib, _rays(depth_map=None, aff_scale=P, depth_g=None, depth_d=None), [], 0, b"aff_scale")
    _fails(lib, _rays(aff_shift=None), [], 0, b"aff_scale")
    _fails(lib, _rays(r=None, c2w_in=None), [], 0, b"pose")
    _fails(lib, _rays(t=None), [], 0, b"pose")
    _fails(lib, _rays(img=None), [], 0, b"img")


def test_pack_descriptor_checks_are_those_of_pack_weights(lib):
    bad = _hip.PackDesc(P, P, None, 4, 8, 4, 0, 0)      # ld_dst < cols
    _fails(lib, None, [bad], 1, b"bad descriptor 0")
    _fails(lib, _rays(), [_desc(), bad], 2, b"bad descriptor 1")
