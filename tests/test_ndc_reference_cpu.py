"""The staged NDC reference of tests/ndc_ref.py on the CPU (no GPU needed): it is the reference's
expression bit for bit, its fp64 gradients pass gradcheck, its f32 run is as close to fp64 as the
bars of tests/test_gpu_ndc_fp64.py assume, those bars reject four wrong variants, and the library
exports and binds nerf_ndc_rays / nerf_ndc_rays_bwd with their argument checks."""
import os

import pytest
import torch

from model import _hip
from model import common as mcommon
from oracle import nerf_oracle as orc
from tests import ndc_ref as N


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_hip.LIB_PATH):
        pytest.fail(f"library not built at {_hip.LIB_PATH}; run __graft_entry__.build()")
    return _hip.load_library()


@pytest.mark.parametrize("R", [1, 65, 1025])
def test_reference_is_the_reference_expression(R):
    inp = N.ndc_inputs(R)
    K = inp["K"]
    fxfy = torch.cat([K[None, 0, 0], K[None, 1, 1]])          # rendering.py:170
    assert fxfy.tolist() == [pytest.approx(2.4), pytest.approx(-3.2)]
    want_o, want_d = orc.get_ndc_rays_fxfy(fxfy, 1.0, inp["cam"], inp["ray"])
    mine_o, mine_d = mcommon.get_ndc_rays_fxfy(fxfy, 1.0, inp["cam"], inp["ray"])
    r32 = N.ndc_ref(inp, torch.float32)
    for got_o, got_d in ((mine_o, mine_d), (r32["o_ndc"], r32["d_ndc"]),
                         N.ndc_expr(K[0, 0], K[1, 1], 1.0, inp["cam"], inp["ray"])):
        assert torch.equal(got_o, want_o) and torch.equal(got_d, want_d)
    assert torch.equal(r32["d_gt"], 1 - 1 / inp["d_src"])
    # the shifted origin lies on the near plane: o_ndc z = -1, d_ndc z = 2 up to rounding
    assert (r32["o_ndc"][:, 2] + 1).abs().max() < 1e-6 and (r32["d_ndc"][:, 2] - 2).abs().max() < 1e-6


def test_generic_set_is_what_the_issue_describes():
    inp = N.ndc_inputs(1025)
    cam, ray = inp["cam"], inp["ray"]
    assert bool((cam.abs() <= torch.tensor([0.3, 0.3, 0.2])).all())
    assert bool(((ray.norm(dim=-1) - 1).abs() < 1e-6).all()) and bool((ray[:, 2].abs() >= 0.8 - 1e-6).all())
    for k in range(3):
        assert bool((ray[:, k] > 0).any()) and bool((ray[:, k] < 0).any())
    assert 0.05 <= inp["d_src"].min() and inp["d_src"].max() <= 20.0


def test_f32_reference_is_close_to_fp64():
    """Finite everywhere and within 3e-7 (outputs) / 3e-6 (gradients) of fp64 at R = 1025, relative to
    each tensor's largest entry."""
    inp = N.ndc_inputs(1025)
    r64, r32 = N.ndc_refs(inp)
    for name in N.FWD_NAMES + N.BWD_NAMES:
        a, b = r32[name].double(), r64[name]
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        rel = ((a - b).abs().max() / b.abs().max()).item()
        print(f"{name}: f32 vs f64 {rel:.3e} of the largest entry {b.abs().max().item():.3e}")
        assert rel <= (3e-7 if name in N.FWD_NAMES else 3e-6), (name, rel)


def test_fp64_gradients_pass_gradcheck():
    inp = N.ndc_inputs(5, seed=3)
    d = lambda t: t.double().clone().requires_grad_(True)      # noqa: E731
    f = torch.tensor([2.4, -3.2], dtype=torch.float64, requires_grad=True)

    def fn(cam, ray, f, d_src):
        o, dd = N.ndc_expr(f[0], f[1], 1.0, cam, ray)
        return o, dd, 1 - 1 / d_src

    assert torch.autograd.gradcheck(fn, (d(inp["cam"]), d(inp["ray"]), f, d(inp["d_src"])), eps=1e-6, atol=1e-6)


@pytest.mark.parametrize("combo", list(N.GRAD_COMBOS))
def test_bars_accept_the_f32_reference(combo):
    for R in (1, 65, 1025):
        inp = N.ndc_inputs(R)
        r64, r32 = N.ndc_refs(inp, combo)
        N.check_all(N.emulate_f32(inp, combo), r64, r32, R, f"R={R} {combo}")


@pytest.mark.parametrize("wrong", N.WRONG)
def test_bars_reject_wrong_variants(wrong):
    """No origin shift, near instead of 2 near in o2, +fy, d_gt = 1 / d: each fails a bar."""
    inp = N.ndc_inputs(257)
    r64, r32 = N.ndc_refs(inp)
    with pytest.raises(AssertionError, match="over the bar"):
        N.check_all(N.emulate_f32(inp, "all", _wrong=wrong), r64, r32, 257, wrong)


def test_reduce_room_is_derived_from_the_terms():
    inp = N.ndc_inputs(1025)
    r64, _ = N.ndc_refs(inp)
    room = N.reduce_room(r64, 1025)
    assert room[0, 0] == 1024 * 2.0 ** -24 * r64["fx_terms"].abs().sum().item()
    assert room[1, 1] > 0 and float(room.sum()) == float(room[0, 0] + room[1, 1])
    assert torch.equal(r64["gK"][0, 0], r64["fx_terms"].sum()) and float(r64["gK"].abs().sum()) > 0


def test_entries_are_exported_and_bound(lib):
    """nerf_ndc_rays / nerf_ndc_rays_bwd: in the library, in the binding, ABI still 15."""
    assert lib.nerf_hip_abi_version() == 15 == _hip.ABI_VERSION
    for name in ("nerf_ndc_rays", "nerf_ndc_rays_bwd"):
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _hip.EXPORTED_SYMBOLS
    assert callable(_hip.ndc_rays) and callable(_hip.ndc_rays_bwd)
    from model import rays
    assert callable(rays.ndc_rays) and issubclass(rays._NdcRays, torch.autograd.Function)


def test_argument_checks(lib):
    """-1 with a message on a null required pointer or n_rays <= 0, before any HIP call."""
    p = 16      # a non-null pointer value: the checks return before any use of it
    assert lib.nerf_ndc_rays(None, p, p, 1.0, 4, None, p, p, None, None) == -1
    assert b"cam" in lib.nerf_hip_last_error()
    assert lib.nerf_ndc_rays(p, p, None, 1.0, 4, None, p, p, None, None) == -1
    assert b"'K'" in lib.nerf_hip_last_error()
    assert lib.nerf_ndc_rays(p, p, p, 1.0, 4, None, p, None, None, None) == -1
    assert b"d_ndc" in lib.nerf_hip_last_error()
    assert lib.nerf_ndc_rays(p, p, p, 1.0, 0, None, p, p, None, None) == -1
    assert b"n_rays" in lib.nerf_hip_last_error()
    assert lib.nerf_ndc_rays(p, p, p, 1.0, 4, None, p, p, p, None) == -1
    assert b"d_src" in lib.nerf_hip_last_error()
    assert lib.nerf_ndc_rays_bwd(p, None, p, 1.0, 4, None, p, p, None, p, p, None, None, None) == -1
    assert b"ray" in lib.nerf_hip_last_error()
    assert lib.nerf_ndc_rays_bwd(p, p, p, 1.0, 4, None, p, p, None, None, p, None, None, None) == -1
    assert b"g_cam" in lib.nerf_hip_last_error()
    assert lib.nerf_ndc_rays_bwd(p, p, p, 1.0, -3, None, p, p, None, p, p, None, None, None) == -1
    assert b"n_rays" in lib.nerf_hip_last_error()
    assert lib.nerf_ndc_rays_bwd(p, p, p, 1.0, 4, None, p, p, None, p, p, None, p, None) == -1
    assert b"d_src" in lib.nerf_hip_last_error()


def test_binding_refuses_cpu_tensors(lib):
    inp = N.ndc_inputs(4)
    e = torch.empty(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.ndc_rays(inp["cam"], inp["ray"], inp["K"], 1.0, 4, None, e, e.clone())
    with pytest.raises(RuntimeError, match="GPU"):
        _hip.ndc_rays_bwd(inp["cam"], inp["ray"], inp["K"], 1.0, 4, None, inp["g_o"], None, None, e, e.clone())


def test_first_step_draw_sits_on_a_relu_kink():
    """Why tests/test_gpu_full_step_ndc.py::test_ndc_training_step_matches_oracle hands the field's own ReLU
    decisions to the oracle: in the fp64 oracle of its first step one pre-activation at the output of layers0.4
    lies in (-1e-6, -1e-7].  Moving every ReLU gate from 0 to -1e-6 (values change by at most 1e-6) moves the
    six NeRF gradients before that unit by 1.9e-3 .. 3.7e-3 in the Frobenius norm -- what the HIP step, which
    evaluates that unit above zero, showed against the unstaged oracle -- and every layer after it by far less;
    at -1e-7 nothing moves.  An f32 evaluation decides that unit by its rounding (the f32 oracle's own
    pre-activations are 2.5e-6 rms from fp64 here)."""
    import copy

    from torch import nn

    from tests import test_gpu_full_step_ndc as T

    class Gate(nn.Module):
        def __init__(self, tau):
            super().__init__()
            self.tau = tau

        def forward(self, x):
            return x * (x > self.tau).to(x.dtype)

    s = T._Setup(torch.device("cpu"), "pose")
    ray_idx, noise = next(T._draw())
    data = s.data(*T.STEPS[0])
    plain = s.ref
    _, _, g0 = s.oracle(data, ray_idx, noise, torch.float64)
    moved = {}
    for tau in (-1e-7, -1e-6):
        s.ref = copy.deepcopy(plain)
        for seq in (s.ref.layers0, s.ref.layers1, s.ref.rgb_layers):
            for i, m in enumerate(seq):
                if isinstance(m, nn.ReLU):
                    seq[i] = Gate(tau)
        _, _, g = s.oracle(data, ray_idx, noise, torch.float64)
        moved[tau] = {n: T._nrel(g[n], g0[n]) for n in g}
    s.ref = plain
    print({n: f"{v:.3e}" for n, v in moved[-1e-6].items()})
    assert max(moved[-1e-7].values()) == 0.0
    before = ("layers0.0.weight", "layers0.0.bias", "layers0.2.weight", "layers0.2.bias", "layers0.4.weight",
              "layers0.4.bias")
    want = (3.74e-3, 2.54e-3, 2.52e-3, 2.33e-3, 1.98e-3, 1.92e-3)
    for n, w in zip(before, want):
        assert abs(moved[-1e-6][n] - w) <= 0.02 * w, (n, moved[-1e-6][n], w)
    assert max(v for n, v in moved[-1e-6].items() if n not in before) < 5e-4
