"""The staged reference of the with_ssim reprojection term (tests/pair_ssim_ref.py) checked on the CPU:
the hand-walked window rule is the oracle's SSIM on the (1, h, w, 3) layout; a torch emulation of the
kernels' algorithm (saved f32 samples, fp64 windows, gather-form backward, N = 3 n_valid) passes the bars
of the GPU module; each of five wrong kernels fails them; the input sets of the GPU module hold their
conditions."""
import pytest
import torch

from oracle import nerf_oracle as orc
from tests import helpers as H
from tests import pair_ssim_ref as S


@pytest.mark.parametrize("h,w", [(1, 2), (2, 3), (3, 7)])
def test_window_rule_is_the_oracle_ssim(h, w):
    """Columns c-1 .. c+1 of the same row and colours k-1 .. k+1, reflected without repeating the edge
    (at w = 2 the window of column 0 is {1, 0, 1}), rows never mixing: walked tap by tap and as index
    tables, against orc.ssim_map on the (1, h, w, 3) tensors at fp64."""
    g = torch.Generator().manual_seed(10 * h + w)
    x, y = torch.rand(h, w, 3, generator=g, dtype=torch.float64), torch.rand(h, w, 3, generator=g, dtype=torch.float64)
    want = orc.ssim_map(x[None], y[None])[0]
    assert 0 < want.min().item() and want.max().item() < 1
    walked = S.ssim_map_walked(x, y)
    assert (walked - want).abs().max().item() <= 1e-14
    tables = S.ssim_moments(x.view(-1, 3), y.view(-1, 3), S.ssim_taps(h, w))["raw"].clamp(0, 1).view(h, w, 3)
    assert (tables - want).abs().max().item() <= 1e-14
    if h > 1:                                            # another row changes nothing in this one
        x2, y2 = x.clone(), y.clone()
        x2[1:], y2[1:] = 0.25, 0.75
        assert torch.equal(S.ssim_map_walked(x2, y2)[0], walked[0])
    col, wc, ct, wk = S.ssim_taps(h, w)
    assert col[0].tolist() == [1, 0, 1] and ct.tolist() == [[1, 0, 1], [0, 1, 2], [1, 2, 1]]
    assert col[w - 1].tolist() == [w - 2, w - 1, w - 2]


def test_emulated_term_is_the_oracle_term():
    """The emulation's forward and its gather-form backward against autograd of the oracle expression,
    fp64 samples, a mask with valid and invalid points side by side."""
    h, w = 3, 7
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, h, w, 3, generator=g, dtype=torch.float64)
    y = torch.rand(1, h, w, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    v = torch.rand(1, h, w, 1, generator=g) < 0.6
    want = orc.rgb_s_loss_ref(x, y, v, with_ssim=True)
    gw, = torch.autograd.grad(want, y)
    y2 = y.detach().clone().requires_grad_(True)
    got = S._EmuTerm.apply(x, y2, v, None)
    gg, = torch.autograd.grad(got, y2)
    assert abs(got.item() - want.item()) <= 1e-7         # the blend is summed in f32, as the kernel sums it
    assert (gg - gw).abs().max().item() <= 1e-13
    assert bool(((gw != 0).any(-1, keepdim=True) & ~v).any())      # an invalid point with a gradient


@pytest.mark.parametrize("h,w", [(3, 85), (2, 129), (19, 27)])
def test_emulation_passes_on_the_generic_sets(h, w):
    for cam in ("diag", "principal"):
        inp = S.ssim_inputs(h, w, cam)
        S.check_emulation(inp, S.emulate_ssim(inp))


WRONG = ["flat_index", "valid_only", "colour_clamped", "mask_on_inputs", "multiplicity_one"]


@pytest.mark.parametrize("wrong", WRONG)
def test_bars_reject_a_wrong_kernel(wrong):
    """The window over the flat index (crossing row ends), gradient to valid points only, the colour axis
    clamped instead of reflected, the mask on window inputs instead of outputs, reflection multiplicity 1:
    the unmodified emulation passes on the input set, the wrong one fails."""
    inp = S.ssim_inputs(3, 85, "diag")
    S.check_emulation(inp, S.emulate_ssim(inp))
    with pytest.raises(AssertionError):
        S.check_emulation(inp, S.emulate_ssim(inp, wrong))


def test_wrong_kernels_fail_on_their_own_bar():
    """valid_only changes nothing but g_d1 (and dR, dt) of invalid points: out3 still passes, the `rgbs`
    gradients do not."""
    inp = S.ssim_inputs(3, 85, "diag")
    got = S.emulate_ssim(inp, "valid_only")
    ref = S.PairSsimRef(inp)
    ref.check_out3(got["out3"], got["nn"])
    with pytest.raises(AssertionError, match="g_d1"):
        ref.check_grads(got["grads"]["rgbs", 0], got["nn"], "rgbs", 0)


def test_conditions_hold_on_every_input_set():
    """Every input set of tests/test_gpu_pair_ssim_fp64.py: the decisions' margins, the map inside (0, 1),
    an invalid point with a gradient (waived for the narrow frames), and the emulation within the bars on
    the crafted ones."""
    for h, w in ((3, 85), (2, 128), (2, 129), (19, 27), (3, 300)):
        for cam in ("diag", "principal"):
            assert S.PairSsimRef(S.ssim_inputs(h, w, cam)).n_invalid_grad > 0
    assert S.PairSsimRef(S.ssim_inputs(47, 155, "skew")).n_invalid_grad > 0
    for h, w in ((2, 2), (3, 2), (2, 3)):
        inp = S.narrow_inputs(h, w)
        ref = S.check_emulation(inp, S.emulate_ssim(inp), need_invalid_grad=False)
        assert bool(ref.dec["valid"].any())
    inp = H.pair_clamped_inputs()[0]
    ref = S.check_emulation(inp, S.emulate_ssim(inp))
    assert int((ref.dec["bad"] & S.row_near(ref.dec["valid"] & ~ref.dec["bad"], 19, 27)).sum()) > 0
    inp = H.pair_no_valid_inputs()
    S.check_emulation(inp, S.emulate_ssim(inp), need_valid=False, need_invalid_grad=False)
    inp = S.constant_inputs()
    ref = S.check_emulation(inp, S.emulate_ssim(inp), need_map=False, need_sign=False, need_invalid_grad=False)
    assert bool(ref.dec["valid"].all()) and ref.map64.abs().max().item() <= 1e-12
    assert 0.0 <= S.emulate_ssim(inp)["out3"][1].item() <= 1e-6
