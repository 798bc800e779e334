"""The fp64 references of the weight-gradient and head tests (tests/helpers.py) checked on the CPU:
wgrad_ref and heads_ref are the autograd of nn.Linear / of fc_density and fc_rgb behind a ReLU, the
fp16-pair emulation stays under wgrad_ceiling on every input kind and within one f32 ulp of the
condition sum on the tight kinds, the `exact` kind is exact, and every reference fails its own check
when broken through its _wrong switch."""
import pytest
import torch

from tests import helpers as H

NOUT, KIN, SPLITS = 64, 128, 3


def _linear_grads(dy, x):
    lin = torch.nn.Linear(x.shape[1], dy.shape[1]).double()
    (lin(x.double()) * dy.double()).sum().backward()
    return lin.weight.grad, lin.bias.grad


@pytest.mark.parametrize("kind", ["generic", "zeros", "outlier"])
def test_wgrad_ref_is_linear_autograd(kind):
    dy, x, _, _ = H.wgrad_inputs(kind, 384, NOUT, KIN, 5, SPLITS)
    gw, gb = _linear_grads(dy, x)
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()      # noqa: E731
    slab, bias, cond, bcond = H.wgrad_ref(dy, x, SPLITS)
    assert slab.shape == (SPLITS, NOUT, KIN) and bias.shape == (SPLITS, NOUT)
    assert rel(slab.sum(0), gw) < 1e-13 and rel(bias.sum(0), gb) < 1e-13
    assert bool((cond >= slab.abs()).all()) and bool((bcond >= bias.abs()).all())
    slab, bias, _, _ = H.wgrad_ref(dy, x, SPLITS, _wrong="row")          # one row left out of every split
    # (per element against the condition sum: the outlier kind hides it from a max-normalised error)
    assert H.cond_error(slab.sum(0), gw, cond.sum(0))[0] > 1e-4 and H.cond_error(bias.sum(0), gb, bcond.sum(0))[0] > 1e-4


def test_heads_ref_is_autograd():
    """fc_density on h8 and fc_rgb behind the colour layer's ReLU: raw4, dyr = dL/d(pre-activation), the
    head gradients.  The pre-activations hold exact zeros (dead columns, 0.0, -0.0): the gate is hr > 0."""
    inp = H.heads_inputs(128, 144, 3)
    pre = inp["hr"].double().clone()
    pre[pre == 0] = -1.0
    pre[:, 5] = inp["hr"][:, 5].double()                                  # 0.0, -0.0, 2^-149 stay
    pre.requires_grad_(True)
    fd, fr = torch.nn.Linear(128, 1).double(), torch.nn.Linear(64, 3).double()
    with torch.no_grad():
        fd.weight.copy_(inp["wd"]); fd.bias.copy_(inp["bd"]); fr.weight.copy_(inp["wc"]); fr.bias.copy_(inp["bc"])
    hr = torch.relu(pre)
    raw4 = torch.cat([fd(inp["h8"].double()), fr(hr)], 1)
    (raw4 * inp["graw4"].double()).sum().backward()
    r = H.heads_ref(inp["h8"], hr, inp["wd"], inp["bd"], inp["wc"], inp["bc"], inp["graw4"])
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()      # noqa: E731
    assert rel(r["raw4"], raw4.detach()) < 1e-13
    assert rel(r["dyr"], pre.grad) < 1e-13
    assert bool((r["dyr"][hr.detach() == 0] == 0).all()) and bool((r["dyr"][3::16, 5] != 0).any())    # a subnormal opens the gate
    assert rel(r["gwd"], fd.weight.grad[0]) < 1e-13 and rel(r["gbd"], fd.bias.grad) < 1e-13
    assert rel(r["gwc"], fr.weight.grad) < 1e-13 and rel(r["gbc"], fr.bias.grad) < 1e-13
    assert torch.equal(r["rmax"], r["dyr"].abs().amax(1)) and r["cmax"] is None
    w = H.heads_ref(inp["h8"], hr, inp["wd"], inp["bd"], inp["wc"], inp["bc"], inp["graw4"], _wrong="gate")
    assert rel(w["dyr"], pre.grad) > 1e-3                                # the gate read as >= 0
    # the ReLU words carry the same gate
    assert torch.equal(H.relu_bits(H.relu_words(r["gate"]), 64), r["gate"])


def _emulation_case(kind, rows, _wrong=None):
    """-> (under the ceiling everywhere, non-zero outputs at condition 0, max e of the emulation)."""
    m = rows * SPLITS
    dy, x, dcm, xcm = H.wgrad_inputs(kind, m, NOUT, KIN, 11, SPLITS)
    slab, _, cond, _ = H.wgrad_ref(dy, x, SPLITS)
    emu = H.wgrad_pair_emulate(dy, x, dcm, xcm, SPLITS, _wrong=_wrong)
    bd, bx = H.wgrad_bounds(dcm, SPLITS), H.wgrad_bounds(xcm, SPLITS)
    under, worst = True, 0.0
    for s in range(SPLITS):
        ceil = H.wgrad_ceiling(rows, cond[s], dy[s * rows:(s + 1) * rows], x[s * rows:(s + 1) * rows], bd[s], bx[s])
        err = (emu[s] - slab[s]).abs()
        under = under and bool(torch.isfinite(emu[s]).all()) and bool((err <= ceil).all())
        worst = max(worst, (err / ceil)[torch.isfinite(err)].max().item())
    e, nz = H.cond_error(emu, slab, cond)
    return under, nz, e, worst


@pytest.mark.parametrize("rows", [128, 384])
@pytest.mark.parametrize("kind", H.WGRAD_KINDS)
def test_emulation_under_the_ceiling(kind, rows):
    under, nz, e, worst = _emulation_case(kind, rows)
    print(f"{kind} K={rows}: emulation e {e / H.U24:.3f} ulp of the condition sum, {worst:.4f} of the ceiling")
    assert under and nz == 0
    if kind in H.WGRAD_TIGHT:
        assert e <= H.U24                  # the tight bar's headroom is the accumulator's rounding alone
    if kind == "exact":
        assert e == 0.0


def test_wrong_emulations_fail():
    under, nz, e, _ = _emulation_case("generic", 128, _wrong="drop")           # the lo.hi product dropped
    assert e > 16 * H.U24 and not under
    under, nz, e, _ = _emulation_case("outlier", 128, _wrong="split")          # a bound from the wrong split
    assert not under


def test_pair_exp_is_the_header_rule():
    b = torch.tensor([0.0, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 0.125, 0.99, 1.0, 2.0 ** 15, 3e38])
    e = H.pair_exp(b)
    assert e.tolist() == [0, 140, 140, 140, 17, 15, 14, -1, -113]
    s = b[3:].double() * 2.0 ** e[3:].double()
    assert bool((s >= 2.0 ** 14).all()) and bool((s < 2.0 ** 15).all())


def test_exact_kind_is_exact():
    """Every product and sum of the `exact` kind is exact in f32 and every operand in fp16: the slab is a
    known integer matrix, different at every (split, o, j) of a tile."""
    for m, nout, kin, splits in ((9216, 256, 256, 8), (96, 64, 64, 3)):
        dy, x, _, _ = H.wgrad_inputs("exact", m, nout, kin, 0, splits)
        slab, bias, cond, _ = H.wgrad_ref(dy, x, splits)
        assert torch.equal(x.half().float(), x) and torch.equal(dy.half().float(), dy)
        assert slab.abs().max().item() < 2 ** 24 and torch.equal(slab, cond) and torch.equal(slab, slab.round())
        r = m // splits
        f32 = torch.stack([dy[s * r:(s + 1) * r].t() @ x[s * r:(s + 1) * r] for s in range(splits)])
        assert torch.equal(f32.double(), slab)
        assert slab.sum(0).abs().max().item() < 2 ** 24
        # a transposed or permuted store cannot pass: neighbouring entries differ along j, and all but a few along o and the splits
        # (where a split has a row for the output at all: rows per split < nout leaves zero rows)
        live = bias > 0
        assert bool((slab[:, :, 1:] != slab[:, :, :-1])[live].all())
        assert (slab[:, 1:] != slab[:, :-1])[live[:, 1:] & live[:, :-1]].float().mean().item() > 0.99
        both = live[1:] & live[:-1]
        assert not bool(both.any()) or (slab[1:] != slab[:-1])[both].float().mean().item() > 0.99
        assert bool(live.any(1).all())
        if nout == kin:
            assert bool((slab != slab.transpose(1, 2)).any())


def test_input_kinds_hold_their_conditions():
    m, splits = 768, 3
    dy, x, dcm, xcm = H.wgrad_inputs("zeros", m, NOUT, KIN, 2, splits)
    assert not dy[:, 1].any() and not x[:, 2].any() and not dcm[:, 1].any() and not xcm[:, 2].any()
    assert not dy[256:512, 3].any() and dy[:256, 3].any() and not dy[512:].any() and not x[-5:].any()
    assert not dcm[0, 6].any() and dcm[1, 6] > 0
    dy, x, dcm, xcm = H.wgrad_inputs("edge", m, NOUT, KIN, 2, splits)
    assert torch.equal(dcm[:, :5], torch.tensor([2.0 ** -130, 0.125, 1.0, 2.0 ** 15, 3e38]).expand(6, 5))
    assert torch.equal(xcm[:, :4], torch.tensor([2.0 ** -130, 0.125, 1.0, 2.0 ** 15]).expand(6, 4))
    assert xcm[:, KIN // 2:].max().item() == 2.0 ** -100 and bool((xcm[:, KIN // 2] == 2.0 ** -100).all())
    assert x[dy[:, 4] != 0].abs().max().item() <= 2.0 ** -100
    slab, bias, _, _ = H.wgrad_ref(dy, x, splits)
    assert slab.abs().max().item() < 3e38 and bias.abs().max().item() < 3.4e38
    dy, x, dcm, xcm = H.wgrad_inputs("loose", m, NOUT, KIN, 2, splits)
    assert bool((xcm[:, :-1] == 1).all()) and not xcm[:, -1].any() and not x[:, -1].any()
    assert torch.equal(dcm, 8 * dy.abs().view(6, 128, NOUT).amax(1))
    tm = x.abs().amax(0)[:-1]
    assert 0.25 < tm.min().item() and tm.max().item() <= 1.0
    assert H.wgrad_inputs("generic", 96, NOUT, KIN, 2, 3)[2] is None       # no scales below a group
