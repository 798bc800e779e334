"""The host checks of the six chain entry points (chain.hip): every bad argument below is refused
with NERF_EINVAL and the entry's own message before anything is launched (GPU only: the operands
are device pointers, but no case reaches a kernel).

Each case starts from arguments the entry accepts (tests.helpers.chain_kernel_state, chain_descs,
chain_bwd_args, GEMM precision mode 2) and breaks one thing.  Two of the common cases have no
literal counterpart and use the nearest check of the entry:
  * nerf_render_eval_fused takes no n_pad (it derives it from n_rays x n_samples): its row-count
    cases are the sample count that does not tile the block and the sample total past 2^30;
  * nerf_chain_bwd has no bias: the backward entries' 16-byte case is the density head's weight
    (wd), their other LDS-DMA source next to the weight images.
nerf_render_eval_fused also refuses an output (rgb, dist, alpha, z) that is not 16-byte aligned."""
import re

import pytest
import torch

from model import _hip
from tests import helpers as H

pytestmark = pytest.mark.gpu

NP, R0, S0 = H.CHAIN_NP, H.CHAIN_R0, H.CHAIN_S0
FWD, TRAIN, FROZEN, EVAL = "nerf_mlp_chain_fwd", "nerf_mlp_chain_train", "nerf_mlp_chain_frozen", "nerf_render_eval_fused"
BWD, RAYS = "nerf_mlp_chain_bwd", "nerf_mlp_chain_bwd_rays"
LF, LR = 8, 9                      # the feature layer (no ReLU) and the colour layer


@pytest.fixture(scope="module")
def state(dev):
    old = _hip.gemm_get_precision()
    _hip.gemm_set_precision(2)
    try:
        k = H.chain_kernel_state(dev)
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)      # noqa: E731
        w = lambda i: 128 if i == 0 else 256                                  # noqa: E731
        k["graw4"] = torch.randn(NP, 4, generator=torch.Generator().manual_seed(9)).to(dev)
        k["dy"] = [e(NP, w(i)) for i in range(10)]
        k["cm"] = [e(NP // 128, w(i)) for i in range(10)]
        k["rm"] = [e(NP) for _ in range(10)]
        k["scratch"] = e(512)
        k["eval_out"] = (e(R0, 3), e(R0), e(R0, S0), e(NP))
        return k
    finally:
        _hip.gemm_set_precision(old)


def _forward(entry, k, edit):
    """The entry's call on valid arguments after edit(descs, kw) changed them."""
    runner, none = k["runner"], [None] * 10
    descs = {FWD: lambda: H.chain_descs(runner, k["outs"], none, none, plain=True),
             TRAIN: lambda: H.chain_descs(runner, k["outs"], k["masks"], k["cmaxes"]),
             FROZEN: lambda: H.chain_descs(runner, none, k["masks"], none),
             EVAL: lambda: H.chain_descs(runner, none, none, none)}[entry]()
    kw = dict(n_pad=NP, R=R0, S=S0)
    edit(descs, kw)
    enc = (k["enc_p"], k["enc_d"], k["rp"], k["rd"], kw["n_pad"], descs)
    if entry == FWD:
        _hip.mlp_chain_fwd(*enc)
    elif entry == TRAIN:
        _hip.mlp_chain_train(*enc, *k["heads"], k["raw4"])
    elif entry == FROZEN:
        _hip.mlp_chain_frozen(*enc, *k["heads"], k["raw4"])
    else:
        _hip.render_eval_fused(k["o"], k["d"], k["view"], kw["R"], kw["S"], 0.01, 10.0, 0, descs, *k["heads"],
                               *k["eval_out"])


def _backward(entry, k, edit):
    if entry == BWD:
        c = H.chain_bwd_args(k, k["graw4"], k["dy"], k["cm"], k["rm"], k["scratch"])
    else:
        keep = lambda ts: [t if i in (0, 5, 9) else None for i, t in enumerate(ts)]      # noqa: E731
        c = H.chain_bwd_args(k, k["graw4"], keep(k["dy"]), [None] * 10, keep(k["rm"]), None)
    edit(c, k)
    (_hip.mlp_chain_bwd if entry == BWD else _hip.mlp_chain_bwd_rays)(c)


def _set(l, **fields):
    def edit(descs, kw):
        for name, v in fields.items():
            setattr(descs[l], name, v)
    return edit


def _kw(**values):
    return lambda descs, kw: kw.update(values)


def _bias_off4(l):
    def edit(descs, kw):
        descs[l].bias += 4          # the address of a [1:] view of the float32 bias
    return edit


def _out_of(l):
    def edit(descs, kw):
        descs[l].out = descs[l].img     # any non-NULL pointer: it is never written
    return edit


def _bwd_field(name, i, value):
    def edit(c, k):
        getattr(c, name)[i] = value
    return edit


def _bwd_n_pad(c, k):
    c.n_pad = 200


def _bwd_wd_off4(c, k):
    c.wd = k["runner"].wd.view(-1)[1:].data_ptr()


def _bwd_cmax0(c, k):
    c.dy_cmax[0] = k["cm"][0].data_ptr()


ROWS_NE = "chain image rows 128 != 256"
FORWARD_CASES = [
    # (entry, edit, a fragment of the message)
    (FWD, _kw(n_pad=200), "n_pad=200 must be a positive multiple of 128"),
    (FWD, _bias_off4(2), "layer 2: bias not 16-byte aligned (16-byte LDS-DMA)"),
    (FWD, _set(1, img_rows=128), "layer 1: image rows 128 < 256 or image not 16-byte aligned"),
    (TRAIN, _kw(n_pad=200), "n_pad=200 must be a positive multiple of 128"),
    (TRAIN, _bias_off4(2), "layer 2: image / bias not 16-byte aligned or chain image rows 256 != 256"),
    (TRAIN, _set(1, img_rows=128), "layer 1: image / bias not 16-byte aligned or " + ROWS_NE),
    (TRAIN, _set(3, mask=None), "layer 3: the ReLU words are mandatory (ldmask 8, even, 8-byte aligned)"),
    (TRAIN, lambda d, kw: setattr(d[LR], "cmax", d[0].cmax),
     "layer 9: column maxima are mandatory for l0..lf and absent for the colour layer"),
    (TRAIN, _set(5, out=None), "layer 5: the training chain saves every layer output (ldo 256"),
    (FROZEN, _kw(n_pad=200), "n_pad=200 must be a positive multiple of 128"),
    (FROZEN, _bias_off4(2), "layer 2: image / bias not 16-byte aligned or chain image rows 256 != 256"),
    (FROZEN, _set(1, img_rows=128), "layer 1: image / bias not 16-byte aligned or " + ROWS_NE),
    (FROZEN, lambda d, kw: setattr(d[LF], "mask", d[0].mask), "the feature layer has no ReLU"),
    (EVAL, _kw(S=96), "n_rays=12, n_samples=96: the samples of a ray must tile the 128-row block"),
    (EVAL, _kw(R=1 << 25, S=64), "too many samples"),
    (EVAL, _bias_off4(2), "layer 2: image / bias not 16-byte aligned or chain image rows 256 != 256"),
    (EVAL, _set(1, img_rows=128), "layer 1: image / bias not 16-byte aligned or " + ROWS_NE),
    (EVAL, _out_of(4), "layer 4: the eval render saves no activations, masks or column maxima"),
]
BACKWARD_CASES = [
    (BWD, _bwd_n_pad, "n_pad=200 must be a positive multiple of 128"),
    (BWD, _bwd_wd_off4, "pointer 'p.wd' not 16-byte aligned"),
    (BWD, _bwd_field("wt_img_rows", 0, 256), "layer 0: weight-transpose chain image missing, unaligned or not 320 rows"),
    (BWD, _bwd_field("wt_img", 3, None), "layer 3: weight-transpose chain image missing, unaligned or not 256 rows"),
    (BWD, _bwd_field("ld_in_mask", 2, 4), "layer 2: the input's ReLU words (ld >= 8, 16-byte rows) are required"),
    (BWD, _bwd_field("dy_rmax", 4, None), "D_4: output, column maxima and row maxima are mandatory (ld == 256"),
    (RAYS, _bwd_n_pad, "n_pad=200 must be a positive multiple of 128"),
    (RAYS, _bwd_wd_off4, "pointer 'p.wd' not 16-byte aligned"),
    (RAYS, _bwd_field("wt_img_rows", 0, 256), "layer 0: weight-transpose chain image missing, unaligned or not 320 rows"),
    (RAYS, _bwd_cmax0, "D_0: output and row maxima are mandatory (ld == 128, 16-byte aligned), column maxima are not "
                       "written (dy_cmax must be NULL)"),
]


def _ids(cases):
    return [f"{entry[5:]}-{i}" for i, (entry, _, _) in enumerate(cases)]


def _refused(entry, fragment, call):
    # -1 is NERF_EINVAL, the return of a host check; a launch reports NERF_ELAUNCH (-2) or nothing
    with pytest.raises(RuntimeError, match=re.escape(f"{entry} failed (-1): {entry}: ") + ".*" + re.escape(fragment)):
        call()


@pytest.fixture
def h16(dev):
    old = _hip.gemm_get_precision()
    _hip.gemm_set_precision(2)
    yield
    _hip.gemm_set_precision(old)


def test_valid_arguments_are_what_the_cases_start_from(state, h16):
    """The unedited calls are accepted (so each case below is refused for its one defect)."""
    for entry in (FWD, TRAIN, FROZEN, EVAL):
        _forward(entry, state, lambda descs, kw: None)
    for entry in (BWD, RAYS):
        _backward(entry, state, lambda c, k: None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("entry,edit,fragment", FORWARD_CASES, ids=_ids(FORWARD_CASES))
def test_forward_entry_refuses(state, h16, entry, edit, fragment):
    _refused(entry, fragment, lambda: _forward(entry, state, edit))


@pytest.mark.parametrize("which", ["rgb", "dist", "alpha", "z"])
def test_eval_entry_refuses_a_misaligned_output(state, h16, dev, which):
    """The header's pointer contract (16-byte aligned; alpha is stored as float4 for S >= 64): an
    output 4 bytes off is refused on the host, nothing launches, the guarded outputs stay untouched."""
    k = state
    shapes = dict(rgb=(R0, 3), dist=(R0,), alpha=(R0, S0), z=(NP,))
    G = {n: H.Guarded(s, dev) for n, s in shapes.items()}
    outs = {n: g.t for n, g in G.items()}
    g = G[which]
    outs[which] = g.buf[H.GUARD + 1:H.GUARD + 1 + g.t.numel()]
    assert outs[which].data_ptr() % 16 == 4
    descs = H.chain_descs(k["runner"], [None] * 10, [None] * 10, [None] * 10)
    _refused(EVAL, f"pointer '{which}' not 16-byte aligned",
             lambda: _hip.render_eval_fused(k["o"], k["d"], k["view"], R0, S0, 0.01, 10.0, 0, descs, *k["heads"],
                                            outs["rgb"], outs["dist"], outs["alpha"], outs["z"]))
    torch.cuda.synchronize()
    for n, gd in G.items():
        assert gd.untouched(), n


@pytest.mark.parametrize("entry,edit,fragment", BACKWARD_CASES, ids=_ids(BACKWARD_CASES))
def test_backward_entry_refuses(state, h16, entry, edit, fragment):
    _refused(entry, fragment, lambda: _backward(entry, state, edit))
