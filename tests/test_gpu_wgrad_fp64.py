"""The weight-gradient GEMMs (wgrad.hip, the TN kernels of gemm_x6.hip and gemm_f32.hip) and
nerf_slab_reduce against fp64, per split and per element (GPU only).

Every call writes into sentinel-guarded slabs [splits][nout][ldslab] with ldslab > col0 + kin, and is held to
  * wgrad_ceiling per slab element and wgrad_bias_ceiling per bias partial (tests/helpers.py: derived from
    the arithmetic, with the bounds the call was given in place of the column maxima);
  * exactly 0, no NaN, where the condition sum is 0;
  * the sentinel in every slab column outside [col0, col0 + kin), in every guard, and in bslab when NULL
    was passed;
  * torch.equal on the `exact` kind (an integer slab that differs at every (split, o, j));
  * the launch count and the arithmetic of nerf_prof_read_kinds (1 product: exact f32, 3: the fp16 pair,
    6: bf16x3) -- which path ran is asserted, not assumed;
  * on the four tight kinds, max e (|got - ref| / condition sum) of modes 1 and 2 <= 1.5 x max e of the
    exact-f32 kernel on the same operands and splits + 4 ulp (tight_bar), per element and split.
The shapes are the smallest that reach each instantiation of pick_tn_x6, nerf_linear_bwd_weight's mode-0
dispatch and launch_wgrad; the input kinds are wgrad_inputs' (DESIGN.md section 4.9)."""
import functools
import types

import pytest
import torch

from model import _hip
from tests import helpers as H

pytestmark = pytest.mark.gpu
SENT = H.SENT
PRODUCTS = {0: 1, 1: 6, 2: 3}


def _seed(kind, rows, splits, nout, kin):
    return H.WGRAD_KINDS.index(kind) * 100003 + rows * 17 + splits * 5 + nout + 3 * kin


def _make_ref(dy, x, dcm, xcm, splits):
    """The fp64 slabs of given operands with their ceilings (plain: no scales; pair: the bounds' floor)."""
    m = dy.shape[0]
    rows = m // splits
    slab, bias, cond, bcond = H.wgrad_ref(dy, x, splits)
    R = types.SimpleNamespace(dy=dy, x=x, dcm=dcm, xcm=xcm, splits=splits, rows=rows, m=m, nout=dy.shape[1],
                              kin=x.shape[1], slab=slab, bias=bias, cond=cond, bcond=bcond)
    R.ceil_plain = torch.stack([H.wgrad_ceiling(rows, cond[s], None, None) for s in range(splits)])
    R.ceil_pair = None
    if dcm is not None and rows % 128 == 0:
        bd, bx = H.wgrad_bounds(dcm, splits), H.wgrad_bounds(xcm, splits)
        R.ceil_pair = torch.stack([H.wgrad_ceiling(rows, cond[s], dy[s * rows:(s + 1) * rows], x[s * rows:(s + 1) * rows],
                                                   bd[s], bx[s]) for s in range(splits)])
    R.bceil = H.wgrad_bias_ceiling(rows, bcond)
    return R


@functools.lru_cache(maxsize=16)
def _ref(kind, rows, splits, nout, kin):
    R = _make_ref(*H.wgrad_inputs(kind, rows * splits, nout, kin, _seed(kind, rows, splits, nout, kin), splits), splits)
    R.kind = kind
    return R


def _pair_runs(mode, R, cmax=True):
    """nerf_linear_bwd_weight's rule: mode 2 runs the fp16 pair given both bounds and splits of whole groups."""
    return mode == 2 and cmax and R.dcm is not None and R.rows % 128 == 0


def _wide(t, dev, pad):
    """t as a column-offset view (16-byte aligned offset, ld > columns) of a NaN-filled device buffer."""
    if not pad:
        return t.to(dev)
    buf = torch.full((t.shape[0], t.shape[1] + 2 * pad), float("nan"), device=dev)
    v = buf[:, pad:pad + t.shape[1]]
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and v.stride(0) > t.shape[1]
    return v


class _Out:
    """Guarded slab [splits][nout][col0 + kin_total + 64] and bias partials [splits][nout]."""

    def __init__(self, dev, splits, nout, width, col0=0):
        self.ld = col0 + width + 64
        self.slab = H.Guarded((splits, nout, self.ld), dev)
        self.bslab = H.Guarded((splits, nout), dev)
        self.col0, self.width = col0, width

    def flat(self):
        return self.slab.t.view(-1)

    def read(self, what, bias=True):
        """The written columns as fp64; the rest must still hold the sentinel."""
        t = self.slab.t
        assert self.slab.intact() and self.bslab.intact(), f"{what}: a guard was written"
        assert bool((t[:, :, :self.col0] == SENT).all()) and bool((t[:, :, self.col0 + self.width:] == SENT).all()), \
            f"{what}: slab columns outside [col0, col0 + kin) written"
        if not bias:
            assert self.bslab.untouched(), f"{what}: bslab written though NULL was passed"
        return H._f64(t[:, :, self.col0:self.col0 + self.width]), (H._f64(self.bslab.t) if bias else None)


def _profiled(fn):
    """-> (launches, products of the launches) of the weight-gradient family around fn()."""
    _hip.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        k = _hip.prof_read_kinds()
    finally:
        _hip.prof_enable(False)
    n = k["dw"]["launches"] + k["dw_narrow"]["launches"]
    fl = k["dw"]["flops"] + k["dw_narrow"]["flops"]
    assert sum(v["launches"] for v in k.values()) == n
    ratio = (k["dw"]["mfma_flops"] + k["dw_narrow"]["mfma_flops"]) / fl if fl else 0.0
    return n, (round(ratio) if abs(ratio - round(ratio)) < 1e-9 else ratio)


def _hold(what, R, got, gotb, pair, fails):
    """The common checks of one call's slab (and bias partials) against R -> max e over the slab."""
    ceil = R.ceil_pair if pair else R.ceil_plain
    if not bool(torch.isfinite(got).all()):
        fails.append(f"{what}: non-finite slab")
        return float("inf")
    err = (got - R.slab).abs()
    e, nz = H.cond_error(got, R.slab, R.cond)
    worst = (err / ceil).max().item()
    H.report_err("wgrad_fp64", f"{what} ceiling ratio", worst)
    if worst > 1.0:
        i = int((err / ceil).argmax())
        fails.append(f"{what}: slab element {i} is {worst:.3g} of its ceiling (e {e / H.U24:.2f} ulp)")
    if nz:
        fails.append(f"{what}: {nz} non-zero outputs where the condition sum is 0")
    if gotb is not None:
        berr = (gotb - R.bias).abs()
        if not bool(torch.isfinite(gotb).all()) or bool((berr > R.bceil).any()):
            fails.append(f"{what}: bias partial {(berr / R.bceil).max().item():.3g} of its ceiling")
        if bool((gotb[R.bcond == 0] != 0).any()):
            fails.append(f"{what}: non-zero bias partial where sum |dy| is 0")
    if getattr(R, "kind", None) == "exact":
        if not torch.equal(got, R.slab) or (gotb is not None and not torch.equal(gotb, R.bias)):
            fails.append(f"{what}: the exact kind is not exact")
    return e


def _single(dev, R, mode, cmax=True, col0=0, pad=0, bias=True, what=""):
    """One nerf_linear_bwd_weight call under precision `mode` -> (slab, bias partials) as fp64."""
    _hip.gemm_set_precision(mode)
    out = _Out(dev, R.splits, R.nout, R.kin, col0)
    dy, x = _wide(R.dy, dev, pad), _wide(R.x, dev, pad)
    dcm = R.dcm.to(dev) if cmax and R.dcm is not None else None
    xcm = R.xcm.to(dev) if cmax and R.xcm is not None else None
    n, prod = _profiled(lambda: _hip.linear_bwd_weight(dy, R.nout, x, R.kin, R.m, R.splits, out.flat(), out.ld, col0,
                                                       out.bslab.t.view(-1) if bias else None, dy_cmax=dcm, x_cmax=xcm))
    want = 3 if _pair_runs(mode, R, cmax) else PRODUCTS[mode] if mode < 2 else 6
    assert (n, prod) == (1, want), f"{what}: {n} launches of {prod} products, expected 1 of {want}"
    return out.read(what, bias)


MODES = ((0, True, "f32"), (1, True, "bf16x3"), (2, True, "pair"), (2, False, "pair-nocmax"))


def _case(dev, policy, nout, kin, rows, splits, kinds=H.WGRAD_KINDS, modes=MODES, bf16_edge=False, collect=None, **kw):
    """Every kind under every mode at one shape; the tight bar against the same call in mode 0.  The `edge` kind
    on the bf16x3 arithmetic (mode 1, and mode 2 without bounds or whole groups) is test_bf16x3_edge_kind's:
    bf16_edge selects exactly those calls, otherwise they are left to it.  collect: a list that takes the
    failures instead of the assertion."""
    _hip.gemm_set_policy(0, policy)
    fails = [] if collect is None else collect
    for kind in kinds:
        R = _ref(kind, rows, splits, nout, kin)
        e = {}
        for mode, cmax, name in modes:
            if bf16_edge != (kind == "edge" and mode > 0 and not _pair_runs(mode, R, cmax)):
                continue
            what = f"tn{policy} {nout}x{kin} rows {rows} x {splits} {kind} {name}"
            got, gotb = _single(dev, R, mode, cmax=cmax, what=what, **kw)
            e[name] = _hold(what, R, got, gotb, _pair_runs(mode, R, cmax), fails)
            H.report_err("wgrad_fp64", f"{what} e", e[name])
        if kind in H.WGRAD_TIGHT and "f32" in e:
            for name, v in e.items():
                H.report_err("wgrad_fp64", f"tn{policy} {nout}x{kin} rows {rows} x {splits} {kind} {name} tight ratio",
                             v / H.tight_bar(e["f32"]))
                if v > H.tight_bar(e["f32"]):
                    fails.append(f"tn{policy} {nout}x{kin} rows {rows} x {splits} {kind} {name}: e {v / H.U24:.2f} ulp over "
                                 f"the tight bar (f32 {e['f32'] / H.U24:.2f} ulp)")
    assert collect is not None or not fails, "\n".join(fails)


def _tight_against_f32(dev, what, R, e, kinds, fails):
    """The tight bar for a fused entry point: its max e on R against one exact-f32 nerf_linear_bwd_weight call
    (mode 0) on the same operands and splits, where every kind that went into R is a tight one.  Leaves the
    precision at mode 2."""
    if not all(k in H.WGRAD_TIGHT for k in kinds):
        return
    got, _ = _single(dev, R, 0, what=what + " (mode-0 reference)")
    e0, _ = H.cond_error(got, R.slab, R.cond)
    _hip.gemm_set_precision(2)
    H.report_err("wgrad_fp64", f"{what} tight ratio", e / H.tight_bar(e0))
    if e > H.tight_bar(e0):
        fails.append(f"{what}: e {e / H.U24:.2f} ulp over the tight bar (f32 {e0 / H.U24:.2f} ulp)")


# rows per split x splits: the full cross product of the issue
ROWS_SPLITS = tuple((rows, splits) for rows in (32, 64, 96, 128, 256, 384, 1152) for splits in (1, 2, 3, 8))
# policy 3: (nout, kin) -> the tiles of mode 0 / of the split modes
#   64x64 -> 64x64; 64x128 -> 64x128; 128x64 -> 128x64; 128x128 -> 128x128; 256x128 -> 128x128 at o0 = 128;
#   128x256 -> 128x128, second column tile; 256x64 -> 128x64 (mode 0), 256x64 / 4 waves (split modes);
#   256x256 -> 256x256
SHAPES_3 = ((64, 64), (64, 128), (128, 64), (128, 128), (256, 128), (128, 256), (256, 64), (256, 256))


@pytest.mark.parametrize("rows,splits", ROWS_SPLITS)
@pytest.mark.parametrize("nout,kin", SHAPES_3)
def test_single_call_policy3(dev, nout, kin, rows, splits):
    _case(dev, 3, nout, kin, rows, splits)


@pytest.mark.parametrize("nout,kin,rows,splits", [(512, 256, 128, 8), (512, 256, 96, 3), (256, 512, 128, 8),
                                                  (256, 512, 96, 3), (512, 256, 1152, 2), (256, 512, 1152, 2)])
def test_second_row_and_column_tile_policy3(dev, nout, kin, rows, splits):
    """The 256 x 256 tiles with blockIdx.x > 0 (nout 512) and with a second column tile (kin 512)."""
    _case(dev, 3, nout, kin, rows, splits, kinds=("spread", "zeros", "exact"))


# policy 7: the shapes whose split-mode kernel differs from policy 3's (mode 0 is the same launch):
# 256x256 at splits % 8 == 0 -> XCD-paired 256x128 / 8 waves (other split counts: policy 3's tile),
# 128x256 -> 128x256 / 8 waves, 256x64 -> 256x64 / 8 waves
POLICY7 = [(nout, kin, rows, splits) for nout, kin in ((256, 256), (128, 256), (256, 64)) for rows, splits in ROWS_SPLITS
           if (nout, kin) != (256, 256) or splits % 8 == 0]


@pytest.mark.parametrize("nout,kin,rows,splits", POLICY7)
def test_single_call_policy7(dev, nout, kin, rows, splits):
    _case(dev, 7, nout, kin, rows, splits)


@pytest.mark.parametrize("policy,nout,kin", [(3, nout, kin) for nout, kin in SHAPES_3] +
                         [(7, 256, 256), (7, 128, 256), (7, 256, 64)])
def test_bf16x3_edge_kind(dev, policy, nout, kin):
    """The `edge` kind on the bf16x3 kernels (mode 1, and mode 2 without bounds or whole groups) at every rows x
    splits of the single-call tests, held to the first term of wgrad_ceiling alone, as the exact-f32 kernel is:
    the column scales of the bf16x3 TN kernels (gemm_x6.hip tn_col_exp3), from the caller's bounds where m is
    whole groups and from the block's own scan otherwise."""
    fails = []
    for rows, splits in ROWS_SPLITS:
        if policy == 3 or (nout, kin) != (256, 256) or splits % 8 == 0:
            _case(dev, policy, nout, kin, rows, splits, kinds=("edge",), modes=MODES[1:], bf16_edge=True, collect=fails)
    assert not fails, "\n".join(fails)


# policy 8: the 4-wave kernels of wgrad.hip take mode 2 with bounds at rows >= 96 (here: whole groups)
@pytest.mark.parametrize("rows", [128, 256, 384, 1152])
@pytest.mark.parametrize("splits", [8, 16])
@pytest.mark.parametrize("nout,kin", [(256, 256), (256, 64), (128, 256), (128, 64)])
def test_single_call_policy8_4wave(dev, nout, kin, rows, splits):
    _case(dev, 8, nout, kin, rows, splits, modes=MODES[:1] + MODES[2:3])


@pytest.mark.parametrize("policy,nout,kin", [(3, 64, 64), (3, 64, 128), (3, 128, 64), (3, 128, 128), (3, 256, 64),
                                             (3, 256, 256), (7, 256, 256), (7, 128, 256), (7, 256, 64), (8, 256, 256),
                                             (8, 256, 64), (8, 128, 256), (8, 128, 64)])
def test_leading_dimensions_and_col0(dev, policy, nout, kin):
    """dy and x as column-offset views of wider NaN-filled buffers, the slab columns from col0 = 64, with and
    without bias partials: one case per tile family."""
    for bias in (True, False):
        _case(dev, policy, nout, kin, 256, 8, kinds=("spread", "exact"), col0=64, pad=4, bias=bias)


def _kinds(i):
    return H.WGRAD_KINDS[i % len(H.WGRAD_KINDS)]


def _hold_reduced(what, dev, out, R, fails, pair):
    """nerf_slab_reduce of a checked slab: the sum of the splits' ceilings + (splits + 2) 2^-24 sum |slab|."""
    gw, gb = H.Guarded((R.nout, R.kin), dev), H.Guarded((R.nout,), dev)
    _hip.slab_reduce(out.flat(), R.splits, R.nout, out.ld, R.nout, R.kin, out.bslab.t.view(-1), gw.t, gb.t)
    torch.cuda.synchronize()
    assert gw.intact() and gb.intact()
    ceil = H.wgrad_reduced_ceiling(R.ceil_pair if pair else R.ceil_plain, R.slab.abs().sum(0), R.splits)
    err = (H._f64(gw.t) - R.slab.sum(0)).abs()
    if bool((err > ceil).any()) or not bool(torch.isfinite(H._f64(gw.t)).all()):
        fails.append(f"{what}: reduced gradient {(err / ceil).max().item():.3g} of its ceiling")
    berr = (H._f64(gb.t) - R.bias.sum(0)).abs()
    if bool((berr > R.bceil.sum(0) + H.slab_reduce_bar(R.splits, R.bias.abs().sum(0))).any()):
        fails.append(f"{what}: reduced bias gradient over its ceiling")


@pytest.mark.parametrize("policy", [7, 8])
@pytest.mark.parametrize("nout,m,splits", [(256, 1024, 8), (128, 1024, 8), (256, 3072, 8), (128, 3072, 8), (256, 1024, 4),
                                           (128, 1024, 4)])
def test_seg_against_fp64(dev, policy, nout, m, splits):
    """nerf_linear_bwd_weight_seg: one launch at splits % 8 == 0 in mode 2, two otherwise; the two segments
    draw different kinds.  Where both are tight kinds the slab is also held to the tight bar against one exact-f32
    call over the 320 columns."""
    _hip.gemm_set_policy(0, policy)
    fails = []
    rows = m // splits
    # (the edge kind's 3e38 rows need its own x: another kind's x there would leave f32's range)
    for ka, kb in [(k, "edge" if k == "edge" else _kinds(i + 3)) for i, k in enumerate(H.WGRAD_KINDS)] + [("exact", "exact")]:
        A, B = _ref(ka, rows, splits, nout, 256), _ref(kb, rows, splits, nout, 64)
        R = _make_ref(A.dy, torch.cat([A.x, B.x], 1), A.dcm, torch.cat([A.xcm, B.xcm], 1), splits)
        R.kind = "exact" if ka == kb == "exact" else None
        for mode in (0, 2):
            _hip.gemm_set_precision(mode)
            out = _Out(dev, splits, nout, 320)
            t = [v.to(dev) for v in (A.dy, A.x, B.x, A.dcm, A.xcm, B.xcm)]
            n, prod = _profiled(lambda: _hip.linear_bwd_weight_seg(t[0], nout, t[1], 256, t[2], 64, m, splits, out.flat(),
                                                                   out.ld, out.bslab.t.view(-1), dy_cmax=t[3],
                                                                   x1_cmax=t[4], x2_cmax=t[5]))
            what = f"seg tn{policy} {nout} m {m} x {splits} {ka}|{kb} mode {mode}"
            assert (n, prod) == ((1, 3) if mode == 2 and splits % 8 == 0 else (2, PRODUCTS[mode])), (what, n, prod)
            got, gotb = out.read(what)
            e = _hold(what, R, got, gotb, mode == 2, fails)
            if mode == 2:
                _hold_reduced(what, dev, out, R, fails, True)
                _tight_against_f32(dev, what, R, e, (ka, kb), fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("policy", [7, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_multi_against_fp64(dev, n, policy):
    """nerf_linear_bwd_weight_multi at m = 1024, splits 8: one launch under policy 8 (k_wgrad_pairs), n under
    policy 7; each layer draws another kind, so consecutive layers' exponent sets differ.  Layers of a tight kind
    are also held to the tight bar against their exact-f32 call.  nerf_wgrad_job's binding fixes ldslab = 256 = kin,
    so these slabs have no column outside [0, kin): here only the 64-element guards around each slab and its bias
    partials can show a stray store."""
    _hip.gemm_set_policy(0, policy)
    _hip.gemm_set_precision(2)
    m, splits = 1024, 8
    Rs = [_ref(_kinds(2 * i + 1), m // splits, splits, 256, 256) for i in range(n)]
    outs = [_Out(dev, splits, 256, 256, 0) for _ in Rs]
    for o in outs:
        o.ld = 256
        o.slab = H.Guarded((splits, 256, 256), dev)          # (nerf_wgrad_job: the binding passes ldslab 256)
    layers = [(R.dy.to(dev), R.x.to(dev), o.flat(), o.bslab.t.view(-1), R.dcm.to(dev), R.xcm.to(dev)) for R, o in zip(Rs, outs)]
    launches, prod = _profiled(lambda: _hip.linear_bwd_weight_multi(layers, m, splits))
    assert (launches, prod) == (1 if policy == 8 else n, 3)
    fails = []
    for i, (R, o) in enumerate(zip(Rs, outs)):
        what = f"multi tn{policy} n {n} layer {i} {R.kind}"
        got, gotb = o.read(what)
        e = _hold(what, R, got, gotb, True, fails)
        _tight_against_f32(dev, what, R, e, (R.kind,), fails)
    assert not fails, "\n".join(fails)


# job lists: (nout, kin, split factor, second 64-wide segment) per layer; the shape set k_wgrad_jobs compiles
JOB_LISTS = {
    "colour+trunk": [(128, 256, 2, True)] + [(256, 256, 1, False)] * 4,                           # set 3
    "l4+trunk+l0": [(256, 256, 1, True)] + [(256, 256, 1, False)] * 3 + [(256, 64, 2, False)],    # set 6
    "set0": [(256, 256, 1, False)] * 2,
    "set1": [(128, 256, 2, False), (256, 256, 1, False)],
    "set2": [(256, 256, 1, True)],
    "set4": [(256, 256, 1, False), (256, 64, 2, False)],
    "set5": [(128, 256, 2, False), (256, 64, 2, False), (256, 256, 1, False)],
}


def _jobs_case(dev, which, m, S, groups=None, shift=0):
    """Job i draws kind 3 i + 1 + shift, its second segment the next one (the `exact` and `edge` kinds: their own,
    so that the exact slab stays exact and no sum leaves f32's range)."""
    _hip.gemm_set_policy(0, 8)
    _hip.gemm_set_precision(2)
    jobs, checks = [], []
    flops = mfma = 0.0
    for i, (nout, kin, f, seg) in enumerate(JOB_LISTS[which]):
        sp = f * S
        rows = m // sp
        ka = _kinds(3 * i + 1 + shift)
        kb = _kinds(3 * i + 2 + shift)
        kb = ka if ka in ("exact", "edge") else ("generic" if kb == "edge" else kb)
        A = _ref(ka, rows, sp, nout, kin)
        B = _ref(kb, rows, sp, nout, 64) if seg else None
        out = _Out(dev, sp, nout, kin + (64 if seg else 0))
        dy, dcm = A.dy.to(dev), (A.dcm.to(dev) if A.dcm is not None else None)
        jobs.append((dy, nout, A.x.to(dev), kin, sp, out.flat(), out.ld, 0, out.bslab.t.view(-1), dcm,
                     A.xcm.to(dev) if A.xcm is not None else None))
        R = A
        if seg:
            jobs.append((dy, nout, B.x.to(dev), 64, sp, out.flat(), out.ld, kin, None, dcm,
                         B.xcm.to(dev) if B.xcm is not None else None))
            R = _make_ref(A.dy, torch.cat([A.x, B.x], 1), A.dcm, None if A.dcm is None else torch.cat([A.xcm, B.xcm], 1), sp)
            R.kind = "exact" if ka == kb == "exact" else None
        pair = rows % 128 == 0
        flops += m * nout * R.kin
        mfma += m * nout * R.kin * (3 if pair else 6)
        checks.append((f"jobs {which} m {m} job {i} {nout}x{kin} x {sp} {ka}" + (f"|{kb}" if seg else ""), R, out, pair,
                       (ka, kb) if seg else (ka,)))
    fused = all((m // j[4]) % 128 == 0 for j in jobs)
    n, prod = _profiled(lambda: _hip.linear_bwd_weight_jobs(jobs, m, S, groups=groups))
    # one launch of the fp16 pair, or the per-job calls, each on the arithmetic its rows per split select
    assert n == (1 if fused else len(jobs)) and abs(prod - mfma / flops) < 1e-6, (which, m, n, prod, mfma / flops)
    fails = []
    for what, R, out, pair, kinds in checks:
        got, gotb = out.read(what)
        e = _hold(what, R, got, gotb, pair, fails)
        _tight_against_f32(dev, what, R, e, kinds, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("m", [2048, 9216])
@pytest.mark.parametrize("which", list(JOB_LISTS))
def test_jobs_against_fp64(dev, which, m):
    """nerf_linear_bwd_weight_jobs at S = 8: m = 2048 gives the 2 S jobs 128 rows per split (the edge of
    k_wgrad_jobs<3>'s four stages in flight) and the S jobs 256; at m = 9216 the 2 S jobs' 576 rows are no
    whole groups, so a list with one runs as its per-job calls."""
    _jobs_case(dev, which, m, 8)


@pytest.mark.parametrize("which", ["colour+trunk", "l4+trunk+l0", "set2"])
def test_jobs_exact_on_the_segment_jobs(dev, which):
    """The kinds shifted so that the job with a second segment (two tile jobs into one slab) draws `exact`."""
    _jobs_case(dev, which, 2048, 8, shift=5)


def test_job_groups_against_fp64(dev):
    _jobs_case(dev, "l4+trunk+l0", 2048, 8, groups=[0, 0, 0, 1, 1, 1])


# ---- nerf_slab_reduce ---------------------------------------------------------------------------------
REDUCE_SPLITS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193, 256)
REDUCE_SHAPES = ((64, 136, 64, 130), (256, 320, 256, 283), (128, 320, 128, 155), (1, 256, 1, 256), (3, 128, 3, 128),
                 (64, 67, 60, 63))


@pytest.mark.parametrize("splits", REDUCE_SPLITS)
@pytest.mark.parametrize("nout,ld,nout_ref,kin_ref", REDUCE_SHAPES)
def test_slab_reduce_against_fp64(dev, nout, ld, nout_ref, kin_ref, splits):
    """Every load arm of slab_reduce_block (8 deep, 4 deep, the tail; 193 splits run all three), the scalar
    path of an unaligned row stride and of a 1-wide bias, accumulate 0 and 1, bslab or gb absent in turn:
    (splits + 2) 2^-24 sum |slab| per element, gw and gb in guarded buffers of exactly the reference size."""
    g = torch.Generator().manual_seed(splits * 1009 + nout * 7 + ld)
    slab = (torch.rand(splits, nout, ld, generator=g) * 2 - 1) * 2.0 ** torch.randint(-20, 21, (1, nout, ld), generator=g).float()
    bslab = torch.rand(splits, nout, generator=g) * 2 - 1
    slab[:, :, 1] = 0                                               # a dead column: exactly 0 out
    slab_d, bslab_d = slab.to(dev), bslab.to(dev)
    gw0 = torch.rand(nout_ref, kin_ref, generator=g) * 2 - 1
    gb0 = torch.rand(nout_ref, generator=g) * 2 - 1
    fails = []
    for acc in (False, True):
        for with_b, with_gb in ((True, True), (False, True), (True, False)):
            gw, gb = H.Guarded((nout_ref, kin_ref), dev), H.Guarded((nout_ref,), dev)
            if acc:
                gw.t.copy_(gw0)
                gb.t.copy_(gb0)
            _hip.slab_reduce(slab_d, splits, nout, ld, nout_ref, kin_ref, bslab_d if with_b else None, gw.t,
                             gb.t if with_gb else None, accumulate=acc)
            torch.cuda.synchronize()
            what = f"reduce {nout}x{ld}->{nout_ref}x{kin_ref} splits {splits} acc {acc} bslab {with_b} gb {with_gb}"
            assert gw.intact() and gb.intact(), what
            rw, rb, cw, cb = H.slab_reduce_ref(slab, bslab, nout_ref, kin_ref, gw0 if acc else None, gb0 if acc else None)
            got = H._f64(gw.t)
            ratio = ((got - rw).abs() / H.slab_reduce_bar(splits, cw)).max().item()
            H.report_err("wgrad_fp64", what, ratio)
            if not ratio <= 1.0:
                fails.append(f"{what}: gw {ratio:.3g} of the bar")
            if not acc and bool((got[:, 1] != 0).any()):
                fails.append(f"{what}: a zero column summed to non-zero")
            if with_b and with_gb:
                rb_ratio = ((H._f64(gb.t) - rb).abs() / H.slab_reduce_bar(splits, cb)).max().item()
                if not rb_ratio <= 1.0:
                    fails.append(f"{what}: gb {rb_ratio:.3g} of the bar")
            else:                                                  # no bias reduce: gb keeps what it held
                keep = gb0.to(dev) if acc else torch.full_like(gb.t, SENT)
                if not torch.equal(gb.t, keep):
                    fails.append(f"{what}: gb written without bslab / gb")
    assert not fails, "\n".join(fails)
