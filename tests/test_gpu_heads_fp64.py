"""The head kernels (k_heads_fwd, k_heads_bwd, k_heads_dyr, k_heads_reduce in render.hip) against the
header's formulas in fp64 (tests/helpers.py heads_ref), per element (GPU only).

  * raw4 and dyr per element <= dot_ceiling (hidden, hidden / 2 or 3 terms); dyr exactly 0 behind a closed gate;
  * dyr_rmax / dyr_cmax bitwise the maxima of the stored dyr;
  * the four sums <= heads_sum_ceiling (the kernels' summation order), accumulate 0 and 1;
  * every output in a sentinel-guarded buffer; h8, hr and dyr as views with ld > width; `part` of exactly
    nerf_heads_part_size;
  * modes 3, 1, 2 and mode 1 gated by mask bits, both mode-1 kernels (n_pad % 128 == 0 and != 0), the maxima
    absent in turn.
The inputs (heads_inputs) carry dead columns, 0.0, -0.0 and the smallest subnormal in hr, and zero, sigma-only
and rgb-only rows of graw4 scaled by 2^+-30."""
import pytest
import torch

from model import _hip
from tests import helpers as H

pytestmark = pytest.mark.gpu
SENT = H.SENT
N_SMALL = (16, 48, 64, 80, 128, 144) + tuple(64 * b - 48 for b in (4, 5, 8, 9, 13)) + (16384,)


def _view(t, dev, pad=4):
    """t as a column-offset view (ld > width) of a NaN-filled device buffer."""
    buf = torch.full((t.shape[0], t.shape[1] + 2 * pad), float("nan"), device=dev)
    v = buf[:, pad:pad + t.shape[1]]
    v.copy_(t)
    return v


class _Dyr:
    """dyr [n][HR] as a column-offset view of a guarded [n][HR + 8] buffer."""

    def __init__(self, n, HR, dev):
        self.g = H.Guarded((n, HR + 8), dev)
        self.v = self.g.t[:, 4:4 + HR]

    def read(self, what):
        assert self.g.intact() and bool((self.g.t[:, :4] == SENT).all()) and bool((self.g.t[:, -4:] == SENT).all()), \
            f"{what}: written outside dyr"
        return self.v


def _ratio(got, ref, ceil):
    got = got.to(ref.device).double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all())
    return ((got - ref).abs() / ceil).max().item()


def _check_dyr(what, dyr, rm, cm, r, fails):
    d = dyr.read(what)
    ratio = _ratio(d, r["dyr"], H.dot_ceiling(3, r["c_dyr"]) + H.F32_TINY)
    H.report_err("heads_fp64", f"{what} dyr ceiling ratio", ratio)
    if ratio > 1.0:
        fails.append(f"{what}: dyr {ratio:.3g} of its ceiling")
    if bool((d.to(r["gate"].device)[~r["gate"]] != 0).any()):
        fails.append(f"{what}: dyr not 0 behind a closed gate")
    if rm is not None:
        assert rm.intact()
        if not torch.equal(rm.t, d.abs().amax(1)):
            fails.append(f"{what}: dyr_rmax is not the row maxima of the stored dyr")
    if cm is not None:
        assert cm.intact()
        if not torch.equal(cm.t, d.abs().reshape(d.shape[0] // 128, 128, -1).amax(1)):
            fails.append(f"{what}: dyr_cmax is not the column maxima of the stored dyr")


def _check_sums(what, part, hidden, HR, n, r, dev, fails):
    """nerf_heads_reduce of `part` (accumulate 0, then 1 onto given gradients) against the four sums."""
    blocks = _hip.heads_part_size(hidden, n) // (hidden + 3 * HR + 4)
    assert part.intact(), f"{what}: written outside part"
    g0 = {k: torch.rand(s, generator=torch.Generator().manual_seed(i), dtype=torch.float32) - 0.5
          for i, (k, s) in enumerate((("gwd", (hidden,)), ("gbd", (1,)), ("gwc", (3, HR)), ("gbc", (3,))))}
    for acc in (False, True):
        out = {k: H.Guarded(tuple(v.shape), dev) for k, v in g0.items()}
        if acc:
            for k in out:
                out[k].t.copy_(g0[k])
        _hip.heads_reduce(part.t, hidden, n, out["gwd"].t, out["gbd"].t, out["gwc"].t, out["gbc"].t, accumulate=acc)
        torch.cuda.synchronize()
        for k, o in out.items():
            assert o.intact(), f"{what}: written outside {k}"
            ref, cond = r[k], r["c_" + k]
            if acc:
                base = g0[k].to(ref.device).double().reshape(ref.shape)
                ref, cond = ref + base, cond + base.abs()
            ratio = _ratio(o.t, ref, H.heads_sum_ceiling(n, blocks, cond))
            H.report_err("heads_fp64", f"{what} {k} acc {int(acc)} ceiling ratio", ratio)
            if ratio > 1.0:
                fails.append(f"{what}: {k} (accumulate {int(acc)}) {ratio:.3g} of its ceiling")
            if bool((o.t.to(cond.device).reshape(cond.shape)[cond == 0] != 0).any()):
                fails.append(f"{what}: {k} non-zero where every term is 0")


def _heads_case(dev, hidden, n, on_device=False):
    HR = max(64, hidden // 2)
    inp = H.heads_inputs(hidden, n, hidden * 31 + n, device=dev if on_device else "cpu")
    r = H.heads_ref(inp["h8"], inp["hr"], inp["wd"], inp["bd"], inp["wc"], inp["bc"], inp["graw4"])
    d = {k: v.to(dev) for k, v in inp.items()}
    h8, hr = _view(d["h8"], dev), _view(d["hr"], dev)
    G = d["graw4"].contiguous()
    fails = []
    what = f"heads {hidden} n {n}"
    # forward
    raw4 = H.Guarded((n, 4), dev)
    _hip.heads_fwd(h8, hr, hidden, d["wd"], d["bd"], d["wc"], d["bc"], raw4.t, n)
    torch.cuda.synchronize()
    assert raw4.intact()
    ceil = torch.cat([H.dot_ceiling(hidden, r["c_raw4"][:, :1]), H.dot_ceiling(HR, r["c_raw4"][:, 1:])], 1)
    ratio = _ratio(raw4.t, r["raw4"], ceil)
    H.report_err("heads_fp64", f"{what} raw4 ceiling ratio", ratio)
    if ratio > 1.0:
        fails.append(f"{what}: raw4 {ratio:.3g} of its ceiling")
    psize = _hip.heads_part_size(hidden, n)
    groups = n % 128 == 0
    mk_rm = lambda: H.Guarded((n,), dev)                                       # noqa: E731
    mk_cm = lambda: H.Guarded((n // 128, HR), dev) if groups else None         # noqa: E731
    bits = H.relu_words(d["hr"] > 0)
    # mode 3: dyr + maxima + partials
    dyr, part, rm, cm = _Dyr(n, HR, dev), H.Guarded((psize,), dev), mk_rm(), mk_cm()
    _hip.heads_bwd(G, h8, hr, hidden, d["wc"], dyr.v, part.t, n, dyr_rmax=rm.t, dyr_cmax=None if cm is None else cm.t)
    torch.cuda.synchronize()
    _check_dyr(what + " mode 3", dyr, rm, cm, r, fails)
    _check_sums(what + " mode 3", part, hidden, HR, n, r, dev, fails)
    # mode 1 by value and by mask bits (k_heads_dyr at n % 128 == 0, else k_heads_bwd<.., 1>), the maxima absent in turn
    for gate in ("value", "bits"):
        for with_rm, with_cm in ((True, True), (False, True), (True, False)):
            dyr, rm, cm = _Dyr(n, HR, dev), (mk_rm() if with_rm else None), (mk_cm() if with_cm else None)
            _hip.heads_bwd(G, None, hr if gate == "value" else None, hidden, d["wc"], dyr.v, None, n,
                           dyr_rmax=None if rm is None else rm.t, dyr_cmax=None if cm is None else cm.t, mode=1,
                           hr_mask=bits if gate == "bits" else None)
            torch.cuda.synchronize()
            _check_dyr(f"{what} mode 1 {gate} rmax {with_rm} cmax {with_cm}", dyr, rm, cm, r, fails)
    # mode 2: the partials alone
    part = H.Guarded((psize,), dev)
    _hip.heads_bwd(G, h8, hr, hidden, d["wc"], None, part.t, n, mode=2)
    torch.cuda.synchronize()
    _check_sums(what + " mode 2", part, hidden, HR, n, r, dev, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", N_SMALL)
@pytest.mark.parametrize("hidden", [64, 128, 256, 512])
def test_heads_against_fp64(dev, hidden, n):
    _heads_case(dev, hidden, n)


@pytest.mark.parametrize("n", [131072, 131200])
def test_heads_second_chunk(dev, n):
    """131 200 rows: 1025 chunks over the 1024 waves of the 256-block cap -- the first size at which a wave
    takes a second chunk (131 072: the last at which none does).  Inputs and reference built on the device."""
    _heads_case(dev, 256, n, on_device=True)


@pytest.mark.parametrize("hidden", [64, 256, 512])
def test_gate_agrees_with_linear_fwd(dev, hidden):
    """The value gate (hr > 0), the bit gate and the mask_out bit nerf_linear_fwd writes for the same value agree
    on 0.0, -0.0, the smallest positive subnormal, the smallest normal and dead columns: the colour layer's
    output through an identity weight on the exact-f32 kernel, then mode 1 by value and by its mask bits."""
    HR = max(64, hidden // 2)
    n = 128
    g = torch.Generator().manual_seed(hidden)
    pre = torch.rand(n, HR, generator=g) * 2 - 1
    pre[:, 3] = -0.5                                                     # a dead column
    pre[:, 7] = 0.0
    pre[0::4, 5], pre[1::4, 5], pre[2::4, 5], pre[3::4, 5] = 0.0, -0.0, H.F32_TINY, 2.0 ** -126
    pre[0::2, 9] = -H.F32_TINY
    _hip.gemm_set_precision(0)
    y, mo = torch.empty(n, HR, device=dev), torch.zeros(n, HR // 32, device=dev, dtype=torch.int32)
    _hip.linear_fwd(pre.to(dev), HR, None, 0, torch.eye(HR, device=dev), torch.zeros(HR, device=dev), y, n, HR, 1,
                    mask_out=mo)
    torch.cuda.synchronize()
    bits = H.relu_bits(mo, HR)
    assert torch.equal(bits, y.cpu() > 0)                                # the words are the stored values' gate
    assert torch.equal(y.cpu(), pre.clamp_min(0))                        # and the values are relu(pre), subnormals kept
    assert torch.equal(bits, pre > 0) and torch.equal(mo.cpu(), H.relu_words(pre > 0))
    inp = H.heads_inputs(hidden, n, 5)
    G, wc = inp["graw4"].to(dev), inp["wc"].to(dev)
    r = H.heads_ref(inp["h8"], y.cpu(), inp["wd"], inp["bd"], inp["wc"], inp["bc"], inp["graw4"])
    out = []
    for by_bits in (False, True):
        dyr = _Dyr(n, HR, dev)
        _hip.heads_bwd(G, None, None if by_bits else y, hidden, wc, dyr.v, None, n, mode=1, hr_mask=mo if by_bits else None)
        torch.cuda.synchronize()
        fails = []
        _check_dyr(f"gate {hidden} bits {by_bits}", dyr, None, None, r, fails)
        assert not fails, "\n".join(fails)
        out.append(dyr.read("gate").clone())
    assert torch.equal(out[0], out[1])
    open_ = (out[0] != 0).cpu()
    assert torch.equal(open_ | (r["dyr"] == 0), bits | (r["dyr"] == 0))  # open exactly where the bit is set
