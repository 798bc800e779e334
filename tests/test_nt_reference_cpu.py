"""The fp64 references, ceilings, emulation and inputs of the NT layer GEMMs (tests/nt_ref.py), on the CPU:
the references are torch.nn.Linear's autograd; every wrong kernel fails the per-element check the GPU module
applies (nt_hold); a plain f32 matmul and the fp16 pair emulation pass it on every kind and K of the GPU table,
so a correct kernel can."""
import pytest
import torch

from tests import helpers as H
from tests import nt_ref as N

M, NOUT = 128, 64
FWD = [(kind, k1, k2) for kind in N.NT_KINDS for k1, k2 in N.NT_FWD_K]
BWD = [(kind, k) for kind in N.NT_BWD_KINDS for k in N.NT_BWD_K]


def _seed(kind, k1, k2):
    return 1000 * N.NT_KINDS.index(kind) + k1 + 7 * k2


def test_forward_reference_is_linear():
    g = torch.Generator().manual_seed(1)
    x1, x2 = torch.randn(40, 32, generator=g), torch.randn(40, 64, generator=g)
    lin = torch.nn.Linear(96, 24).double()
    with torch.no_grad():
        want = lin(torch.cat([x1, x2], 1).double())
    for relu in (False, True):
        pre, y, cond = N.nt_fwd_ref(x1, x2, lin.weight, lin.bias, relu)
        assert torch.allclose(pre, want, rtol=0, atol=1e-13)
        assert torch.allclose(y, want.clamp_min(0) if relu else want, rtol=0, atol=1e-13)
        assert bool((cond >= pre.abs()).all()) and bool((cond >= y.abs()).all())


def test_backward_reference_is_autograd_through_a_relu():
    """dx = d/da of sum(dy * lin(relu(a))) + sum(u * (relu(a) @ v)): the gate is a > 0."""
    g = torch.Generator().manual_seed(2)
    a = torch.randn(40, 64, generator=g, dtype=torch.float64)
    a[3, 5], a[4, 6] = 0.0, -0.0
    a.requires_grad_(True)
    lin = torch.nn.Linear(64, 32).double()
    dy = torch.randn(40, 32, generator=g, dtype=torch.float64)
    u, v = torch.randn(40, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    h = torch.relu(a)
    ((lin(h) * dy).sum() + (u * (h @ v)).sum()).backward()
    bits = N.nt_gate(a.detach())
    dx, cond = N.nt_bwd_ref(dy, lin.weight.detach().t().contiguous(), u, v, bits)
    assert torch.allclose(dx, a.grad, rtol=0, atol=1e-13)
    assert bool((cond >= dx.abs()).all())
    assert dx[3, 5] == 0 and dx[4, 6] == 0 and cond[3, 5] == 0
    dx0, _ = N.nt_bwd_ref(dy, lin.weight.detach().t().contiguous(), None, None, None)
    assert torch.allclose(dx0, dy @ lin.weight.detach(), rtol=0, atol=1e-13)


def _fwd_refs(inp, relu=True):
    pre, y, cond = N.nt_fwd_ref(inp.x1, inp.x2, inp.W, inp.b, relu)
    x = N._cat(inp.x1, inp.x2)
    return pre, y, cond, x


@pytest.mark.parametrize("wrong", N.NT_WRONG_FWD)
def test_wrong_forward_fails_the_check(wrong):
    """Each wrong kernel's fp64 output -- no rounding at all -- is over the loosest ceiling (mode 1's)."""
    inp = N.nt_inputs("generic", 128, 128, 32, 64, 5)
    pre, y, cond, x = _fwd_refs(inp)
    bad = N.nt_fwd_ref(inp.x1, inp.x2, inp.W, inp.b, True, _wrong=wrong)[1]
    for mode in (0, 1, 2):
        fails = []
        N.nt_hold(wrong, bad, y, cond, N.nt_ceiling(mode, 96, cond, x, inp.W), fails)
        assert fails, (wrong, mode)
        ok = []
        N.nt_hold("right", y, y, cond, N.nt_ceiling(mode, 96, cond, x, inp.W), ok)
        assert not ok


@pytest.mark.parametrize("wrong", N.NT_WRONG_BWD)
def test_wrong_backward_fails_the_check(wrong):
    inp = N.nt_inputs("generic", 128, 128, 96, 0, 6)
    dx, cond = N.nt_bwd_ref(inp.x1, inp.W, inp.u, inp.v, inp.bits)
    bad = N.nt_bwd_ref(inp.x1, inp.W, inp.u, inp.v, inp.bits, _wrong=wrong)[0]
    for mode in (0, 1, 2):
        fails = []
        N.nt_hold(wrong, bad, dx, cond, N.nt_ceiling(mode, 96, cond, inp.x1, inp.W), fails)
        assert fails, (wrong, mode)


def test_wrong_gate_fails_the_check():
    """A gate read as >= 0: the mask bits of the gate kind's +0.0 entries differ from `stored y > 0`, and a dx
    masked by them is non-zero where the condition sum is 0."""
    inp = N.nt_inputs("gate", M, NOUT, 32, 0, 7)
    pre, y, cond, x = _fwd_refs(inp, relu=False)
    right, wrong = N.nt_gate(y), N.nt_gate(y, _wrong="gate")
    assert not torch.equal(right, wrong)
    for rows, col, val, bit in N.nt_gate_expect(inp):
        assert bool((y[rows, col] == val).all()) and bool((right[rows, col] == bit).all()), col
        if val == 0.0:
            assert bool(wrong[rows, col].all())
    g = torch.Generator().manual_seed(8)
    dy, Wt = torch.randn(M, 32, generator=g), torch.randn(NOUT, 32, generator=g)
    dx, c = N.nt_bwd_ref(dy, Wt, None, None, right)
    bad = N.nt_bwd_ref(dy, Wt, None, None, wrong)[0]
    fails = []
    N.nt_hold("gate", bad, dx, c, N.nt_ceiling(1, 32, c, dy, Wt), fails)
    assert any("condition sum is 0" in f for f in fails)


def test_wrong_emulation_fails():
    """The emulation's own switch: a dropped product is over pair_ceiling."""
    inp = N.nt_inputs("generic", M, NOUT, 32, 64, 9)
    pre, y, cond, x = _fwd_refs(inp, relu=False)
    got = N.nt_pair_emulate(inp.x1, inp.x2, inp.W, inp.r1, inp.r2, b=inp.b, _wrong="drop")
    fails = []
    N.nt_hold("drop", got, y, cond, N.nt_ceiling(2, 96, cond, x, inp.W), fails)
    assert fails


def _check_emulations(what, inp, ref, cond, x, K, kw):
    """The plain f32 matmul under the mode-0 ceiling (and mode 1's, which is wider), the pair emulation under
    pair_ceiling, exactness of the exact and gate kinds, the tight bar on the tight kinds."""
    fails = []
    exact = inp.kind in ("exact", "gate")
    f32 = N.nt_f32_emulate(inp.x1, inp.x2, inp.W, **kw)
    e0 = N.nt_hold(f"{what} f32", f32, ref, cond, N.nt_ceiling(0, K, cond, x, inp.W), fails, exact=exact)
    assert bool((N.nt_ceiling(1, K, cond, x, inp.W) >= N.nt_ceiling(0, K, cond, x, inp.W)).all())
    pair = N.nt_pair_emulate(inp.x1, inp.x2, inp.W, inp.r1, inp.r2, **kw)
    e2 = N.nt_hold(f"{what} pair", pair, ref, cond, N.nt_ceiling(2, K, cond, x, inp.W), fails, exact=exact)
    if inp.kind in N.NT_TIGHT:
        if e2 > H.tight_bar(e0):
            fails.append(f"{what}: pair e {e2 / H.U24:.2f} ulp over the tight bar (f32 {e0 / H.U24:.2f} ulp)")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kind,k1,k2", FWD)
def test_forward_kinds_can_pass(kind, k1, k2):
    inp = N.nt_inputs(kind, M, NOUT, k1, k2, _seed(kind, k1, k2))
    assert torch.equal(inp.r1, inp.x1.abs().amax(1))
    relu = kind != "gate"
    pre, y, cond, x = _fwd_refs(inp, relu)
    assert bool((cond >= y.abs()).all())
    if kind in N.NT_TIGHT:
        assert int((cond == 0).sum()) <= 0.01 * cond.numel(), int((cond == 0).sum())
    if kind == "zeros":
        assert int((cond == 0).sum()) > 0 and int((inp.r1 == 0).sum()) >= 1
    if kind == "cancel":
        assert bool((pre.abs() <= 2.0 ** -10 * cond).all())
    if kind == "exact":
        assert torch.unique(y).numel() == y.numel() and bool((y == y.float().double()).all())
    if kind == "gate":
        for rows, col, val, bit in N.nt_gate_expect(inp):
            assert bool((y[rows, col] == val).all()) and bool((N.nt_gate(y)[rows, col] == bit).all()), col
        y = y.float().double()      # the one rounding of integer + bias
    _check_emulations(f"fwd {kind} {k1}+{k2}", inp, y, cond, x, k1 + k2, dict(b=inp.b, relu=relu))


@pytest.mark.parametrize("kind,k", BWD)
def test_backward_kinds_can_pass(kind, k):
    inp = N.nt_inputs(kind, M, NOUT, k, 0, _seed(kind, k, 0))
    dx, cond = N.nt_bwd_ref(inp.x1, inp.W, inp.u, inp.v, inp.bits)
    live = inp.bits
    assert bool((cond[~live] == 0).all()) and bool((dx[~live] == 0).all())
    if kind in N.NT_TIGHT:      # the cap, over the elements whose bit is set (a clear bit is cond == 0 by definition)
        assert int((cond[live] == 0).sum()) <= 0.01 * int(live.sum())
    if kind == "cancel":
        assert bool((dx.abs() <= 2.0 ** -10 * cond).all())
    if kind == "exact":
        full = N.nt_bwd_ref(inp.x1, inp.W, inp.u, inp.v, None)[0]
        assert torch.unique(full).numel() == full.numel() and bool((full == full.float().double()).all())
    _check_emulations(f"bwd {kind} {k}", inp, dx, cond, inp.x1, k, dict(u=inp.u, v=inp.v, bits=inp.bits))


def test_exact_kind_is_distinct_at_every_table_shape():
    """out differs at every (row, column) at every shape and K of the GPU table (forward and backward)."""
    for m, n in N.NT_SHAPES:
        for K in sorted({k1 + k2 for k1, k2 in N.NT_FWD_K} | set(N.NT_BWD_K)):
            x, W = N._exact_operands(m, n, K)
            out = x.double() @ W.double().t()
            assert torch.unique(out).numel() == out.numel(), (m, n, K)
            assert out.max().item() < 2 ** 20
