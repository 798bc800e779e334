"""The NT layer GEMMs -- nerf_linear_fwd, nerf_linear_fwd_heads, nerf_linear_bwd_data: k_gemm_nt (csrc/gemm_f32.hip),
k_gemm_nt_x6 (csrc/gemm_x6.hip) and their epilogue nt_epilogue_direct (csrc/gemm.hpp) -- against fp64, per element,
at every tile, K and stride edge (GPU only).  References, ceilings and input kinds: tests/nt_ref.py.

Every call reads its activations from interior column views of NaN-filled buffers (ld > columns), u from column 0
of an [m][4] buffer of NaN, the incoming mask from [m][n/32 + 1] words with garbage in the extra word, and writes
y / dx (ld = n + 8), mask_out (ldmo = n/32 + 1), the row and the column maxima into sentinel-guarded buffers.  It
is held to: a finite result; nt_ceiling per element; exactly 0 where the condition sum is 0; torch.equal on the
exact and gate kinds; the sentinel in every guard, pad column and pad word; mask_out == stored y > 0 bit for bit;
in mode 2 y_rmax / y_cmax torch.equal to the maxima of the stored values, from a sentinel-filled buffer (the header
promises that no pre-zeroing is needed at any n or policy); exactly one launch of the expected kind with 1, 6 or 3
MFMA products per term (1 without the weight image); a second identical call bit-identical; and on the tight kinds
max e of modes 1 and 2 <= tight_bar(max e of mode 0) on the same operands, policy and shape.

The table.  Every (m x n, policy) case runs every K of its direction in all three modes, the kind, the ReLU flag
and the form of the weight image (whole, or rows [64, 64 + n) of a taller image whose other rows are 2^20 larger)
rotating with the case and the K -- so every instantiation sees K = 32, a two-segment K (forward; backward: 96,
the third clamp pattern of the prefetch) and the largest K of its direction (forward 320, backward 256: the
backward list of the issue ends there), and every kind meets every mode, policy and K.
    forward  (k1, k2): (32, 0) (64, 0) (32, 64) (256, 32) (256, 64)        backward  k: 32 64 96 128 256
    m x n      policy 1                policy 2                policy 3 (f32, bf16x3 / pair)
    128 x  64  128x64                  128x64                  128x64
    256 x 192  128x64, 2 x 3 blocks    128x64                  128x64
    384 x 128  128x128                 128x128                 128x128
    256 x 256  128x128, 2 col blocks   128x256                 256x256 / 128x256
    384 x 256  128x128                 128x256                 128x256 (m % 256 != 0) / 128x256
    128 x 320  128x64, 5 col blocks    128x64                  128x64
    128 x 384  128x128, 3 col blocks   128x128                 128x128
    256 x 512  128x128, 4 col blocks   128x256, 2 col blocks   256x256, 2 col blocks / 128x256
Each tile exists as k_gemm_nt (mode 0, and any mode without the image), k_gemm_nt_x6 bf16x3 (mode 1) and
k_gemm_nt_x6 fp16 pair (mode 2; no 256x256), each with the forward and the backward epilogue; the fused heads add
the pair kernel's 128x128 and 128x256 head instantiations.  INSTANTIATIONS lists them; test_table_reaches_every_
instantiation derives the set the table reaches from the dispatch rule, and every call asserts its product count."""
import contextlib
import functools

import pytest
import torch

from model import _hip
from tests import helpers as H
from tests import nt_ref as N

pytestmark = pytest.mark.gpu
SENT = H.SENT
MSENT = 0x5a5a5a5a
PRODUCTS = {0: 1, 1: 6, 2: 3}
NAMES = {0: "f32", 1: "bf16x3", 2: "pair"}
POLICIES = (1, 2, 3)
TILES = ((128, 64), (128, 128), (128, 256), (256, 256))
INSTANTIATIONS = frozenset([(k, t, e) for k in ("f32", "bf16x3", "pair") for t in TILES for e in ("fwd", "dx")
                            if not (k == "pair" and t == (256, 256))] +
                           [("pair-heads", (128, 128), "fwd"), ("pair-heads", (128, 256), "fwd")])


@contextlib.contextmanager
def _gemm(mode, policy):
    """Precision mode and NT policy for the block; policy 0 and the previous mode restored."""
    prev = _hip.gemm_get_precision()
    try:
        _hip.gemm_set_precision(mode)
        _hip.gemm_set_policy(policy, 0)
        yield
    finally:
        _hip.gemm_set_policy(0, 0)
        _hip.gemm_set_precision(prev)


def _tile(mode, image, policy, m, n, heads=False):
    """(kernel, (BM, BN)) of dispatch_nt (csrc/gemm_f32.hip) and pick_nt_x6 (csrc/gemm_x6.hip)."""
    pol = policy or 3
    if mode == 2 and image:
        if heads:
            return "pair-heads", (128, 256 if n == 256 else 128)
        return "pair", ((128, 256) if pol >= 2 and n % 256 == 0 else (128, 128) if n % 128 == 0 else (128, 64))
    name = NAMES[mode] if image and mode else "f32"
    if pol == 3 and m % 256 == 0 and n % 256 == 0:
        return name, (256, 256)
    return name, ((128, 256) if pol >= 2 and n % 256 == 0 else (128, 128) if n % 128 == 0 else (128, 64))


def _wide(t, dev, pad=4):
    """t as a column-offset view (16-byte aligned offset, ld > columns, ld % 4 == 0) of a NaN-filled buffer."""
    buf = torch.full((t.shape[0], t.shape[1] + 2 * pad), float("nan"), device=dev)
    v = buf[:, pad:pad + t.shape[1]]
    v.copy_(t)
    assert v.data_ptr() % 16 == 0 and v.stride(0) > t.shape[1] and v.stride(0) % 4 == 0
    return v


def _weights(dev, W, mode, sliced, image=True):
    """-> (f32 weight [n][K], its image or None) in the form of the current precision mode, from nerf_pack_weights;
    sliced: both are rows [64, 64 + n) of a taller matrix whose other rows are 2^20 larger (w_split_rows > n)."""
    n, K = W.shape
    r0 = 64 if sliced else 0
    tall = W
    if sliced:
        g = torch.Generator().manual_seed(n + K)
        alien = lambda r: (torch.rand(r, K, generator=g) * 2 - 1) * 2.0 ** 20      # noqa: E731
        tall = torch.cat([alien(r0), W, alien(64)])
    rows = tall.shape[0]
    src = tall.to(dev).contiguous()
    if mode == 0 or not image:
        return src[r0:r0 + n], None
    Wp, Wt = torch.zeros(rows, K, device=dev), torch.zeros(K, rows, device=dev)
    ws, wts = _hip.split_image(rows, K, dev), _hip.split_image(K, rows, dev)
    _hip.pack_weights([_hip.PackDesc(src.data_ptr(), Wp.data_ptr(), Wt.data_ptr(), rows, K, K, K, rows, ws.data_ptr(),
                                     wts.data_ptr())])
    return Wp[r0:r0 + n], ws[:, :, r0:r0 + n]


def _profiled(fn, kind):
    """-> (launches of `kind`, launches of every other kind, MFMA products per term) around fn()."""
    _hip.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        k = _hip.prof_read_kinds()
    finally:
        _hip.prof_enable(False)
    fl = k[kind]["flops"]
    ratio = k[kind]["mfma_flops"] / fl if fl else 0.0
    return k[kind]["launches"], sum(v["launches"] for v in k.values()) - k[kind]["launches"], ratio


class _Outs:
    """Guarded outputs of one call: out [m][n + 8], mask words [m][n/32 + 1], row maxima [m], column maxima."""

    def __init__(self, dev, m, n):
        self.m, self.n = m, n
        self.out = H.Guarded((m, n + 8), dev)
        self.mo = H.Guarded((m, n // 32 + 1), dev, dtype=torch.int32, fill=MSENT)
        self.rm = H.Guarded((m,), dev)
        self.cm = H.Guarded((m // 128, n), dev)
        self.y, self.words = self.out.t[:, :n], self.mo.t[:, :n // 32]

    def snapshot(self):
        return [t.clone() for t in (self.out.buf, self.mo.buf, self.rm.buf, self.cm.buf)]

    def check(self, what, fails, mask, maxima):
        n = self.n
        if not (self.out.intact() and self.mo.intact() and self.rm.intact() and self.cm.intact()):
            fails.append(f"{what}: a guard was written")
        if not bool((self.out.t[:, n:] == SENT).all()):
            fails.append(f"{what}: output columns outside [0, n) written")
        if not bool((self.mo.t[:, n // 32:] == MSENT).all()):
            fails.append(f"{what}: mask words outside [0, n/32) written")
        if not mask and not self.mo.untouched():
            fails.append(f"{what}: mask_out written though NULL was passed")
        if not maxima and not (self.rm.untouched() and self.cm.untouched()):
            fails.append(f"{what}: row / column maxima written outside the fp16 pair kernel")
        if maxima:
            y = self.y
            if not torch.equal(self.rm.t, y.abs().amax(1)):
                bad = int((self.rm.t != y.abs().amax(1)).sum())
                fails.append(f"{what}: row maxima differ from amax |stored value| in {bad} rows")
            if not torch.equal(self.cm.t, y.abs().view(self.m // 128, 128, n).amax(1)):
                fails.append(f"{what}: column maxima differ from the 128-row group maxima of the stored values")


def _run(what, call, outs, kind, want_products, fails, mask=True, maxima=False):
    """The call profiled, then once more: one launch of `kind`, the product count, bit-identical outputs."""
    launches, others, ratio = _profiled(call, kind)
    if (launches, others) != (1, 0) or abs(ratio - want_products) > 1e-9:
        fails.append(f"{what}: {launches} launches of {kind} ({others} others) with {ratio:g} products per term, "
                     f"expected 1 with {want_products}")
    first = outs.snapshot()
    call()
    torch.cuda.synchronize()
    if not all(torch.equal(a, b) for a, b in zip(first, outs.snapshot())):
        fails.append(f"{what}: a second identical call differs")
    outs.check(what, fails, mask, maxima)


@functools.lru_cache(maxsize=8)
def _fwd_ref(kind, m, n, k1, k2, relu):
    inp = N.nt_inputs(kind, m, n, k1, k2, 7919 * N.NT_KINDS.index(kind) + 3 * m + 5 * n + k1 + 11 * k2)
    pre, y, cond = N.nt_fwd_ref(inp.x1, inp.x2, inp.W, inp.b, relu)
    if kind == "gate":
        y = y.float().double()          # integer + bias: the one rounding of the epilogue's add
    return inp, y, cond, N._cat(inp.x1, inp.x2)


@functools.lru_cache(maxsize=8)
def _bwd_ref(kind, m, n, k, plain):
    inp = N.nt_inputs(kind, m, n, k, 0, 104729 * N.NT_KINDS.index(kind) + 3 * m + 5 * n + k)
    if plain:
        inp.u = inp.v = inp.bits = None
    dx, cond = N.nt_bwd_ref(inp.x1, inp.W, inp.u, inp.v, inp.bits)
    return inp, dx, cond


def _forward(dev, what, inp, ref, cond, x, mode, policy, relu, sliced, fails, image=True):
    """One nerf_linear_fwd call under (mode, policy) held to everything of the module docstring -> max e."""
    m, n, k1, k2 = inp.m, inp.n, inp.k1, inp.k2
    pair = mode == 2 and image
    eff = mode if image else 0
    with _gemm(mode, policy):
        w, ws = _weights(dev, inp.W, mode, sliced, image)
        x1, x2 = _wide(inp.x1, dev), (_wide(inp.x2, dev) if k2 else None)
        b = inp.b.to(dev)
        r1 = inp.r1.to(dev) if mode == 2 else None
        r2 = inp.r2.to(dev) if mode == 2 and k2 else None
        outs = _Outs(dev, m, n)
        call = lambda: _hip.linear_fwd(x1, k1, x2, k2, w, b, outs.y, m, n, relu, mask_out=outs.words, w_split=ws,      # noqa: E731
                                       x1_rmax=r1, x2_rmax=r2, y_rmax=outs.rm.t if pair else None,
                                       y_cmax=outs.cm.t if pair else None)
        _run(what, call, outs, "fwd", PRODUCTS[eff], fails, maxima=pair)
    y = outs.y.cpu()
    e = N.nt_hold(what, y, ref, cond, N.nt_ceiling(eff, k1 + k2, cond, x, inp.W), fails, exact=inp.kind in ("exact", "gate"))
    if not torch.equal(H.relu_bits(outs.words, n), y > 0):
        fails.append(f"{what}: mask_out differs from stored y > 0")
    if inp.kind == "gate":
        bits = H.relu_bits(outs.words, n)
        for rows, col, val, bit in N.nt_gate_expect(inp):
            val = max(val, 0.0) if relu else val
            if not bool((y[rows, col].double() == val).all()) or not bool((bits[rows, col] == bit).all()):
                fails.append(f"{what}: gate column {col}: stored {y[rows, col][:2].tolist()} bits "
                             f"{bits[rows, col][:2].tolist()}, expected {val!r} and {bit}")
    return e


def _backward(dev, what, inp, ref, cond, mode, policy, sliced, fails, image=True):
    """One nerf_linear_bwd_data call under (mode, policy) -> max e."""
    m, n, k = inp.m, inp.n, inp.k1
    pair = mode == 2 and image
    eff = mode if image else 0
    with _gemm(mode, policy):
        w, ws = _weights(dev, inp.W, mode, sliced, image)
        dy = _wide(inp.x1, dev)
        u = v = words = None
        if inp.u is not None:
            u = torch.full((m, 4), float("nan"), device=dev)
            u[:, 0] = inp.u.to(dev)
            v = inp.v.to(dev)
        if inp.bits is not None:
            words = torch.randint(-2 ** 31, 2 ** 31 - 1, (m, n // 32 + 1), dtype=torch.int32,
                                  generator=torch.Generator().manual_seed(m + n)).to(dev)
            words[:, :n // 32] = H.relu_words(inp.bits).to(dev)
            words = words[:, :n // 32]
        r1 = inp.r1.to(dev) if mode == 2 else None
        outs = _Outs(dev, m, n)
        call = lambda: _hip.linear_bwd_data(dy, k, w, outs.y, m, n, mask=words, u=u, ldu=4, v=v, wt_split=ws,      # noqa: E731
                                            dy_rmax=r1, dx_rmax=outs.rm.t if pair else None,
                                            dx_cmax=outs.cm.t if pair else None)
        _run(what, call, outs, "dx", PRODUCTS[eff], fails, mask=False, maxima=pair)
    return N.nt_hold(what, outs.y.cpu(), ref, cond, N.nt_ceiling(eff, k, cond, inp.x1, inp.W), fails,
                     exact=inp.kind == "exact")


def _tight(what, kind, e, fails):
    """Modes 1 and 2 against mode 0 on the same operands, policy and shape: tight_bar, on the tight kinds."""
    for mode in (1, 2):
        ratio = e[mode] / H.tight_bar(e[0])
        print(f"{what}: max e f32 {e[0] / H.U24:.2f} ulp, {NAMES[mode]} {e[mode] / H.U24:.2f} ulp, "
              f"{NAMES[mode]} / tight_bar(f32) = {ratio:.3f}" + ("" if kind in N.NT_TIGHT else "  (not a tight kind)"))
        H.report_err("nt_fp64", f"{what} {NAMES[mode]} tight ratio", ratio)
        if kind in N.NT_TIGHT and ratio > 1.0:
            fails.append(f"{what}: {NAMES[mode]} e {e[mode] / H.U24:.2f} ulp over the tight bar (f32 {e[0] / H.U24:.2f} ulp)")


def _rotation(m, n, policy, i):
    return 3 * N.NT_SHAPES.index((m, n)) + policy - 1 + i


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("m,n", N.NT_SHAPES)
def test_linear_fwd_fp64(dev, m, n, policy):
    fails = []
    for i, (k1, k2) in enumerate(N.NT_FWD_K):
        c = _rotation(m, n, policy, i)
        kind, relu, sliced = N.NT_KINDS[c % len(N.NT_KINDS)], c % 3 != 0, c % 2 == 1
        inp, ref, cond, x = _fwd_ref(kind, m, n, k1, k2, relu)
        e = {}
        for mode in (0, 1, 2):
            kernel, tile = _tile(mode, True, policy, m, n)
            what = f"fwd {m}x{n} K {k1}+{k2} nt{policy} {kind} relu {int(relu)} {'slice' if sliced else 'whole'} {kernel}"
            print(f"{what}: tile {tile[0]}x{tile[1]}, {m // tile[0]} x {n // tile[1]} blocks")
            e[mode] = _forward(dev, what, inp, ref, cond, x, mode, policy, relu, sliced, fails)
            H.report_err("nt_fp64", f"{what} e", e[mode])
        _tight(f"fwd {m}x{n} K {k1}+{k2} nt{policy} {kind}", kind, e, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("m,n", N.NT_SHAPES)
def test_linear_bwd_data_fp64(dev, m, n, policy):
    fails = []
    for i, k in enumerate(N.NT_BWD_K):
        c = _rotation(m, n, policy, i)
        kind, sliced, plain = N.NT_BWD_KINDS[c % len(N.NT_BWD_KINDS)], c % 2 == 1, c % 5 == 4
        inp, ref, cond = _bwd_ref(kind, m, n, k, plain)
        e = {}
        for mode in (0, 1, 2):
            kernel, tile = _tile(mode, True, policy, m, n)
            what = (f"dx {m}x{n} K {k} nt{policy} {kind} {'plain' if plain else 'mask+u'} "
                    f"{'slice' if sliced else 'whole'} {kernel}")
            print(f"{what}: tile {tile[0]}x{tile[1]}, {m // tile[0]} x {n // tile[1]} blocks")
            e[mode] = _backward(dev, what, inp, ref, cond, mode, policy, sliced, fails)
            H.report_err("nt_fp64", f"{what} e", e[mode])
        _tight(f"dx {m}x{n} K {k} nt{policy} {kind}", kind, e, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("m,n,policy", [(128, 64, 1), (256, 256, 3), (256, 512, 2)])
def test_without_the_image_the_exact_f32_kernel_runs(dev, mode, m, n, policy):
    """w_split / wt_split NULL: one product per term in modes 1 and 2 (the header's promise), mode 0's ceiling."""
    fails = []
    inp, ref, cond, x = _fwd_ref("spread", m, n, 32, 64, True)
    _forward(dev, f"fwd {m}x{n} nt{policy} mode {mode} no image", inp, ref, cond, x, mode, policy, True, False, fails,
             image=False)
    inp, ref, cond = _bwd_ref("spread", m, n, 96, False)
    _backward(dev, f"dx {m}x{n} nt{policy} mode {mode} no image", inp, ref, cond, mode, policy, False, fails, image=False)
    assert not fails, "\n".join(fails)


def test_table_reaches_every_instantiation():
    """The dispatch rule over the table (and the heads table) names every instantiation of the family."""
    reached = set()
    for m, n in N.NT_SHAPES:
        for policy in POLICIES:
            for mode in (0, 1, 2):
                kernel, tile = _tile(mode, True, policy, m, n)
                reached |= {(kernel, tile, "fwd"), (kernel, tile, "dx")}
    for n in HEAD_N:
        reached.add(_tile(2, True, 1, 128, n, heads=True) + ("fwd",))
    assert reached == INSTANTIATIONS, (sorted(INSTANTIATIONS - reached), sorted(reached - INSTANTIATIONS))


# ---- nerf_linear_fwd_heads ---------------------------------------------------------------------------------------
HEAD_N = (128, 256)
HEAD_PAIRS = tuple((nh, col) for nh in (1, 2, 3) for col in range(0, 5 - nh))      # every valid (n_heads, raw_col)
HEAD_KINDS = ("generic", "zeros", "exact")


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("k1,k2", [(32, 0), (256, 64)])
@pytest.mark.parametrize("n", HEAD_N)
@pytest.mark.parametrize("m", [128, 384])
def test_linear_fwd_heads_fp64(dev, m, n, k1, k2, policy):
    """Mode 2: y, mask_out, y_rmax and y_cmax torch.equal to nerf_linear_fwd's on the same operands; raw4's head
    columns against the fp64 dot of the kernel's own stored y with the head weights (dot_ceiling: the head's error
    alone); the other raw4 columns and the guards keep the sentinel."""
    fails = []
    assert len(HEAD_PAIRS) == 9
    for ki, kind in enumerate(HEAD_KINDS):
        inp, ref, cond, x = _fwd_ref(kind, m, n, k1, k2, True)
        g = torch.Generator().manual_seed(m + n + k1 + ki)
        with _gemm(2, policy):
            w, ws = _weights(dev, inp.W, 2, ki % 2 == 1)
            x1, x2 = _wide(inp.x1, dev), (_wide(inp.x2, dev) if k2 else None)
            b, r1, r2 = inp.b.to(dev), inp.r1.to(dev), (inp.r2.to(dev) if k2 else None)
            base = _Outs(dev, m, n)
            _hip.linear_fwd(x1, k1, x2, k2, w, b, base.y, m, n, True, mask_out=base.words, w_split=ws, x1_rmax=r1,
                            x2_rmax=r2, y_rmax=base.rm.t, y_cmax=base.cm.t)
            torch.cuda.synchronize()
            want = base.snapshot()
            for nh, col in HEAD_PAIRS[ki::len(HEAD_KINDS)]:
                what = f"heads {m}x{n} K {k1}+{k2} nt{policy} {kind} n_heads {nh} raw_col {col}"
                kernel, tile = _tile(2, True, policy, m, n, heads=True)
                print(f"{what}: {kernel} tile {tile[0]}x{tile[1]}")
                hw = (torch.rand(nh, n, generator=g) * 2 - 1)
                hb = (torch.rand(nh, generator=g) * 2 - 1)
                if kind == "zeros":
                    hw[:, 1::8] = 0
                outs, raw4 = _Outs(dev, m, n), H.Guarded((m, 4), dev)
                hwd, hbd = hw.to(dev).contiguous(), hb.to(dev)
                call = lambda: _hip.linear_fwd(x1, k1, x2, k2, w, b, outs.y, m, n, True, mask_out=outs.words, w_split=ws,      # noqa: E731
                                               x1_rmax=r1, x2_rmax=r2, y_rmax=outs.rm.t, y_cmax=outs.cm.t,
                                               heads=(hwd, hbd, raw4.t, col))
                _run(what, call, outs, "fwd", 3, fails, maxima=True)
                if not all(torch.equal(a, b_) for a, b_ in zip(want, outs.snapshot())):
                    fails.append(f"{what}: y, mask_out, y_rmax or y_cmax differ from nerf_linear_fwd's")
                y = H._f64(outs.y)
                href = y @ hw.double().t() + hb.double()
                hcond = y.abs() @ hw.double().abs().t() + hb.double().abs()
                r = raw4.t.cpu()
                N.nt_hold(what + " raw4", r[:, col:col + nh], href, hcond, H.dot_ceiling(n, hcond), fails)
                others = [c for c in range(4) if not col <= c < col + nh]
                if not raw4.intact() or not bool((r[:, others] == SENT).all()):
                    fails.append(f"{what}: raw4 written outside its head columns")
        N.nt_hold(f"heads {m}x{n} K {k1}+{k2} nt{policy} {kind} y", base.y.cpu(), ref, cond,
                  N.nt_ceiling(2, k1 + k2, cond, x, inp.W), fails, exact=kind == "exact")
    assert not fails, "\n".join(fails)


# ---- entry checks ------------------------------------------------------------------------------------------------
def _strided(dev, rows, ld, cols, dtype=torch.float32):
    """A [rows][cols] view with row stride ld < cols (overlapping rows): only ever handed to a call that must
    refuse it before any launch."""
    return torch.zeros(rows * cols, device=dev, dtype=dtype).as_strided((rows, cols), (ld, 1))


def test_entry_checks(dev):
    """Each bad argument returns NERF_EINVAL from check_nt or the entry function, before any launch, with the
    outputs untouched.  Nothing here is accepted by the checks."""
    m, n, k = 128, 64, 32
    inp = N.nt_inputs("generic", 256, 256, 32, 0, 1)
    with _gemm(2, 0):
        W, ws = _weights(dev, inp.W, 2, False)
        x, r1, b = inp.x1.to(dev), inp.r1.to(dev), inp.b.to(dev)
        u, v = inp.u.to(dev), inp.v.to(dev)
        words = torch.zeros(256, 9, device=dev, dtype=torch.int32)
        outs, raw4 = _Outs(dev, 256, 256), H.Guarded((256, 4), dev)
        y, mo = outs.out.t, outs.mo.t
        hw, hb = torch.zeros(3, 256, device=dev), torch.zeros(3, device=dev)
        small = _hip.split_image(n - 8, k, dev)

        def fwd(m=m, n=n, k1=k, y=y, mo=mo, ws=ws, r1=r1, **kw):
            _hip.linear_fwd(x, k1, None, 0, W, b, y, m, n, 1, mask_out=mo, w_split=ws, x1_rmax=r1, y_rmax=outs.rm.t,
                            y_cmax=outs.cm.t, **kw)

        def dx(m=m, n=n, k=k, mask=words, ws=ws, u=None, v=None, r1=r1):
            _hip.linear_bwd_data(x, k, W, y, m, n, mask=mask, u=u, ldu=1, v=v, wt_split=ws, dy_rmax=r1,
                                 dx_rmax=outs.rm.t, dx_cmax=outs.cm.t)

        cases = {
            "m = 64": lambda: fwd(m=64), "n = 32": lambda: fwd(n=32), "k1 = 16": lambda: fwd(k1=16),
            "ldy < n": lambda: fwd(y=_strided(dev, m, n - 4, n)),
            "ldmo < n/32": lambda: fwd(mo=_strided(dev, m, 1, 2, torch.int32)),
            "w_split_rows < n": lambda: fwd(ws=small),
            "mode 2 without row maxima": lambda: fwd(r1=None),
            "heads n = 192": lambda: fwd(n=192, heads=(hw, hb, raw4.t, 0)),
            "heads raw_col + n_heads > 4": lambda: fwd(n=256, m=256, heads=(hw, hb, raw4.t, 2)),
            "dx m = 64": lambda: dx(m=64), "dx n = 32": lambda: dx(n=32), "dx k = 16": lambda: dx(k=16),
            "ldmask < n/32": lambda: dx(mask=_strided(dev, m, 1, 2, torch.int32)),
            "dx wt_split_rows < n": lambda: dx(ws=small),
            "u without v": lambda: dx(u=u),
            "dx mode 2 without row maxima": lambda: dx(r1=None),
        }
        for name, call in cases.items():
            with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
                call()
            torch.cuda.synchronize()
            assert outs.out.untouched() and outs.mo.untouched() and outs.rm.untouched() and outs.cm.untouched() and \
                raw4.untouched(), f"{name}: an output was written"
