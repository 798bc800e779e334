"""fp64 references, derived ceilings, a CPU emulation and the edge inputs of the NT layer GEMMs:
nerf_linear_fwd, nerf_linear_fwd_heads and nerf_linear_bwd_data (k_gemm_nt in csrc/gemm_f32.hip, k_gemm_nt_x6 in
csrc/gemm_x6.hip, the epilogue nt_epilogue_direct in csrc/gemm.hpp).  From the text of include/nerf_hip.h:
  y[m, n]  = act( sum_k x1[m, k] w[n, k] + sum_k x2[m, k] w[n, k1 + k] + bias[n] ),  mask_out bit = stored y > 0
  dx[m, j] = ( sum_o dy[m, o] wt[j, o] + u[m] v[j] ) * bit(m, j)
Plain torch on the CPU; shared by tests/test_nt_reference_cpu.py and tests/test_gpu_nt_fp64.py."""
import types

import torch

from tests import helpers as H

U24 = H.U24
NT_KINDS = ("generic", "spread", "zeros", "segments", "cancel", "gate", "exact")
NT_TIGHT = ("generic", "spread", "zeros", "segments")        # the kinds held to tight_bar
NT_BWD_KINDS = tuple(k for k in NT_KINDS if k != "gate")     # the gate kind is the forward's
NT_WRONG_FWD = ("k", "segment", "bias_after_relu", "transposed")
NT_WRONG_BWD = ("k", "transposed")
# the table of tests/test_gpu_nt_fp64.py
NT_SHAPES = ((128, 64), (256, 192), (384, 128), (256, 256), (384, 256), (128, 320), (128, 384), (256, 512))
NT_FWD_K = ((32, 0), (64, 0), (32, 64), (256, 32), (256, 64))
NT_BWD_K = (32, 64, 96, 128, 256)
EPS1 = 2.0 ** -24          # 1 - pred(1): the smallest non-zero |acc + bias| of an integer acc against a bias near 1


def _cat(x1, x2):
    return H._f64(x1) if x2 is None else torch.cat([H._f64(x1), H._f64(x2)], 1)


def nt_fwd_ref(x1, x2, W, b, relu, _wrong=None):
    """fp64 (pre, y, cond): pre = [x1 | x2] @ W.T + b, y = relu(pre) or pre, cond = |x| @ |W|.T + |b|.
    _wrong (the wrong kernels of tests/test_nt_reference_cpu.py, nothing else): "k" one k (the middle one)
    left out; "segment" the segment boundary one 16-wide K tile early (the last tile of x1 read from the start
    of x2; needs x2); "bias_after_relu"; "transposed" the output written transposed into the same buffer."""
    x, W = _cat(x1, x2), H._f64(W)
    b = torch.zeros(W.shape[0], dtype=torch.float64) if b is None else H._f64(b)
    cond = x.abs() @ W.abs().t() + b.abs()
    if _wrong == "k":
        x = x.clone()
        x[:, x.shape[1] // 2] = 0
    elif _wrong == "segment":
        assert x2 is not None and x2.shape[1] >= 16
        k1 = x1.shape[1]
        x = x.clone()
        x[:, k1 - 16:k1] = H._f64(x2)[:, :16]
    else:
        assert _wrong in (None, "bias_after_relu", "transposed"), _wrong
    pre = x @ W.t() + b
    y = pre.clamp_min(0.0) if relu else pre
    if _wrong == "bias_after_relu":
        y = (x @ W.t()).clamp_min(0.0) + b if relu else pre
    if _wrong == "transposed":
        y = y.t().contiguous().view(y.shape)
    return pre, y, cond


def nt_gate(y, _wrong=None):
    """The ReLU bits of a stored output: y > 0 (so +0.0 and -0.0 are clear).  _wrong="gate": read as y >= 0."""
    return y >= 0 if _wrong == "gate" else y > 0


def nt_bwd_ref(dy, Wt, u, v, bits, _wrong=None):
    """fp64 (dx, cond): dx = (dy @ Wt.T + u v^T) * bit, cond = |dy| @ |Wt|.T + |u||v|, both zero where the bit is
    clear.  u [m] and v [n] (both or neither), bits bool [m][n] or None.  _wrong: "k" one k left out,
    "transposed"; a gate read as >= 0 is nt_gate's switch (the bits are this function's input)."""
    dy, Wt = H._f64(dy), H._f64(Wt)
    cond = dy.abs() @ Wt.abs().t()
    if _wrong == "k":
        dy = dy.clone()
        dy[:, dy.shape[1] // 2] = 0
    else:
        assert _wrong in (None, "transposed"), _wrong
    dx = dy @ Wt.t()
    if u is not None:
        r1 = H._f64(u).reshape(-1, 1) * H._f64(v).reshape(1, -1)
        dx, cond = dx + r1, cond + r1.abs()
    if bits is not None:
        dx, cond = dx * bits, cond * bits
    if _wrong == "transposed":
        dx = dx.t().contiguous().view(dx.shape)
    return dx, cond


def nt_ceiling(mode, K, cond, x, B):
    """The derived ceiling of |got - ref| per element of out = x @ B.T (+ the terms inside cond), per precision
    mode (include/nerf_hip.h, nerf_gemm_set_precision).  Every f32 accumulation is counted at 2 ulp of the
    condition sum, because the MFMA's internal rounding is not documented; 16 ulp cover the epilogue (bias or
    rank-one term, the unscale of mode 2, the second-order terms); 2^-149 is the grid of an f32 output below
    2^-126 (modes 0 and 1 work in f32's own exponent range).
      0  an f32 fma chain over K terms: K accumulations            -> (2 K + 16) 2^-24 cond + 2^-149
      1  three bf16 words per operand, exact for |x| >= 2^-110; six products per term into one f32
         accumulator: 6 K accumulations; the three dropped products (mid.lo, lo.mid, lo.lo) are <= 2^-26 |a||b|
         each (the header comment of csrc/gemm_x6.hip)             -> (12 K + 16) 2^-24 cond + 3 2^-26 cond + 2^-149
      2  helpers.pair_ceiling unchanged (3 K accumulations, two 11-bit words, the row-maximum floor).
    A condition, not a measurement."""
    if mode == 2:
        return H.pair_ceiling(K, cond, H._f64(x), H._f64(B))
    if mode == 0:
        return (2 * K + 16) * U24 * cond + H.F32_TINY
    assert mode == 1, mode
    return (12 * K + 16) * U24 * cond + 3 * 2.0 ** -26 * cond + H.F32_TINY


def nt_pair_emulate(x1, x2, W, r1, r2, b=None, relu=False, u=None, v=None, bits=None, _wrong=None):
    """The mode-2 arithmetic of the NT kernels on the CPU -> the output as f32: the row scale of [x1 | x2] from
    max(r1, r2) (ONE scale for both segments: a_rowmax in csrc/gemm.hpp; helpers.pair_exp), the weight's row
    exponents as helpers.pair_image_ref defines them (pair_row_exp), two fp16 words per operand, the three
    products hi.lo + lo.hi + hi.hi each as an f32 matmul and summed in f32 in that order, the scales undone
    (exact), then the epilogue in f32: + bias and ReLU, or + u v^T and the mask.
    _wrong="drop": the lo.hi product dropped."""
    x = _cat(x1, x2)
    Wd = H._f64(W)
    rm = r1.float() if r2 is None else torch.maximum(r1.float(), r2.float())
    ea = H.pair_exp(rm).unsqueeze(1)
    eb = H.pair_row_exp(W.detach().cpu().float()).unsqueeze(1)
    ah, al = H._pair_words(x, ea)
    bh, bl = H._pair_words(Wd, eb)
    f = lambda t: t.float()      # noqa: E731  (fp16 words and their 2^15-bounded sums are f32 values)
    acc = f(ah) @ f(bl).t()
    if _wrong != "drop":
        acc = acc + f(al) @ f(bh).t()
    acc = acc + f(ah) @ f(bh).t()
    out = (acc.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), -(ea + eb.t()).double())).float()
    if u is not None:
        out = out + u.float().reshape(-1, 1) * v.float().reshape(1, -1)
    if b is not None:
        out = out + b.float()
    if relu:
        out = out.clamp_min(0.0)
    if bits is not None:
        out = torch.where(bits, out, torch.zeros_like(out))
    return out


def nt_f32_emulate(x1, x2, W, b=None, relu=False, u=None, v=None, bits=None):
    """The same operation as a plain CPU f32 matmul with the f32 epilogue (the mode-0 arithmetic up to the
    summation order) -> f32."""
    x = _cat(x1, x2).float()
    out = x @ W.detach().cpu().float().t()
    if u is not None:
        out = out + u.float().reshape(-1, 1) * v.float().reshape(1, -1)
    if b is not None:
        out = out + b.float()
    if relu:
        out = out.clamp_min(0.0)
    if bits is not None:
        out = torch.where(bits, out, torch.zeros_like(out))
    return out


def _pm1(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def _exact_operands(m, n, K):
    """x [m][K] with two non-zeros per row: c1 = 1 + r // 256 at an even column ka, 2^12 at an odd column kb, both
    inside a 32-column block that moves with the row (two segments: either one); W [n][K] periodic in k with
    period 32, odd integers A = 2 (16 (n % 64) + k // 2) + 1 <= 2047 in the even columns, B = 1 + 16 (n // 64) +
    k // 2 <= 128 in the odd ones.  out[r][n] = c1 A + 4096 B < 2^20 decodes to (r, n) for r < 512, n < 512:
    c1 from the parity of out % 4096, (n % 64, r % 16) from A, (n // 64, r // 16 % 16) from B."""
    assert m <= 512 and n <= 512 and K % 32 == 0
    rows, blocks = torch.arange(m), K // 32
    ka = 32 * (rows % blocks) + 2 * (rows % 16)
    kb = 32 * ((rows // 2) % blocks) + 2 * ((rows // 16) % 16) + 1
    x = torch.zeros(m, K)
    x[rows, ka] = (1 + rows // 256).float()
    x[rows, kb] = 4096.0
    nn, k = torch.arange(n).unsqueeze(1), (torch.arange(K) % 32).unsqueeze(0)
    W = torch.where(k % 2 == 0, 2 * (16 * (nn % 64) + k // 2) + 1, 1 + 16 * (nn // 64) + k // 2).float()
    return x, W


def nt_inputs(kind, m, n, k1, k2, seed):
    """The operands of one forward call (x1 [m][k1], x2 [m][k2] or None, W [n][k1 + k2], b [n]) with their exact
    row maxima r1, r2, and -- for k2 == 0, where dy = x1 and wt = W make a backward call -- u [m], v [n] and the
    gate bits [m][n]; f32 CPU tensors in a namespace.
      generic   +-1 uniform activations, +-0.1 weights, +-0.5 bias, u and v +-1, half the bits set.
      spread    activation row r (and u[r]) scaled by 2^e, e cycling through helpers.CRAFT_EXPS; weight row j
                scaled by 2^8 (j even) or 2^-8; the bias live in every third column only, u in every second
                row, so the small rows are not drowned by an O(1) epilogue term.
      zeros     the last m / 128 rows all zero in both segments and in u (rmax = 0: the padding rows of a real
                batch); rows 8 .. 15 zero in x2 beside a live x1; weight rows 1 and n - 2 zero; bias and v zero in
                the columns 8 i + 5.  Forward: cond == 0 on (zero row, column 8 i + 5) only; backward (no bias):
                on the whole zero rows, 1 / 128 = 0.78 % of the elements -- under the 1 % cap of the tight kinds.
      segments  even rows: x1 at 2^-20, x2 at 2^10; odd rows the reverse (k2 == 0: the two halves of x1).  The
                kernel takes ONE scale per row for both segments.
      cancel    the second half of every segment is -(1 + 2^-12) times the first (rounded to f32) against equal
                weights, no bias, u, v at 2^-14: |ref| <= 2^-10 cond.
      gate      forward only.  Integer operands (x in {0..3}, w in {-2..2}), exact in every mode, and six gate
                columns whose weight row is a unit vector or zero:
                  column 0  w = +e_0, b = -1            pre = +0.0 in the rows with x[r][0] = 1 (r even)
                  column 1  w = +e_1, b = -(1 - 2^-24)  pre = +2^-24 in the rows with x[r][1] = 1 (r % 3 == 0)
                  column 2  w = -e_2, b = +(1 - 2^-24)  pre = -2^-24 in the rows with x[r][2] = 1 (r % 3 == 1)
                  column 3  w = 0,    b = -0.0          pre = +0.0 everywhere
                  column 4  w = 0,    b = +2^-149       pre = the smallest positive f32
                  column 5  w = 0,    b = -2^-149       pre = its negative
                2^-24 = 1 - pred(1) is the smallest non-zero |acc + bias| an integer accumulator can give against
                a bias near 1.  Left out: a pre-activation of -0.0.  No kernel of the family can produce one --
                every accumulator starts at +0.0, a round-to-nearest sum is -0.0 only when both terms are, so
                acc is never -0.0 and acc + bias never is; column 3 holds the nearest case, a bias of -0.0.
      exact     _exact_operands: x with 1 or 2 and 2^12 in a row, w integers <= 2047, bias (n % 7) 2^20, u = r % 5,
                v = (n % 3) 2^20: every operand has at most 11 significant bits (one fp16 word, two bf16 words),
                every product and partial sum is an integer below 2^24 -- exact in f32 and in both splits --
                and out[r][n] differs at every (r, n) (the epilogue terms sit above the GEMM's 20 bits).
    Domains: every kind keeps |x| >= 2^-110 or 0 (mode 1's limit, include/nerf_hip.h) -- the smallest non-zero
    operands are spread's 2^-60 rows; subnormal operands are left out for that reason, and because the f32 MFMA's
    treatment of them is not documented."""
    assert kind in NT_KINDS, kind
    g = torch.Generator().manual_seed(seed)
    K = k1 + k2
    x = _pm1(g, m, K)
    W = _pm1(g, n, K) * 0.1
    b = _pm1(g, n) * 0.5
    u, v = _pm1(g, m), _pm1(g, n)
    bits = torch.rand(m, n, generator=g) < 0.5
    rows, cols = torch.arange(m), torch.arange(n)
    if kind == "spread":
        s = 2.0 ** torch.tensor([H.CRAFT_EXPS[r % 6] for r in range(m)], dtype=torch.float32)
        x = x * s.unsqueeze(1)
        u = u * s * (rows % 2 == 0)
        W = W * torch.where(cols % 2 == 0, 2.0 ** 8, 2.0 ** -8).unsqueeze(1)
        b = b * (cols % 3 == 0)
    elif kind == "zeros":
        zr = list(range(m - m // 128, m))
        x[zr] = 0
        u[zr] = 0
        if k2:
            x[8:16, k1:] = 0
        W[1] = 0
        W[n - 2] = 0
        b[5::8] = 0
        v[5::8] = 0
    elif kind == "segments":
        ka = k1 if k2 else k1 // 2
        even = (rows % 2 == 0).unsqueeze(1)
        lo, hi = torch.tensor(2.0 ** -20), torch.tensor(2.0 ** 10)
        x[:, :ka] *= torch.where(even, lo, hi)
        x[:, ka:] *= torch.where(even, hi, lo)
    elif kind == "cancel":
        for a, w in ((0, k1),) + (((k1, k2),) if k2 else ()):
            h = w // 2
            x[:, a + h:a + w] = -(x[:, a:a + h] * (1 + 2.0 ** -12))
            W[:, a + h:a + w] = W[:, a:a + h]
        b = torch.zeros(n)
        u, v = u * 2.0 ** -14, v * 2.0 ** -14
    elif kind == "gate":
        x = torch.randint(0, 4, (m, K), generator=g).float()
        W = torch.randint(-2, 3, (n, K), generator=g).float()
        b = torch.randint(-3, 4, (n,), generator=g).float()
        x[:, 0] = (rows % 2 == 0).float()
        x[:, 1] = (rows % 3 == 0).float()
        x[:, 2] = (rows % 3 == 1).float()
        W[:6] = 0
        W[0, 0], W[1, 1], W[2, 2] = 1.0, 1.0, -1.0
        b[:6] = torch.tensor([-1.0, -(1 - EPS1), 1 - EPS1, -0.0, H.F32_TINY, -H.F32_TINY])
        u = v = bits = None
    elif kind == "exact":
        x, W = _exact_operands(m, n, K)      # two segments: the index rule puts a row's two non-zeros in either
        b = (cols % 7).float() * 2.0 ** 20
        u, v = (rows % 5).float(), (cols % 3).float() * 2.0 ** 20
    x, W, b = x.float().contiguous(), W.float().contiguous(), b.float().contiguous()
    x1 = x[:, :k1].contiguous()
    x2 = x[:, k1:].contiguous() if k2 else None
    if k2 or kind == "gate":
        u = v = bits = None
    return types.SimpleNamespace(kind=kind, m=m, n=n, k1=k1, k2=k2, x1=x1, x2=x2, W=W, b=b, r1=x1.abs().amax(1),
                                 r2=x2.abs().amax(1) if k2 else None, u=u, v=v, bits=bits)


def nt_gate_expect(inp):
    """The gate kind's expected entries -> (rows, column, pre-activation, bit) per gate column."""
    rows = torch.arange(inp.m)
    tiny = H.F32_TINY
    every = rows >= 0
    return ((rows % 2 == 0, 0, 0.0, False), (rows % 3 == 0, 1, EPS1, True), (rows % 3 == 1, 2, -EPS1, False),
            (every, 3, 0.0, False), (every, 4, tiny, True), (every, 5, -tiny, False))


def nt_hold(what, got, ref, cond, ceil, fails, exact=False):
    """The per-element check of one output against its fp64 reference, shared by the CPU and the GPU module:
    finite; |got - ref| <= ceil per element; exactly 0 where cond == 0; torch.equal for the exact kind.
    Failures go to `fails` -> max e = max |got - ref| / cond."""
    got = H._f64(got)
    if not bool(torch.isfinite(got).all()):
        fails.append(f"{what}: non-finite output")
        return float("inf")
    err = (got - ref).abs()
    e, nz = H.cond_error(got, ref, cond)
    ratio = err / ceil.clamp_min(1e-300)
    worst = ratio.max().item()
    if worst > 1.0:
        i = int(ratio.argmax())
        fails.append(f"{what}: element {divmod(i, got.shape[1])} is {worst:.3g} of its ceiling (max e {e / U24:.2f} ulp)")
    if nz:
        fails.append(f"{what}: {nz} non-zero outputs where the condition sum is 0")
    if exact and not torch.equal(got, ref):
        fails.append(f"{what}: the exact kind is not exact ({int((got != ref).sum())} elements differ)")
    return e
