"""The fused chain kernels (csrc/chain.hip) layer by layer against the fp64 reference of
tests/helpers.py, at edge rows (GPU only, GEMM precision mode 2, D = 256, three 128-row blocks).

Every layer's reference is taken from the kernel's own saved f32 output of the layer before it (and
its saved ReLU words), so each layer's error stands alone and no ReLU decision cascades;
|relu(a) - relu(b)| <= |a - b|, so no element is left out of a value comparison.

Error measure: e[m, n] = |got - ref| / cond[m, n] with cond the sum of the absolute products (and
|bias|); where cond = 0 the output must be exactly 0.  Two bars per layer:
  * the derived ceiling helpers.pair_ceiling (a condition from the arithmetic, not a measurement);
  * the tight bar max e_chain <= 1.5 max e_f32 + 4 ulp, e_f32 the same measure of the exact-f32
    per-layer kernel (precision mode 0) on the very same operands -- the bar of
    test_gpu_kernels.test_split_accuracy, which the per-layer pair kernel meets.
The ratios max e_chain / max e_f32 go through helpers.report_err and are tabled in DESIGN.md."""
import pytest
import torch

from model import _hip
from tests import helpers as H

pytestmark = pytest.mark.gpu

NP, NREAL = 384, 256
SENTINEL = -12345.5
_STATE = {}


def _mode(m):
    class _Ctx:
        def __enter__(self):
            self.old = _hip.gemm_get_precision()
            _hip.gemm_set_precision(m)

        def __exit__(self, *a):
            _hip.gemm_set_precision(self.old)
    return _Ctx()


def _forward_state(dev, variant):
    """Seeded field (helpers.chain_test_net), the crafted [384][64] encodings and what
    nerf_mlp_chain_train saved from them; computed once per parameter set and never modified."""
    if variant in _STATE:
        return _STATE[variant]
    net = H.chain_test_net(0, variant)
    params, heads = H.chain_params(net)
    net = net.to(dev)
    with _mode(2):
        runner = net.hip_runner()
        runner.pack()
        o, d = (t.to(dev) for t in H.chain_test_rays())
        view = (-d).contiguous()
        e = lambda *s: torch.full(s, SENTINEL, device=dev, dtype=torch.float32)      # noqa: E731
        z, ep, ed = e(NREAL), e(NREAL, 64), e(NREAL, 64)
        _hip.encode_samples(o, d, view, None, 5, 50, NREAL, 0.01, 10.0, z, ep, ed)
        torch.cuda.synchronize()
        assert bool((ep[250:] == 0).all()) and bool((ed[250:] == 0).all())      # real padding rows
        enc_p, enc_d = (t.to(dev) for t in H.chain_crafted_inputs(ep, ed, tiny=variant == "P1"))
        assert bool((enc_p[:, 63] == 0).all()) and bool((enc_d[:, 27:] == 0).all())      # the pad columns stay zero
        rp, rd = enc_p.abs().amax(1), enc_d.abs().amax(1)      # exact
        outs = [e(NP, l.out_p) for l in runner.layers]
        cmaxes = [e(NP // 128, l.out_p) if l.name != "lr" else None for l in runner.layers]
        masks = [torch.zeros(NP, l.out_p // 32, device=dev, dtype=torch.int32) if l.relu else None for l in runner.layers]
        raw4 = e(NP, 4)
        hd = (net.fc_density.weight, net.fc_density.bias, runner.wc, net.fc_rgb.bias)
        _hip.mlp_chain_train(enc_p, enc_d, rp, rd, NP, H.chain_descs(runner, outs, masks, cmaxes), *hd, raw4)
        torch.cuda.synchronize()
    st = dict(net=net, runner=runner, params=params, heads=heads, enc_p=enc_p, enc_d=enc_d, rp=rp, rd=rd, outs=outs,
              cmaxes=cmaxes, masks=masks, raw4=raw4, hd=hd)
    _STATE[variant] = st
    return st


def _seg2(st, l):
    return st["enc_p"] if l == 4 else st["enc_d"] if l == 9 else None


def _per_layer_fwd(st, l, x1, mode):
    """nerf_linear_fwd of layer l on (x1, its encoding segment): precision mode 0 (w_split None, the
    exact-f32 MFMA) or mode 2 (the per-layer fp16 pair kernel)."""
    runner = st["runner"]
    L = runner.layers[l]
    x2 = _seg2(st, l)
    y = torch.empty(NP, L.out_p, device=x1.device)
    with _mode(mode):
        _hip.linear_fwd(x1, L.k1, x2, 64 if x2 is not None else 0, runner.w[L.name], runner.bias(L), y, NP, L.out_p,
                        L.relu, w_split=runner.ws[L.name] if mode == 2 else None,
                        x1_rmax=x1.abs().amax(1) if mode == 2 else None,
                        x2_rmax=x2.abs().amax(1) if mode == 2 and x2 is not None else None)
        torch.cuda.synchronize()
    return y


def _check_layers(test, tag, st, outs, fails, rows=None):
    """Every layer output of one forward kernel against the fp64 reference of its own inputs; returns
    the e_f32 of each layer.  rows: the rows the bars apply to (None: all)."""
    e_f32s = []
    for l in range(10):
        x1 = st["enc_p"] if l == 0 else outs[l - 1]
        W, b = st["params"][l]
        pre, cond = H.chain_fwd_ref(l, x1, _seg2(st, l), W, b)
        ref = H.chain_act(l, pre)
        x, Wp = H.chain_fwd_operands(l, x1, _seg2(st, l), W)
        ceil = H.pair_ceiling(H.CHAIN_KPAD[l], cond, x, Wp)
        sel = slice(None) if rows is None else rows
        got = outs[l].cpu().double()
        assert torch.isfinite(got).all(), (tag, l)
        over = ((got - ref).abs() > ceil)[sel]
        e, nz = H.cond_error(got[sel], ref[sel], cond[sel])
        e0, _ = H.cond_error(_per_layer_fwd(st, l, x1, 0)[sel], ref[sel], cond[sel])
        e2, _ = H.cond_error(_per_layer_fwd(st, l, x1, 2)[sel], ref[sel], cond[sel])
        e_f32s.append(e0)
        ratio = H.report_err(test, f"{tag} {H.CHAIN_NAMES[l]} e_chain/e_f32", e / max(e0, 1e-300))
        print(f"{tag} {H.CHAIN_NAMES[l]}: e_chain {e / H.U24:.2f} ulp, e_f32 {e0 / H.U24:.2f} ulp, per-layer pair "
              f"{e2 / H.U24:.2f} ulp, ratio {ratio:.2f}, bar {H.tight_bar(e0) / H.U24:.2f} ulp; over the ceiling: "
              f"{int(over.sum())}; non-zero at cond = 0: {nz}")
        if bool(over.any()):
            fails.append(f"{tag} {H.CHAIN_NAMES[l]}: {int(over.sum())} elements over the derived ceiling")
        if nz:
            fails.append(f"{tag} {H.CHAIN_NAMES[l]}: {nz} non-zero outputs where cond = 0")
        if e > H.tight_bar(e0):
            fails.append(f"{tag} {H.CHAIN_NAMES[l]}: e_chain {e / H.U24:.2f} ulp > 1.5 x {e0 / H.U24:.2f} + 4 ulp")
    return e_f32s


def _check_heads(tag, st, outs, raw4, fails):
    wd, bd, wc, bc = st["heads"]
    h8, hr = outs[7].cpu().double(), outs[9].cpu().double()
    got = raw4.cpu().double()
    assert torch.isfinite(got).all(), tag
    ref_d, cond_d = h8 @ wd.t() + bd, h8.abs() @ wd.abs().t() + bd.abs()
    ref_c, cond_c = hr @ wc.t() + bc, hr.abs() @ wc.abs().t() + bc.abs()
    for name, g, r, c, n in (("sigma_raw", got[:, :1], ref_d, cond_d, 256), ("rgb logits", got[:, 1:], ref_c, cond_c, 128)):
        over = (g - r).abs() > H.dot_ceiling(n, c)
        e, nz = H.cond_error(g, r, c)
        print(f"{tag} {name}: e {e / H.U24:.2f} ulp against ({n} + 2) ulp; non-zero at cond = 0: {nz}")
        if bool(over.any()) or nz:
            fails.append(f"{tag} {name}: {int(over.sum())} over (n + 2) 2^-24 cond, {nz} non-zero at cond = 0")


def _check_words(tag, st, e_f32s, fails):
    """The training chain's ReLU words against its saved outputs and against the reference."""
    outs, masks = st["outs"], st["masks"]
    for l in range(10):
        if masks[l] is None:
            continue
        out = outs[l].cpu().double()
        bits = H.relu_bits(masks[l], out.shape[1])
        name = H.CHAIN_NAMES[l]
        if bool((bits & ~(out > 0)).any()):
            fails.append(f"{tag} {name}: a ReLU bit set on an output that is not positive")
        if l == 9:
            if not torch.equal(bits, out > 0):
                fails.append(f"{tag} {name}: the colour layer's bits differ from out > 0")
        else:
            # the two-wave chain takes the bit from the fp16 hi word of the next layer's A operand:
            # values below 2^-39 of the row maximum (the encoding l4 joins included) are consumed as 0
            M = out.amax(1, keepdim=True)
            if l == 3:
                M = torch.maximum(M, st["rp"].cpu().double().unsqueeze(1))
            miss = (out >= 2.0 ** -38 * M) & (out > 0) & ~bits
            if bool(miss.any()):
                fails.append(f"{tag} {name}: {int(miss.sum())} outputs >= 2^-38 of the row maximum without their bit")
        x1 = st["enc_p"] if l == 0 else outs[l - 1]
        pre, cond = H.chain_fwd_ref(l, x1, _seg2(st, l), *st["params"][l])
        # (cond = 0: the pre-activation is exactly 0 whatever the rounding, so its bit is compared too)
        clear = (pre.abs() > H.tight_bar(e_f32s[l]) * cond) | (cond == 0)
        share = 1.0 - clear.double().mean().item()
        wrong = int((bits != (pre > 0))[clear].sum())
        print(f"{tag} {name}: ReLU words: {wrong} wrong where |pre| clears the bar, {share:.4%} of the elements left out")
        if wrong:
            fails.append(f"{tag} {name}: {wrong} ReLU bits differ from the reference where |pre| > bar x cond")
        if share > 0.01:
            fails.append(f"{tag} {name}: {share:.2%} of the elements within the bar of zero (> 1 %)")


def _check_cmax(tag, st, fails):
    for l in range(9):
        want = st["outs"][l].abs().view(NP // 128, 128, -1).amax(1)
        if not torch.equal(st["cmaxes"][l], want):
            fails.append(f"{tag} {H.CHAIN_NAMES[l]}: cmax differs from amax |out| over the group's 128 rows in "
                         f"{int((st['cmaxes'][l] != want).sum())} places")


@pytest.mark.parametrize("variant", ["P1", "P2"])
def test_forward_chains_against_fp64(dev, variant):
    """nerf_mlp_chain_train (every out, ReLU word, cmax, raw4), nerf_mlp_chain_fwd (every out, the plain
    images) and nerf_mlp_chain_frozen (bit-identical to train) on the crafted rows.  P1: the biases as
    initialised except l2.bias = -1, so rows at a small scale are dead from l2 on; P2: every bias zero,
    so small rows stay small through all ten layers (without the 2^-118 rows)."""
    test = "test_forward_chains_against_fp64"
    st = _forward_state(dev, variant)
    runner, fails = st["runner"], []
    e_f32s = _check_layers(test, f"{variant} train", st, st["outs"], fails)
    _check_heads(f"{variant} train", st, st["outs"], st["raw4"], fails)
    _check_words(f"{variant} train", st, e_f32s, fails)
    _check_cmax(f"{variant} train", st, fails)
    # the one-wave eval chain, reading the plain images, every output stored
    with _mode(2):
        outs2 = [torch.full((NP, l.out_p), SENTINEL, device=dev) for l in runner.layers]
        _hip.mlp_chain_fwd(st["enc_p"], st["enc_d"], st["rp"], st["rd"], NP,
                           H.chain_descs(runner, outs2, [None] * 10, [None] * 10, plain=True))
        masks3 = [None if m is None else torch.zeros_like(m) for m in st["masks"]]
        raw4_3 = torch.full((NP, 4), SENTINEL, device=dev)
        _hip.mlp_chain_frozen(st["enc_p"], st["enc_d"], st["rp"], st["rd"], NP,
                              H.chain_descs(runner, [None] * 10, masks3, [None] * 10), *st["hd"], raw4_3)
        torch.cuda.synchronize()
    _check_layers(test, f"{variant} fwd", st, outs2, fails)
    if not torch.equal(raw4_3, st["raw4"]):
        fails.append(f"{variant}: nerf_mlp_chain_frozen's raw4 differs from nerf_mlp_chain_train's")
    for l, (a, b) in enumerate(zip(masks3, st["masks"])):
        if a is not None and not torch.equal(a, b):
            fails.append(f"{variant}: nerf_mlp_chain_frozen's ReLU words of {H.CHAIN_NAMES[l]} differ from train's")
    if variant == "P1":
        # conditions on the fp64 reference alone: dead rows (every l2 pre-activation < -0.5) and alive rows
        pres, _ = H.chain_compose_fwd(st["params"], st["heads"], st["enc_p"], st["enc_d"])
        dead, alive = (pres[2] < -0.5).all(1), (pres[2] > 0).any(1)
        assert int(dead.sum()) >= 8 and int(alive.sum()) >= 8, (int(dead.sum()), int(alive.sum()))
        o2 = st["outs"][2].cpu()[dead]
        if not bool((o2.view(torch.int32) == 0).all()):
            fails.append("P1: a dead row's l2 output is not bitwise +0")
        if not bool((st["masks"][2].cpu()[dead] == 0).all()):
            fails.append("P1: a dead row's l2 ReLU words are not 0")
        b3 = st["params"][3][1].clamp_min(0)      # l3 of a dead row: relu(bias), one rounding at most
        if not bool(((st["outs"][3].cpu().double()[dead] - b3).abs() <= 16 * H.U24 * b3).all()):
            fails.append("P1: a dead row's l3 output is not relu(bias)")
    else:
        zero = list(H.CRAFT["zero"]) + list(H.CRAFT["tiny"]) + list(range(250, 256))
        for l in range(10):      # homogeneous field: a zero row stays exactly zero
            if not bool((st["outs"][l][zero] == 0).all()):
                fails.append(f"P2: {H.CHAIN_NAMES[l]} of an all-zero row is not 0")
        if not bool((st["raw4"][zero] == 0).all()):
            fails.append("P2: raw4 of an all-zero row is not 0")
    assert not fails, "\n".join(fails)


def _per_layer_bwd(st, i, dy, graw4, mode):
    """nerf_linear_bwd_data producing D_i (i >= 1) from the saved D_{i-1}: mode 0 or mode 2."""
    runner = st["runner"]
    L = runner.layers[10 - i]
    mask = None if i == 1 else st["masks"][9 - i]
    dx = torch.empty(NP, 256, device=dy.device)
    with _mode(mode):
        kw = dict(u=graw4, ldu=4, v=runner.wd.view(-1)) if i == 2 else {}
        _hip.linear_bwd_data(dy, L.out_p, runner.wt[L.name][:256], dx, NP, 256, mask=mask,
                             wt_split=runner.wts[L.name][:, :, :256] if mode == 2 else None,
                             dy_rmax=dy.abs().amax(1) if mode == 2 else None, **kw)
        torch.cuda.synchronize()
    return dx


def test_backward_chains_against_fp64(dev):
    """nerf_mlp_chain_bwd on the P1 forward's ReLU words and a crafted graw4 (zero rows, sigma-only
    rows, rgb-only rows, rows 2^+-30 apart in one block): every D_i against fp64 from the saved
    D_{i-1}, dy_cmax / dy_rmax bitwise the maxima of the saved D_i, nerf_mlp_chain_bwd_rays
    bit-identical on D_0, D_5, D_9 and their row maxima."""
    test = "test_backward_chains_against_fp64"
    st = _forward_state(dev, "P1")
    runner, fails = st["runner"], []
    graw4 = H.chain_crafted_graw4().to(dev)
    e = lambda *s: torch.full(s, SENTINEL, device=dev, dtype=torch.float32)      # noqa: E731
    w = lambda i: 128 if i == 0 else 256                                          # noqa: E731
    dy = [e(NP, w(i)) for i in range(10)]
    cm = [e(NP // 128, w(i)) for i in range(10)]
    rm = [e(NP) for _ in range(10)]
    keep = (0, 5, 9)
    dy2 = [e(NP, w(i)) if i in keep else None for i in range(10)]
    rm2 = [e(NP) if i in keep else None for i in range(10)]
    with _mode(2):
        _hip.mlp_chain_bwd(H.chain_bwd_args(st, graw4, dy, cm, rm, e(512)))
        _hip.mlp_chain_bwd_rays(H.chain_bwd_args(st, graw4, dy2, [None] * 10, rm2, None))
        torch.cuda.synchronize()
    for i in keep:
        if not (torch.equal(dy2[i], dy[i]) and torch.equal(rm2[i], rm[i])):
            fails.append(f"nerf_mlp_chain_bwd_rays: D_{i} or its row maxima differ from nerf_mlp_chain_bwd's")
    wd, _, wc, _ = st["heads"]
    zero, sigma = list(H.GRAW["zero"]), list(H.GRAW["sigma"])
    for i in range(10):
        got = dy[i].cpu().double()
        assert torch.isfinite(got).all(), i
        bits = None if i == 1 else H.relu_bits(st["masks"][9 if i == 0 else 9 - i], w(i))
        W = None if i == 0 else st["params"][10 - i][0]
        ref, cond = H.chain_bwd_ref(i, dy[i - 1] if i else None, W, bits, graw4=graw4, wd=wd, wc=wc)
        e_c, nz = H.cond_error(got, ref, cond)
        if i == 0:
            over = (got - ref).abs() > H.dot_ceiling(3, cond)
            print(f"D_0: e {e_c / H.U24:.2f} ulp against (3 + 2) ulp; non-zero at cond = 0: {nz}")
        else:
            B = H.chain_bwd_weight(i, W)
            over = (got - ref).abs() > H.pair_ceiling(w(i - 1), cond, dy[i - 1].cpu().double(), B)
            e0, _ = H.cond_error(_per_layer_bwd(st, i, dy[i - 1], graw4, 0), ref, cond)
            e2, _ = H.cond_error(_per_layer_bwd(st, i, dy[i - 1], graw4, 2), ref, cond)
            ratio = H.report_err(test, f"bwd D_{i} e_chain/e_f32", e_c / max(e0, 1e-300))
            print(f"D_{i}: e_chain {e_c / H.U24:.2f} ulp, e_f32 {e0 / H.U24:.2f} ulp, per-layer pair {e2 / H.U24:.2f} ulp, "
                  f"ratio {ratio:.2f}, bar {H.tight_bar(e0) / H.U24:.2f} ulp; over the ceiling: {int(over.sum())}; "
                  f"non-zero at cond = 0: {nz}")
            if e_c > H.tight_bar(e0):
                fails.append(f"D_{i}: e_chain {e_c / H.U24:.2f} ulp > 1.5 x {e0 / H.U24:.2f} + 4 ulp")
        if bool(over.any()):
            fails.append(f"D_{i}: {int(over.sum())} elements over the derived ceiling")
        if nz:
            fails.append(f"D_{i}: {nz} non-zero outputs where cond = 0")
        # the maxima the weight-gradient and ray-gradient GEMMs scale by: bitwise those of the saved D_i
        if not torch.equal(rm[i], dy[i].abs().amax(1)):
            fails.append(f"dy_rmax[{i}] differs from the row maxima of the saved D_{i}")
        if not torch.equal(cm[i], dy[i].abs().view(NP // 128, 128, -1).amax(1)):
            fails.append(f"dy_cmax[{i}] differs from the column maxima of the saved D_{i}")
        if not (bool((dy[i][zero] == 0).all()) and bool((rm[i][zero] == 0).all())):
            fails.append(f"D_{i}: a row with zero graw4 is not exactly zero (or its rmax)")
    # sigma-only rows: nothing reaches the colour branch, and D_2 is the rank-one density term alone
    if not (bool((dy[0][sigma] == 0).all()) and bool((dy[1][sigma] == 0).all())):
        fails.append("a sigma-only row has a non-zero D_0 or D_1")
    r1 = graw4.cpu().double()[sigma, 0:1] * wd.reshape(1, -1) * H.relu_bits(st["masks"][7], 256)[sigma]
    assert bool((r1 != 0).any())
    if not bool(((dy[2].cpu().double()[sigma] - r1).abs() <= H.dot_ceiling(1, r1.abs())).all()):
        fails.append("a sigma-only row's D_2 is not d sigma x wd, masked")
    assert not fails, "\n".join(fails)
