"""Shared test fixtures: configs and seeded synthetic V_KITTI-shaped inputs."""
from __future__ import annotations

import torch

from model.synthetic import BASE_CFG, camera_K, make_cfg, rigid_c2w  # noqa: F401  (the package's builders)


def synthetic_rays(R=1024, S=128, H=188, W=621, seed=0, zero_frac=0.05, fx=362.5):
    """A V_KITTI-shaped batch: R random pixels of an HxW image, depth prior U[1,8] with
    some zeros (mask exercise), a fixed rigid pose, stratified noise U[0,1)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(H * W, generator=g)[:R]
    rows, cols = idx // W, idx % W
    px = 2.0 * cols.float() / (W - 1) - 1.0
    py = 2.0 * rows.float() / (H - 1) - 1.0
    pixels = torch.stack([px, py], -1).unsqueeze(0)
    depth = 1.0 + 7.0 * torch.rand(1, R, 1, generator=g)
    depth[torch.rand(1, R, 1, generator=g) < zero_frac] = 0.0
    c2w = rigid_c2w(seed)
    return {"pixels": pixels, "depth": depth, "K": camera_K(H, W, fx, fx), "c2w": c2w,
            "w2c": torch.inverse(c2w).unsqueeze(0), "scale": torch.eye(4).unsqueeze(0),
            "noise": torch.rand(1, R, S, generator=g), "ray_idx": idx}


# ---- parity bar (BASELINE.json north_star: 1e-4 rel on rendered RGB / depth) -----------
RENDER_RTOL = 1e-4     # elementwise, relative to the oracle value
RENDER_ATOL = 1e-6     # absolute floor for values near zero (dark pixels, masked depths)


def elementwise_excess(a, b, rtol=RENDER_RTOL, atol=RENDER_ATOL):
    """max over elements of |a - b| / (rtol |b| + atol): <= 1 passes the elementwise bar
    |a - b| <= rtol |b| + atol."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs() / (rtol * b.abs() + atol)).max().item()


def assert_elementwise(a, b, rtol=RENDER_RTOL, atol=RENDER_ATOL, what=""):
    """|a - b| <= rtol |b| + atol for every element; the message carries the worst element
    and, as a diagnostic, the max-normalised error max|a-b| / max|b|."""
    a_, b_ = a.detach().double().cpu(), b.detach().double().cpu()
    assert a_.shape == b_.shape, (what, a_.shape, b_.shape)
    err = (a_ - b_).abs()
    lim = rtol * b_.abs() + atol
    ratio = err / lim
    if ratio.numel() and ratio.max().item() > 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{what}: element {i}: |{a_.flatten()[i].item():.9g} - {b_.flatten()[i].item():.9g}| = "
                             f"{err.flatten()[i].item():.3g} > {rtol:g}*|b| + {atol:g} "
                             f"(max-normalised error {(err.max() / b_.abs().max().clamp_min(1e-30)).item():.3g})")


def report_err(test: str, name: str, err: float) -> float:
    """Observed parity error of one checked quantity, appended to $NERF_ERR_REPORT (one JSON
    line each) when set -- the survey the gradient tolerances are set from; returns err."""
    import json
    import os
    path = os.environ.get("NERF_ERR_REPORT")
    if path:
        from model import _hip
        with open(path, "a") as f:
            f.write(json.dumps({"test": test, "name": name, "err": float(err),
                                "mode": _hip.gemm_get_precision()}) + "\n")
    return err


# ---- the fused chain kernels (csrc/chain.hip): shared builders ---------------------------
CHAIN_R0, CHAIN_S0, CHAIN_NP = 12, 32, 384        # kernel level: three 128-row blocks
CHAIN_NAMES = ("l0", "l1", "l2", "l3", "l4", "l5", "l6", "l7", "lf", "lr")


def chain_descs(runner, outs, masks, cmaxes, plain=False):
    """The ten nerf_chain_layer descriptors over a packed FieldRunner: the chain images
    (nerf_mlp_chain_train / _frozen) or, plain=True, the plain ones (nerf_mlp_chain_fwd)."""
    from model import _hip
    descs = []
    for i, l in enumerate(runner.layers):
        ws = (runner.ws if plain else runner.wsc)[l.name]
        P = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        descs.append(_hip.ChainLayer(ws.data_ptr(), ws.shape[2], runner.bias(l).data_ptr(), P(outs[i]), l.out_p,
                                     P(masks[i]), l.out_p // 32, P(cmaxes[i])))
    return descs


def chain_kernel_state(dev):
    """Seeded D = 256 field, encodings of 12 rays x 32 samples, and nerf_mlp_chain_train's saves."""
    import model as mdl
    from model import _hip
    from torch.nn import functional as F
    R0, S0, NP = CHAIN_R0, CHAIN_S0, CHAIN_NP
    torch.manual_seed(7)
    net = mdl.OfficialStaticNerf(make_cfg(hidden=256, S=S0)).to(dev)
    runner = net.hip_runner()
    runner.pack()
    g = torch.Generator().manual_seed(8)
    o = ((torch.rand(R0, 3, generator=g) - 0.5) * 4).to(dev)
    d = F.normalize(torch.rand(R0, 3, generator=g) - 0.5, dim=-1).to(dev)
    view = (-d).contiguous()
    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)      # noqa: E731
    z, enc_p, enc_d, rp, rd = e(NP), e(NP, 64), e(NP, 64), e(NP), e(NP)
    cp, cd = e(NP // 128, 64), e(NP // 128, 64)
    _hip.encode_samples(o, d, view, None, R0, S0, NP, 0.01, 10.0, z, enc_p, enc_d, enc_p_rmax=rp, enc_d_rmax=rd,
                        enc_p_cmax=cp, enc_d_cmax=cd)
    m = net
    heads = (m.fc_density.weight, m.fc_density.bias, runner.wc, m.fc_rgb.bias)
    new_masks = lambda: [torch.zeros(NP, l.out_p // 32, device=dev, dtype=torch.int32) if l.relu else None    # noqa: E731
                         for l in runner.layers]
    outs = [e(NP, l.out_p) for l in runner.layers]
    cmaxes = [e(NP // 128, l.out_p) if l.name != "lr" else None for l in runner.layers]
    masks, raw4 = new_masks(), e(NP, 4)
    _hip.mlp_chain_train(enc_p, enc_d, rp, rd, NP, chain_descs(runner, outs, masks, cmaxes), *heads, raw4)
    torch.cuda.synchronize()
    return dict(net=net, runner=runner, o=o, d=d, view=view, z=z, enc_p=enc_p, enc_d=enc_d, rp=rp, rd=rd, cp=cp, cd=cd,
                heads=heads, outs=outs, cmaxes=cmaxes, masks=masks, raw4=raw4, new_masks=new_masks)


def chain_bwd_args(k, graw4, dy, cm, rm, scratch):
    """nerf_chain_bwd over a state with runner and masks (the ten layers' ReLU words, lf's None)."""
    from model import _hip
    runner = k["runner"]
    names = [l.name for l in runner.layers]
    c = _hip.ChainBwd()
    c.graw4, c.hr_mask, c.ld_hr_mask = graw4.data_ptr(), k["masks"][9].data_ptr(), 4
    c.wd, c.wc = runner.wd.data_ptr(), runner.wc.data_ptr()
    for i in range(9):
        l = 9 - i
        c.wt_img[i] = runner.wtsc[names[l]].data_ptr()
        c.wt_img_rows[i] = runner.layers[l].kp
        c.in_mask[i] = None if i == 0 else k["masks"][l - 1].data_ptr()
        c.ld_in_mask[i] = 8
    for i in range(10):
        c.dy[i] = None if dy[i] is None else dy[i].data_ptr()
        c.lddy[i] = 128 if i == 0 else 256
        c.dy_cmax[i] = None if cm[i] is None else cm[i].data_ptr()
        c.dy_rmax[i] = None if rm[i] is None else rm[i].data_ptr()
    c.scratch = None if scratch is None else scratch.data_ptr()
    c.n_pad = graw4.shape[0]
    return c


# ---- fp64 layer reference of the chain kernels (plain torch on the CPU) ---------------------
# Forward layers 0..9 = l0..l7, lf, lr (official_nerf.py:60-91): l4 reads [h3 | enc_p], lr reads
# [f | enc_d], ReLU on every layer except lf.  Backward: D_0 = the colour layer's output gradient,
# D_i (i >= 1) the gradient at the output (pre-activation) of forward layer 9 - i; the kernel's
# layer i (include/nerf_hip.h) produces D_{i+1}.
U24 = 2.0 ** -24
CHAIN_KPAD = (64, 256, 256, 256, 320, 256, 256, 256, 256, 320)


def chain_relu(layer: int) -> bool:
    return layer != 8


def relu_bits(words, n: int):
    """ReLU words [m][>= n/32] (int32) -> bool [m][n]: bit b of word w is column 32 w + b."""
    w = words.detach().cpu().long() & 0xffffffff
    return ((w.unsqueeze(-1) >> torch.arange(32)) & 1).reshape(w.shape[0], -1)[:, :n].bool()


def _f64(t):
    return t.detach().cpu().double()


def _pad_cols(W, k):
    W = _f64(W)
    return W if W.shape[1] == k else torch.cat([W, W.new_zeros(W.shape[0], k - W.shape[1])], 1)


def chain_fwd_operands(layer: int, x1, x2, W):
    """(x, Wp) in fp64: x = [x1 | x2] as the kernel reads it (the 64-wide padded encodings), Wp the
    reference weight [out][in] zero-padded to x's columns (the pad columns of the packed weight)."""
    assert (x2 is not None) == (layer in (4, 9)), layer
    x = _f64(x1) if x2 is None else torch.cat([_f64(x1), _f64(x2)], 1)
    return x, _pad_cols(W, x.shape[1])


def chain_fwd_ref(layer: int, x1, x2, W, b):
    """fp64 pre-activation x @ W.T + b of forward layer `layer` and its condition sum
    cond[m, n] = sum_k |x[m, k]| |W[n, k]| + |b[n]|."""
    x, Wp = chain_fwd_operands(layer, x1, x2, W)
    b = _f64(b)
    return x @ Wp.t() + b, x.abs() @ Wp.abs().t() + b.abs()


def chain_act(layer: int, pre):
    return pre.clamp_min(0.0) if chain_relu(layer) else pre


def chain_bwd_weight(i: int, W):
    """The B operand [256][k] of D_i = D_{i-1} @ B.T (i >= 1): the transpose of the forward weight
    of layer 10 - i restricted to its first 256 input columns (l4, lr: without the encoding)."""
    return _f64(W)[:, :256].t().contiguous()


def chain_bwd_ref(i: int, d_prev=None, W=None, bits=None, graw4=None, wd=None, wc=None):
    """fp64 D_i and its condition sum.
    D_0[m, j] = (sum_c graw4[m, 1 + c] wc[c, j]) bit(hr mask);   D_1 = D_0 W_lr[:, :256] (no mask);
    D_2 = (D_1 W_lf + graw4[:, 0] (x) wd) bit(l7 mask);   D_i = (D_{i-1} W_{l(10-i)}[:, :256]) bit(l(9-i) mask).
    W: the forward weight [out][in] of layer 10 - i; bits: bool [m][width] (relu_bits) or None."""
    if i == 0:
        g, wc = _f64(graw4)[:, 1:4], _f64(wc)[:, :128]
        val, cond = g @ wc, g.abs() @ wc.abs()
    else:
        d, B = _f64(d_prev), chain_bwd_weight(i, W)
        val, cond = d @ B.t(), d.abs() @ B.abs().t()
        if i == 2:
            r1 = _f64(graw4)[:, 0:1] * _f64(wd).reshape(1, -1)
            val, cond = val + r1, cond + r1.abs()
    assert (bits is None) == (i == 1), i
    if bits is not None:
        val, cond = val * bits, cond * bits
    return val, cond


def chain_params(net):
    """[(W, b)] of the ten layers and (wd, bd, wc, bc), fp64 on the CPU, reference layout."""
    lin = [net.layers0[0], net.layers0[2], net.layers0[4], net.layers0[6], net.layers1[0], net.layers1[2],
           net.layers1[4], net.layers1[6], net.fc_feature, net.rgb_layers[0]]
    heads = (net.fc_density.weight, net.fc_density.bias, net.fc_rgb.weight, net.fc_rgb.bias)
    return [(_f64(m.weight), _f64(m.bias)) for m in lin], tuple(_f64(t) for t in heads)


def chain_compose_fwd(params, heads, enc_p, enc_d):
    """The ten reference layers composed in fp64, each fed its own output -> (pre [10], raw4)."""
    wd, bd, wc, bc = heads
    pres, x = [], _f64(enc_p)
    for l, (W, b) in enumerate(params):
        x2 = _f64(enc_p) if l == 4 else _f64(enc_d) if l == 9 else None
        pre, _ = chain_fwd_ref(l, x, x2, W, b)
        pres.append(pre)
        x = chain_act(l, pre)
    h8 = chain_act(7, pres[7])
    raw4 = torch.cat([h8 @ wd.t() + bd, x @ wc.t() + bc], 1)
    return pres, raw4


def chain_compose_bwd(params, heads, pres, graw4):
    """D_0 .. D_9 composed in fp64 from the composed forward's ReLU decisions (pre > 0)."""
    wd, _, wc, _ = heads
    D = [chain_bwd_ref(0, graw4=graw4, wc=wc, bits=pres[9] > 0)[0]]
    for i in range(1, 10):
        bits = None if i == 1 else pres[9 - i] > 0
        D.append(chain_bwd_ref(i, D[-1], params[10 - i][0], bits, graw4=graw4, wd=wd)[0])
    return D


def cond_error(got, ref, cond):
    """e = |got - ref| / cond where cond > 0 -> (max e, number of non-zero outputs where cond == 0)."""
    got, ref = _f64(got), _f64(ref)
    pos = cond > 0
    e = ((got - ref).abs()[pos] / cond[pos]).max().item() if bool(pos.any()) else 0.0
    return e, int((got[~pos] != 0).sum())


def pair_ceiling(K: int, cond, x, B):
    """The derived ceiling of a row-scaled fp16 pair GEMM out = x @ B.T (+ terms inside cond) with f32
    accumulation: (6 K + 16) 2^-24 cond + 2^-37 (rowmax|x[m]| sum_k |B[n,k]| + rowmax|B[n]| sum_k |x[m,k]|).
    Each operand is (hi + lo) 2^-e with |x 2^e - hi - lo| <= 2^-22 |x 2^e| (two 11-bit words) or,
    where lo falls below fp16's smallest denormal 2^-24 at a row maximum below 2^15, 2^-39 of the
    row maximum; the dropped lo.lo product is <= 2^-22 |x||B|; the three products are 3 K f32
    accumulations, counted at 2 ulp each because the MFMA's internal rounding is not documented;
    16 ulp cover the epilogue (unscale, bias, rank-one term).  A condition, not a measurement."""
    x, B = x.abs(), B.abs()
    floor = x.amax(1, keepdim=True) * B.sum(1).unsqueeze(0) + x.sum(1, keepdim=True) * B.amax(1).unsqueeze(0)
    return (6 * K + 16) * U24 * cond + 2.0 ** -37 * floor


def dot_ceiling(n: int, cond):
    """A plain f32 dot product of n terms (the heads, D_0): (n + 2) 2^-24 cond."""
    return (n + 2) * U24 * cond


def tight_bar(e_f32: float) -> float:
    """The bar of test_split_accuracy: 1.5 x the exact-f32 kernel's error on the same operands + 4 ulp."""
    return 1.5 * e_f32 + 4 * U24


CRAFT_EXPS = (-60, -30, -8, 0, 8, 30)
CRAFT = dict(scaled=range(256, 362), zero=range(362, 370), p_zero=range(370, 374), d_zero=range(374, 378),
             single=range(378, 382), tiny=range(382, 384))
GRAW = dict(zero=tuple(range(250, 256)) + tuple(range(362, 370)) + tuple(range(30, 38)), sigma=range(10, 18),
            rgb=range(20, 28), scaled=tuple(range(128, 250)) + tuple(range(256, 362)))


def chain_crafted_inputs(enc_p, enc_d, tiny=True):
    """[256][64] encodings (rows 250..255 padding) -> [384][64]: rows 256..383 crafted from real rows
    by exact operations (CRAFT): scaled by 2^j, j cycling over CRAFT_EXPS; all-zero; enc_p zero only;
    enc_d zero only; a single non-zero element; two rows at 2^-118 (zero when tiny is False)."""
    enc_p, enc_d = enc_p.detach().cpu().float(), enc_d.detach().cpu().float()
    assert enc_p.shape == (256, 64) and enc_d.shape == (256, 64)
    src = [(7 * t) % 250 for t in range(128)]
    p, d = enc_p[src].clone(), enc_d[src].clone()
    for t in range(128):
        r = 256 + t
        if r in CRAFT["scaled"]:
            s = 2.0 ** CRAFT_EXPS[t % 6]
            p[t] *= s
            d[t] *= s
        elif r in CRAFT["zero"] or (r in CRAFT["tiny"] and not tiny):
            p[t] = 0
            d[t] = 0
        elif r in CRAFT["p_zero"]:
            p[t] = 0
        elif r in CRAFT["d_zero"]:
            d[t] = 0
        elif r in CRAFT["single"]:
            in_p = t % 2 == 0
            c = (6, 7, 45, 20)[r - 378]
            keep = (p if in_p else d)[t, c].clone()
            assert keep != 0
            p[t] = 0
            d[t] = 0
            (p if in_p else d)[t, c] = keep
        else:
            p[t] *= 2.0 ** -118
            d[t] *= 2.0 ** -118
    return torch.cat([enc_p, p]), torch.cat([enc_d, d])


def chain_crafted_graw4(seed=12):
    """[384][4] N(0, 1) upstream gradient with the rows of GRAW: zero rows (the padding, the all-zero
    crafted rows, eight real rows), sigma-only rows, rgb-only rows, rows scaled by 2^j."""
    g = torch.randn(384, 4, generator=torch.Generator().manual_seed(seed))
    for n, r in enumerate(GRAW["scaled"]):
        g[r] *= 2.0 ** CRAFT_EXPS[(5 * n + n // 6) % 6]
    g[list(GRAW["zero"])] = 0
    g[list(GRAW["sigma"]), 1:] = 0
    g[list(GRAW["rgb"]), 0] = 0
    return g


def chain_test_net(seed=0, variant="P1"):
    """The D = 256 field of the fp64 chain tests on the CPU: weights spread row-wise as
    tests/test_gpu_chain._net (logspace -1..1); P1: the biases as initialised except l2.bias = -1
    (rows at a small scale are dead from l2 on), P2: every bias zero (positively homogeneous)."""
    import model as mdl
    torch.manual_seed(seed)
    net = mdl.OfficialStaticNerf(make_cfg(hidden=256, S=50))
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            if p.dim() == 2:
                p.mul_(torch.logspace(-1, 1, p.shape[0]).unsqueeze(1) * (0.5 + 0.1 * i))
        if variant == "P1":
            net.layers0[4].bias.fill_(-1.0)
        else:
            for p in net.parameters():
                if p.dim() == 1:
                    p.zero_()
    return net


def chain_test_rays(R=5, seed=3):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(R, 3, generator=g) - 0.5) * 4
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=g) - 0.5, dim=-1)
    return o, d


# ---- the per-ray kernels (csrc/render.hip, misc.hip): fp64 references and edge inputs ----------
# Sample counts of tests/test_gpu_ray_kernels_fp64.py: the 16-lanes-per-ray composite family
# (S <= 256: every J arm, S == 16 J, a partial last lane, both sides of S % 4) and the wave-per-ray
# family (256 < S <= 1024).
COMPOSITE_S16 = (1, 2, 15, 16, 17, 31, 32, 33, 34, 36, 63, 64, 65, 100, 127, 128, 129, 132, 255, 256)
COMPOSITE_SWAVE = (257, 511, 512, 513, 1000, 1023, 1024)
COMPOSITE_R = 37
COMPOSITE_KINDS = ("generic", "saturated")
COMPOSITE_T = dict(rgb=1e-5, dist=1e-4, alpha=1e-5)      # the fixed bars of test_composite_fwd_bwd
COMPOSITE_T_GRAD = 2e-4                                   # times max(1, max |ref|)
F32_MARGIN = 4.0                                          # |hip - f64| <= T_project + F32_MARGIN E_f32


def composite_ref(raw, z, flags, g_rgb, g_dist, dtype):
    """The composite and its backward in plain torch at `dtype`: density activation (ReLU or
    softplus; 1 - exp(-sigma) unless dist_alpha), colour sigmoid, oracle.composite, autograd of
    sum(rgb g_rgb) + sum(dist g_dist).  raw [R*S][4], z [R][S] -> (rgb [R][3], dist [R],
    alpha [R][S], graw [R*S][4]).  float64: the reference; float32: the reference's own arithmetic."""
    from oracle import nerf_oracle as orc
    R, S = z.shape
    rr = raw.detach().cpu().to(dtype).clone().requires_grad_(True)
    zz = z.detach().cpu().to(dtype)
    sig = torch.relu(rr[:, 0]) if flags & 4 else torch.nn.functional.softplus(rr[:, 0])
    if not flags & 1:
        sig = 1 - torch.exp(-sig)
    c = torch.sigmoid(rr[:, 1:])
    rgb, dist, alpha, _ = orc.composite(sig.view(R, S), c.view(R, S, 3), zz, dist_alpha=bool(flags & 1),
                                        white_background=bool(flags & 2))
    loss = (rgb * g_rgb.detach().cpu().to(dtype)).sum() + (dist * g_dist.detach().cpu().to(dtype)).sum()
    loss.backward()
    return rgb.detach(), dist.detach(), alpha.detach(), rr.grad


def composite_edge_inputs(R, S, seed, kind):
    """(raw [R*S][4], z [R][S], g_rgb [R][3], g_dist [R]) in f32.  "generic": the distribution of
    test_composite_fwd_bwd (randn * 2, density logit + 0.5, depths sorted in [0.01, 9.01]).
    "saturated": ray r takes pattern r % 6 on top of it -- 0: density logit -30 everywhere (an empty
    ray); 1: +30 from sample S/3 on (softplus' x > 20 branch, alpha = 1: the transmittance runs
    through eps^k and underflows in f32); 2: alternating +25 / -25; 3: colour logits +-40; 4: density
    logit exactly 0 on the first half (the ReLU kink); 5: for S > 2, samples 1 .. S/2 at one repeated
    depth (dist_alpha's delta = 0).  Rays 7, 19, 31, ... carry a zero upstream gradient."""
    assert kind in COMPOSITE_KINDS, kind
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(R, S, 4, generator=g) * 2
    raw[:, :, 0] += 0.5
    z = torch.sort(torch.rand(R, S, generator=g) * 9 + 0.01, dim=1)[0]
    g_rgb = torch.randn(R, 3, generator=g)
    g_dist = torch.randn(R, generator=g) * 0.1
    g_rgb[7::12] = 0
    g_dist[7::12] = 0
    if kind == "saturated":
        i = torch.arange(S)
        for r in range(R):
            p = r % 6
            if p == 0:
                raw[r, :, 0] = -30.0
            elif p == 1:
                raw[r, S // 3:, 0] = 30.0
            elif p == 2:
                raw[r, :, 0] = torch.where(i % 2 == 0, 25.0, -25.0)
            elif p == 3:
                raw[r, :, 1:] = torch.where((i[:, None] + torch.arange(3)[None, :]) % 2 == 0, 40.0, -40.0)
            elif p == 4:
                raw[r, :(S + 1) // 2, 0] = 0.0
            elif S > 2:
                z[r, 1:S // 2 + 1] = z[r, S // 2].clone()
    return raw.reshape(R * S, 4).contiguous(), z.contiguous(), g_rgb, g_dist


def composite_refs(raw, z, flags, g_rgb, g_dist):
    """(the f64 reference, E_f32): E_f32[name] = max |f32 reference - f64 reference| of rgb, dist,
    alpha and grad on these very inputs -- the reference's own rounding, the yardstick of the bar."""
    names = ("rgb", "dist", "alpha", "grad")
    r64 = dict(zip(names, composite_ref(raw, z, flags, g_rgb, g_dist, torch.float64)))
    r32 = composite_ref(raw, z, flags, g_rgb, g_dist, torch.float32)
    e32 = {n: (t.double() - r64[n]).abs().max().item() for n, t in zip(names, r32)}
    return r64, e32


def f32_bar(t_project: float, e_f32: float) -> float:
    """The bar of the per-ray kernel tests: T_project + 4 E_f32.  T_project is the fixed tolerance
    the suite already holds that quantity to; E_f32 the plain f32 reference's own error against
    fp64 on the same inputs.  The factor covers the hardware exp / log / rcp of the 16-lane kernels
    (a few ulp each against libm's sub-ulp), the scan-tree order of the transmittance product and
    the butterfly order of the sums: a margin, not a measurement."""
    return t_project + F32_MARGIN * e_f32


def lattice_points(n, seed, lo=0, hi=4):
    """[3][n] f32 points on the integer lattice {lo .. hi-1}^3: every squared distance is exact in
    f32, so nearest-neighbour ties are exact ties."""
    return torch.randint(lo, hi, (3, n), generator=torch.Generator().manual_seed(seed)).float()


# ---- guarded outputs of the kernel tests ---------------------------------------------------------
SENT = 1234.5      # float sentinel (finite: a stray read of it shows as a wrong value, not a NaN)
GUARD = 64         # elements before and after the payload (payload 16-byte aligned, nerf_hip.h)


class Guarded:
    """A tensor of `shape` inside a sentinel-filled buffer; the payload starts sentinel-filled too."""

    def __init__(self, shape, dev, dtype=torch.float32, fill=SENT):
        import math
        n = math.prod(shape)
        self.buf = torch.full((2 * GUARD + n,), fill, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        self.fill = fill
        assert self.t.data_ptr() % 16 == 0

    def intact(self) -> bool:
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[-GUARD:] == self.fill).all())

    def untouched(self) -> bool:
        return bool((self.buf == self.fill).all())


# ---- the image-pair kernels (csrc/pair.hip): staged fp64 reference and inputs ------------------------
# The operations of nerf_pair_forward / _backward (include/nerf_hip.h) in plain torch at a dtype, in
# stages, so that a discontinuous choice is never compared across precisions: the points; the
# neighbours of given points; the losses and gradients with nn, valid and bad given; the decisions
# with their distance to the threshold.  An input set is a dict of f32 CPU tensors: h, w, d1 [P],
# d2 [P], K [4][4], Rt [4][4], s1 [1] or None, img1 / img2 [3][h][w] or None, nl.
PAIR_NL = 0.01
PAIR_SHAPES = ((2, 2), (3, 85), (2, 128), (2, 129), (19, 27), (3, 300), (47, 155))
PAIR_LARGE = (2, 8193)          # P > 2^14: fixed-point scale 2^47, 15 chunks of five 256-point tiles
PAIR_CAMERAS = ("diag", "principal", "skew")
PAIR_GAP = 1e-5                 # relative gap below which a neighbour choice is not compared
PAIR_D_VALID, PAIR_D_BAD = 1e-5, 1e-6    # no point this close to the validity / the nearest-limit threshold
PAIR_D_CELL, PAIR_D_SIGN = 5e-7, 1e-6    # nor to a bilinear cell edge (in [-1, 1] units), nor |img1 - img2| to 0
PAIR_COMBOS = dict(both=(1.0, 0.7), pc=(1.0, None), rgbs=(None, 0.7))
PAIR_T_ELEM = 2.0 ** -23        # x max |ref|: X, Y, g_d1, g_d2 per element
PAIR_T_G13 = 1e-6               # x the condition sum: every entry of g13
# seeds of the generic sets; a set whose default seed (1000 h + w) breaks a condition of
# pair_assert_conditions has another one here
PAIR_SEEDS = {(3, 85, "principal"): 103085, (2, 128, "diag"): 202128, (19, 27, "principal"): 119027,
              (3, 300, "principal"): 303300, (47, 155, "diag"): 247155, (47, 155, "principal"): 747155,
              (47, 155, "skew"): 2547155, (47, 155, "many"): 54}


def pair_camera(kind, h, w):
    """[4][4] camera of the pair tests: |K00| = |K11| = 1.5 at every aspect ("diag"), with a principal
    point, with skew, and "full": every entry of K[:3] non-zero (inverse4's pivoting, K[2][c] and
    K[r][3] in the reprojection and its gradient, the translation column of inv(K))."""
    K = camera_K(4 * h, 4 * w, 3.0 * w, 3.0 * h)[0].clone()
    if kind in ("principal", "full"):
        K[0, 2], K[1, 2] = 0.1, -0.07
    if kind in ("skew", "full"):
        K[0, 1] = 0.2
    if kind == "full":
        K[1, 0], K[2, 0], K[2, 1] = 0.05, 0.02, -0.03
        K[0, 3], K[1, 3], K[2, 3] = 0.01, -0.02, 0.03
    assert kind in PAIR_CAMERAS + ("full",), kind
    return K


def pair_pose(t=(0.05, -0.02, 0.3), r=(0.05, -0.03, 0.02)):
    """Rt [4][4]: a small rotation about a general axis (Rodrigues), the translation of test_gpu_pair."""
    r = torch.tensor(r, dtype=torch.float64)
    th = r.norm()
    k = r / th
    Kx = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    Rt = torch.eye(4, dtype=torch.float64)
    Rt[:3, :3] = torch.eye(3, dtype=torch.float64) + torch.sin(th) * Kx + (1 - torch.cos(th)) * (Kx @ Kx)
    Rt[:3, 3] = torch.tensor(t, dtype=torch.float64)
    return Rt.float()


def pair_generic_inputs(h, w, camera="diag", with_img=True, with_scale=True, seed=None):
    """Depths in [2, 5], the small rotation, s1 = 1.3, random images."""
    seed = PAIR_SEEDS.get((h, w, camera), 1000 * h + w) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    P = h * w
    d1, d2 = 2.0 + 3.0 * torch.rand(P, generator=g), 2.0 + 3.0 * torch.rand(P, generator=g)
    img1 = torch.rand(3, h, w, generator=g) if with_img else None
    img2 = torch.rand(3, h, w, generator=g) if with_img else None
    return dict(h=h, w=w, d1=d1, d2=d2, K=pair_camera(camera, h, w), Rt=pair_pose(),
                s1=torch.tensor([1.3]) if with_scale else None, img1=img1, img2=img2, nl=PAIR_NL)


def pair_large_inputs():
    """2x8193 without images.  The pose is a tenth of the generic one: two rows of 8193 points are two
    dense lines, and a query 0.3 away from the other cloud's line is nearly equidistant from many of its
    points (0.23 % of the queries within a relative gap of 1e-5 at the generic pose, 1 of 16386 here)."""
    inp = pair_generic_inputs(*PAIR_LARGE, "diag", with_img=False)
    inp["Rt"] = pair_pose(t=(0.005, -0.002, 0.03), r=(0.005, -0.003, 0.002))
    return inp


def _pair_cast(inp, dtype):
    return {k: (v.detach().cpu().to(dtype) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _pair_pixels(h, w, dtype):
    from oracle import nerf_oracle as orc
    return orc.arange_pixels(h, w, dtype=dtype)[1][0]


def _pair_unproject(pix, d, Kinv):
    """transform_to_world: (inv(K) [x d, y d, d, 1])[:3], [P][3]."""
    hom = torch.stack([pix[:, 0] * d, pix[:, 1] * d, d, torch.ones_like(d)], 1)
    return (hom @ Kinv.t())[:, :3]


def pair_points(inp, dtype):
    """pc1, pc2, X = R (pc1 / s1) + t, Y = pc2 / s1, each [P][3] at dtype."""
    c = _pair_cast(inp, dtype)
    pix = _pair_pixels(c["h"], c["w"], dtype)
    Kinv = torch.linalg.inv(c["K"])
    pc1, pc2 = _pair_unproject(pix, c["d1"], Kinv), _pair_unproject(pix, c["d2"], Kinv)
    s = 1.0 if c["s1"] is None else c["s1"]
    return dict(pc1=pc1, pc2=pc2, X=(pc1 / s) @ c["Rt"][:3, :3].t() + c["Rt"][:3, 3], Y=pc2 / s)


def pair_dist64(Q, R, idx):
    """fp64 |Q_i - R_idx(i)| in the summation order of pair_neighbours."""
    Q, R = Q.detach().cpu().double(), R.detach().cpu().double()[idx.long()]
    d = Q - R
    return ((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2).sqrt()


def pair_dist32(Q, R, idx):
    """The kernel's f32 distance expression (k_nn_part: every operation rounded, no contraction)."""
    d = Q.detach().cpu().float() - R.detach().cpu().float()[idx.long()]
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sqrt()


def pair_neighbours(Q, R, block=512, device=None):
    """Neighbours of the queries Q [P][3] among R [P'][3] as given, in fp64, in row blocks (no P x P'
    matrix is held): (best distance, first index attaining it, relative gap to the best distance at
    any other index; 0 on an exact tie).  device: where the reduction runs (torch, float64)."""
    dev = torch.device("cpu") if device is None else device
    Q, R = Q.detach().to(dev, torch.float64), R.detach().to(dev, torch.float64)
    rx, ry, rz = R[:, 0][None], R[:, 1][None], R[:, 2][None]
    best, first, second = [], [], []
    for i0 in range(0, Q.shape[0], block):
        q = Q[i0:i0 + block]
        D = (((q[:, 0:1] - rx) ** 2 + (q[:, 1:2] - ry) ** 2) + (q[:, 2:3] - rz) ** 2).sqrt_()
        b, f = D.min(1)
        D.scatter_(1, f[:, None], float("inf"))
        best.append(b)
        first.append(f)
        second.append(D.min(1).values)
    best, first, second = torch.cat(best).cpu(), torch.cat(first).cpu(), torch.cat(second).cpu()
    gap = torch.where(second == best, torch.zeros_like(best), (second - best) / best)
    return best, first, gap


def pair_decisions(inp, dtype=torch.float64):
    """The decisions of the reprojection (in fp64 unless a dtype is given) with their distance to the threshold: bad (-q_z
    against nl), valid (max(|p_x|, |p_y|) against 1); for valid unclamped points the distance of p to
    the nearest bilinear cell edge of img2 (the sample's gradient jumps there) and min |img1 - img2|
    (the sign of the difference).  Without images: no rgb_s term, nothing valid."""
    from oracle import nerf_oracle as orc
    c = _pair_cast(inp, dtype)
    h, w, P = c["h"], c["w"], c["h"] * c["w"]
    pts = pair_points(inp, dtype)
    q = pts["pc1"] @ c["Rt"][:3, :3].t() + c["Rt"][:3, 3]
    m_bad = -q[:, 2] - c["nl"]
    bad = m_bad < 0
    q = torch.where(bad[:, None], torch.full_like(q, c["nl"]), q)
    h3 = q @ c["K"][:3, :3].t() + c["K"][:3, 3]
    p = h3[:, :2] / h3[:, 2:]
    mx = p.abs().amax(1)
    valid = mx <= 1
    out = dict(bad=bad, valid=valid, d_bad=m_bad.abs(), d_valid=(mx - 1).abs(), p=p, d_cell=float("inf"),
               d_sign=float("inf"))
    if c["img1"] is None:
        out["valid"] = torch.zeros(P, dtype=torch.bool)
        return out
    live = valid & ~bad
    if bool(live.any()):
        ij = (p[live] + 1) * 0.5 * torch.tensor([w - 1, h - 1], dtype=dtype)
        out["d_cell"] = ((ij - ij.round()).abs() * 2 / torch.tensor([w - 1, h - 1], dtype=dtype)).min().item()
        pix = _pair_pixels(h, w, dtype)
        e = orc.grid_values(c["img1"][None], pix[None])[0] - orc.grid_values(c["img2"][None], p[None])[0]
        out["d_sign"] = e[live].abs().min().item()
    return out


def pair_assert_conditions(inp, dec=None):
    """The conditions under which the kernel's f32 decisions are the fp64 ones (ISSUE section 3)."""
    dec = pair_decisions(inp) if dec is None else dec
    if inp["img1"] is None:
        return dec
    assert dec["d_valid"].min().item() >= PAIR_D_VALID, ("validity threshold", dec["d_valid"].min().item())
    assert dec["d_bad"].min().item() >= PAIR_D_BAD, ("nearest-limit threshold", dec["d_bad"].min().item())
    assert dec["d_cell"] >= PAIR_D_CELL, ("bilinear cell edge", dec["d_cell"])
    assert dec["d_sign"] >= PAIR_D_SIGN, ("sign of img1 - img2", dec["d_sign"])
    return dec


def pair_loss_ref(inp, nn, valid, bad, go_pc=1.0, go_rgbs=None, detach=False, dtype=torch.float64, _wrong=None):
    """go_pc (mean |X - Y[a]| + mean |Y - X[b]|) + go_rgbs rgb_s with nn = (a, b) [2][P], valid and bad
    given, and its autograd at dtype; R, t and s1 are expanded to per-point leaves, so g13 = {dR, dt,
    ds1} is the sum of the per-point gradients and cond13 the sum of their absolute values.
    detach: rgbs_detach_scale (pc1 of the reprojection carries no gradient).  A weight of None leaves
    its term out.  _wrong: the wrong kernels of tests/test_pair_reference_cpu.py, nothing else."""
    from oracle import nerf_oracle as orc
    c = _pair_cast(inp, dtype)
    h, w, P = c["h"], c["w"], c["h"] * c["w"]
    leaf = lambda t: t.clone().requires_grad_(True)      # noqa: E731
    d1, d2 = leaf(c["d1"]), leaf(c["d2"])
    Rp, tp = leaf(c["Rt"][:3, :3].expand(P, 3, 3)), leaf(c["Rt"][:3, 3].expand(P, 3))
    sp = leaf((torch.ones(1, dtype=dtype) if c["s1"] is None else c["s1"]).expand(P, 1))      # NULL: ds1 at s1 = 1
    pix = _pair_pixels(h, w, dtype)
    Kinv = torch.linalg.inv(c["K"])
    pc1, pc2 = _pair_unproject(pix, d1, Kinv), _pair_unproject(pix, d2, Kinv)
    X = torch.einsum("pij,pj->pi", Rp, pc1 / sp) + tp
    Y = pc2 / sp
    a, b = nn[0].long(), nn[1].long()
    Ya = Y[a]
    if _wrong == "dropped_term":                         # one scattered term missing
        Ya = torch.where((torch.arange(P) == P // 2)[:, None], Ya.detach(), Ya)
    pc = torch.linalg.norm(X - Ya, dim=1).mean() + torch.linalg.norm(Y - X[b], dim=1).mean()
    total = torch.zeros((), dtype=dtype)
    if go_pc is not None:
        total = total + go_pc * pc
    rgb_s = torch.zeros((), dtype=dtype)
    if c["img1"] is not None:
        K3 = c["K"][:3]
        pr = pc1.detach() if (detach and _wrong != "scale_attached") else pc1
        q = torch.einsum("pij,pj->pi", Rp, pr) + tp
        nlq = torch.full_like(q, c["nl"])
        q = torch.where(bad[:, None], nlq + (q - q.detach()) if _wrong == "clamped_gradient" else nlq, q)
        h3 = q @ K3[:, :3].t() + K3[:, 3]
        if _wrong == "diagonal_K":                       # the gradient as if K were diagonal
            hd = q * torch.diagonal(K3[:, :3])
            h3 = hd + (h3 - hd).detach()
        p_re = h3[:, :2] / h3[:, 2:]
        rgb1 = orc.grid_values(c["img1"][None], pix[None])
        rgb2 = orc.grid_values(c["img2"][None], p_re[None])
        rgb_s = orc.rgb_s_loss_ref(rgb1.view(1, h, w, 3), rgb2.view(1, h, w, 3), valid.view(1, h, w, 1))
        if go_rgbs is not None:
            total = total + go_rgbs * rgb_s
    if total.requires_grad:
        total.backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    gR, gt = z(Rp), z(tp)
    gs = z(sp)
    g13 = torch.cat([gR.sum(0).reshape(9), gt.sum(0), gs.sum().reshape(1)])
    cond13 = torch.cat([gR.abs().sum(0).reshape(9), gt.abs().sum(0), gs.abs().sum().reshape(1)])
    return dict(pc=pc.detach(), rgb_s=rgb_s.detach(), g_d1=z(d1), g_d2=z(d2), g13=g13, cond13=cond13, gR_pp=gR, gt_pp=gt)


class PairRef:
    """The checks of one input set, shared by the GPU module (the kernels' outputs) and the CPU module
    (a torch-f32 emulation and its wrong variants).  Bars: |got - f64| <= T + 4 E_f32 (f32_bar), E_f32
    the max-norm error of the f32 run of the staged reference against its f64 run on the same inputs,
    nn, valid and bad.  worst[name]: the largest |got - f64| / (T + E_f32) seen."""

    def __init__(self, inp, device=None, generic=True):
        self.inp, self.P, self.device, self.generic = inp, inp["h"] * inp["w"], device, generic
        self.with_img = inp["img1"] is not None
        self.pts64, self.pts32 = pair_points(inp, torch.float64), pair_points(inp, torch.float32)
        self.dec = pair_assert_conditions(inp)
        self.worst = {}
        self._refs = {}

    def bar(self, name, got, r64, r32, T, where):
        got, r32 = got.detach().cpu().double().reshape(r64.shape), r32.double()
        assert bool(torch.isfinite(got).all()), f"{where}: {name} not finite"
        e32 = (r32 - r64).abs().max().item() if r64.numel() else 0.0
        err = (got - r64).abs()
        T = torch.as_tensor(T, dtype=torch.float64).expand_as(err)
        lim = T + F32_MARGIN * e32
        den = T + e32
        ratio = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
        r = ratio.max().item() if ratio.numel() else 0.0
        self.worst[name] = max(self.worst.get(name, 0.0), r)
        print(f"{where} {name}: |got-f64| {err.max().item():.3e}  E_f32 {e32:.3e}  T {T.max().item():.3e}  ratio {r:.3f}")
        bad = (err > lim).nonzero().flatten()
        assert bad.numel() == 0, (f"{where}: {name}: {bad.numel()} elements over the bar, first {bad[:4].tolist()}: "
                                  f"|got - f64| = {err.flatten()[bad[:4]].tolist()} > T + 4 * {e32:.3e} "
                                  f"= {lim.flatten()[bad[:4]].tolist()}")

    def check_points(self, X, Y, where=""):
        for name, got in (("X", X), ("Y", Y)):
            r64 = self.pts64[name]
            self.bar(name, got, r64, self.pts32[name], PAIR_T_ELEM * r64.abs().max().item(), where)

    def check_nn(self, X, Y, nn, where=""):
        """nn [2][P] against the fp64 neighbours of the very points X, Y -> per direction (best, first, gap)."""
        P, out = self.P, []
        nn = nn.detach().cpu().view(2, P).long()
        assert bool(((nn >= 0) & (nn < P)).all()), f"{where}: nn outside [0, P)"
        for z, (Q, R) in enumerate(((X, Y), (Y, X))):
            best, first, gap = pair_neighbours(Q, R, device=self.device)
            d = pair_dist64(Q, R, nn[z])
            worse = (d > best * (1 + PAIR_GAP)).nonzero().flatten()
            assert worse.numel() == 0, (f"{where}: direction {z}: {worse.numel()} queries with a neighbour farther than "
                                        f"the best, first {worse[:4].tolist()}")
            strict = gap > PAIR_GAP
            wrong = (strict & (nn[z] != first)).nonzero().flatten()
            assert wrong.numel() == 0, (f"{where}: direction {z}: {wrong.numel()} wrong neighbours, first at "
                                        f"{wrong[:4].tolist()}: {nn[z][wrong[:4]].tolist()} vs {first[wrong[:4]].tolist()}")
            if self.generic:
                assert int((~strict).sum()) <= 1e-3 * P, f"{where}: direction {z}: {int((~strict).sum())} near-ties"
            out.append((best, first, gap))
        return out

    def refs(self, nn, combo, detach):
        """(f64, f32) runs of the staged reference with this nn."""
        nn = nn.detach().cpu().view(2, self.P).long()
        key = (combo, bool(detach), hash(nn.numpy().tobytes()))
        if key not in self._refs:
            go_pc, go_rgbs = PAIR_COMBOS[combo]
            self._refs[key] = tuple(pair_loss_ref(self.inp, nn, self.dec["valid"], self.dec["bad"], go_pc, go_rgbs, detach, dt)
                                    for dt in (torch.float64, torch.float32))
        return self._refs[key]

    def check_out3(self, out3, nn, where=""):
        out3 = out3.detach().cpu()
        r64, r32 = self.refs(nn, "both" if self.with_img else "pc", False)
        self.bar("out3[0]", out3[0], r64["pc"], r32["pc"], 1e-5 * r64["pc"].abs().item(), where)
        self.bar("out3[1]", out3[1], r64["rgb_s"], r32["rgb_s"], 1e-5 * r64["rgb_s"].abs().item() + 1e-7, where)
        n_valid = int(self.dec["valid"].sum())
        assert out3[2].item() == 3.0 * n_valid, f"{where}: out3[2] = {out3[2].item()} with {n_valid} valid points"
        if not self.with_img or n_valid == 0:
            assert out3[1].item() == 0.0, f"{where}: rgb_s without a valid point"

    def check_grads(self, g, nn, combo, detach, where=""):
        """g: dict(g_d1 [P], g_d2 [P], g13 [13]) of one backward."""
        r64, r32 = self.refs(nn, combo, detach)
        where = f"{where} {combo} detach={int(detach)}"
        for name in ("g_d1", "g_d2"):
            self.bar(name, g[name], r64[name], r32[name], PAIR_T_ELEM * r64[name].abs().max().item(), where)
        g13 = g["g13"].detach().cpu()
        for name, sl in (("dR", slice(0, 9)), ("dt", slice(9, 12)), ("ds1", slice(12, 13))):
            self.bar(name, g13[sl], r64["g13"][sl], r32["g13"][sl], PAIR_T_G13 * r64["cond13"][sl], where)
        if combo == "rgbs":
            assert bool((g["g_d2"].detach().cpu() == 0).all()), f"{where}: g_d2 from rgb_s alone"
            live = self.dec["valid"] & ~self.dec["bad"]
            dead = ~live
            if not detach:
                assert bool((g["g_d1"].detach().cpu()[dead] == 0).all()), f"{where}: g_d1 of an invalid or clamped point"
            else:
                assert bool((g["g_d1"].detach().cpu() == 0).all()), f"{where}: g_d1 through a detached scale"
                if bool(live.any()):
                    assert g13[:9].abs().max().item() > 0 and g13[9:12].abs().max().item() > 0, f"{where}: dR, dt"
            assert g13[12].item() == 0.0, f"{where}: ds1 from rgb_s alone"
            if not bool(live.any()):
                assert bool((g13 == 0).all()) and bool((g["g_d1"].detach().cpu() == 0).all()), f"{where}: nothing valid"

    def report(self, test):
        for name, r in self.worst.items():
            report_err(test, name, r)


# ---- crafted input sets of the pair tests ------------------------------------------------------------
def pair_tie_inputs(case):
    """Exact nearest-neighbour ties (diagonal K, Rt the identity, no scale, no images) -> (inputs,
    tied X queries, the first index each must return).
    "chunks" 3x300: d2 equal in rows 0 and 2 per column, row 1 far: every query of X's row 1 (y = 0) is
    equidistant from Y[c'] and Y[2w + c'], which lie in different chunks (k_nn_final).
    "tile" 3x129 and "tiles" 2x8193 (w - 1 a power of two: x(c) = -x(w - 1 - c) exactly): Y is far
    except columns c0 and w - 1 - c0 of row 0 at one depth; the centre-column queries (x = 0) are
    equidistant from both -- inside one 256-point tile (40, 88), and in two tiles of the chunk
    3840..5119 (3896, 4296)."""
    h, w = dict(chunks=(3, 300), tile=(3, 129), tiles=PAIR_LARGE)[case]
    g = torch.Generator().manual_seed(41 + h * w)
    d1 = 2.0 + 3.0 * torch.rand(h, w, generator=g)
    if case == "chunks":
        row = 2.0 + 3.0 * torch.rand(w, generator=g)
        d2 = torch.stack([row, torch.full((w,), 50.0), row])
        tied = torch.arange(w, 2 * w)
        first = None                                     # the reference's first index, < w
    else:
        c0 = 40 if case == "tile" else 3896
        d2 = 1000.0 + 50.0 * torch.rand(h, w, generator=g)
        d2[0, c0] = d2[0, w - 1 - c0] = 3.0
        tied = torch.arange(h) * w + (w - 1) // 2
        first = torch.full((h,), c0)
    inp = dict(h=h, w=w, d1=d1.reshape(-1), d2=d2.reshape(-1), K=pair_camera("diag", h, w), Rt=torch.eye(4), s1=None,
               img1=None, img2=None, nl=PAIR_NL)
    return inp, tied, first


def pair_assert_ties(X, Y, tied, first_want, neigh):
    """The premise of a tie case on the points X, Y as given: every query of `tied` has an exact tie
    (fp64 gap 0, and the f32 distance expression of the kernel bitwise equal at two indices at least);
    -> the first index of each."""
    best, first, gap = neigh
    assert tied.numel() >= 1
    assert bool((gap[tied] == 0).all()), "a tie is not exact in fp64"
    Xq, Yr = X.detach().cpu().float()[tied], Y.detach().cpu().float()
    d = Xq[:, None, :] - Yr[None, :, :]
    D = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).sqrt()
    n_min = (D == D.min(1, keepdim=True).values).sum(1)
    assert bool((n_min >= 2).all()), "a tie is not exact in the f32 expression"
    assert torch.equal(D.argmin(1), first[tied]), "f32 and fp64 disagree on the first index"
    if first_want is not None:
        assert torch.equal(first[tied], first_want)
    return first[tied]


def pair_many_to_one_inputs(h, w):
    """d2 about 1e3 except one pixel near the X cloud: every X query chooses it (P scattered terms on one
    point).  Generic d1, pose and scale; images at 47x155, none at the large shape."""
    inp = pair_generic_inputs(h, w, "diag", with_img=(h, w) != PAIR_LARGE, seed=PAIR_SEEDS.get((h, w, "many"), 7 + h))
    g = torch.Generator().manual_seed(h + w)
    hot = (h // 2) * w + w // 2
    inp["d2"] = 1000.0 + 50.0 * torch.rand(h * w, generator=g)
    inp["d2"][hot] = 3.5
    return inp, hot


def pair_coincident_inputs():
    """19x27, Rt the identity, no scale, no images, d1 == d2 on the patch rows 5..10 x columns 5..15:
    X_i == Y_i there (distance 0: the d > 0 branches) -> (inputs, patch indices)."""
    h, w = 19, 27
    inp = pair_generic_inputs(h, w, "diag", with_img=False, with_scale=False, seed=77)
    inp["Rt"] = torch.eye(4)
    m = torch.zeros(h, w, dtype=torch.bool)
    m[5:11, 5:16] = True
    patch = m.reshape(-1).nonzero().flatten()
    inp["d2"][patch] = inp["d1"][patch]
    return inp, patch


def pair_clamped_inputs():
    """19x27 (P = 513) with |K00| = |K11| = 0.8 and d1 = nl on the first 256 points (the whole first
    workgroup): rotated and translated they lie behind the camera (bad), and (nl, nl, nl) projects to
    (-0.8, 0.8): valid.  The forward counts them, the backward gives them nothing."""
    h, w = 19, 27
    inp = pair_generic_inputs(h, w, "diag", seed=PAIR_SEEDS.get("clamped", 91))
    inp["K"] = camera_K(h, w, 0.4 * w, 0.4 * h)[0].clone()
    inp["d1"][:256] = PAIR_NL
    return inp, torch.arange(256)


def pair_no_valid_inputs():
    """12x17: a sideways translation puts every projection outside [-1, 1]."""
    inp = pair_generic_inputs(12, 17, "diag", seed=12)
    inp["Rt"] = pair_pose(t=(20.0, -0.02, 0.3))
    return inp


def pair_input_sets():
    """Every input set of tests/test_gpu_pair_fp64.py with images or a decision in it: (name, inputs)."""
    for h, w in PAIR_SHAPES:
        for cam in PAIR_CAMERAS:
            yield f"{h}x{w}-{cam}", pair_generic_inputs(h, w, cam)
    for h, w in ((19, 27), (3, 85)):
        yield f"{h}x{w}-full", pair_generic_inputs(h, w, "full")
    yield "large", pair_large_inputs()
    for case in ("chunks", "tile", "tiles"):
        yield f"tie-{case}", pair_tie_inputs(case)[0]
    yield "many-47x155", pair_many_to_one_inputs(47, 155)[0]
    yield "many-large", pair_many_to_one_inputs(*PAIR_LARGE)[0]
    yield "coincident", pair_coincident_inputs()[0]
    yield "clamped", pair_clamped_inputs()[0]
    yield "no-valid", pair_no_valid_inputs()


# ---- the prologue, loss, Adam and pack kernels (csrc/rays.hip, misc.hip): references and inputs ------
# Plain numpy / torch at a given dtype, written from the text of include/nerf_hip.h and the reference
# lines it cites.  Each *_refs helper returns the fp64 run and E_f32, the f32 run's own distance to it on
# the same inputs.  _wrong=...: the wrong kernels of tests/test_prologue_reference_cpu.py, nothing else.
SAMPLE_CASES = ((2, 2, 1), (2, 3, 3), (33, 62, 1023), (32, 64, 1024), (41, 50, 1025), (2, 2049, 2049),
                (90, 91, 4095), (64, 128, 4096), (188, 621, 1024))          # (H, W, R)
SAMPLE_SEED = 20240611
SAMPLE_MAX_ROUNDS_USED = 20
MAT4_BATCHES = (1, 63, 64, 65, 130)
POSE_R_SCALES = (0.0, 1e-25, 1e-7, 1e-3, 0.7, 3.141592653589793 - 1e-3, 4.0)
POSE_AXIS = (0.48, -0.6, 0.64)                      # a unit vector
AFFINE_N = (1, 63, 1023, 1024, 1025, 65536, 65537, 66600)
CAMERA_R = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)
LOSS_SHAPES = ((1, 1), (21, 21), (22, 22), (341, 341), (342, 342), (1025, 1025), (5, 40), (40, 5))     # (R, n_depth)
LOSS_MASKS = ("none", "all", "one", "zero")
ADAM_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 524288, 524292, 524293, 525315)
ADAM_HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
T_VALUE, T_GRAD = 1e-5, 1e-4                        # the fixed tolerances of tests/test_gpu_rays.py


def tree_ceiling(n: int, threads: int) -> float:
    """The derived ceiling, as a multiple of sum |term|, of an f32 sum of n terms taken as per-thread
    serial sums of ceil(n / threads) terms, a 6-step wave butterfly and a 16-term serial tail, each
    addition one rounding, with 4 roundings for forming a term: (ceil(n / threads) + 26) 2^-24.
    A derivation, not a measurement."""
    return (-(-n // threads) + 26) * U24


def max_bar(t_rel: float, ref, e_f32: float) -> float:
    """t_rel max|ref| + 4 E_f32 (f32_bar with the project tolerance relative to the largest entry)."""
    return f32_bar(t_rel * (ref.abs().max().item() if ref.numel() else 0.0), e_f32)


def assert_max_bar(name, got, r64, e_f32, t_rel, where="", worst=None, finite=None):
    """|got - f64| <= t_rel max|ref| + 4 E_f32 over the elements of `finite` (default: all, and then
    got must be finite everywhere); records |got - f64| / (T + E_f32) in worst[name]."""
    got, r64 = got.detach().cpu().double().reshape(r64.shape), r64.double()
    if finite is None:
        assert bool(torch.isfinite(got).all()), f"{where}: {name} not finite"
        finite = torch.ones_like(r64, dtype=torch.bool)
    rf = r64[finite]
    T = t_rel * (rf.abs().max().item() if rf.numel() else 0.0)
    err = (got[finite] - rf).abs().max().item() if rf.numel() else 0.0
    assert err == err, f"{where}: {name} is NaN where the reference is finite"
    ratio = err / (T + e_f32) if T + e_f32 > 0 else (0.0 if err == 0 else float("inf"))
    if worst is not None:
        worst[name] = max(worst.get(name, (0.0, 0.0))[0], ratio), max(worst.get(name, (0.0, 0.0))[1], e_f32)
    print(f"{where} {name}: |got-f64| {err:.3e}  E_f32 {e_f32:.3e}  T {T:.3e}  ratio {ratio:.3f}")
    assert err <= f32_bar(T, e_f32), f"{where}: {name}: |got - f64| = {err:.3e} > {T:.3e} + 4 * {e_f32:.3e}"


def assert_sum_bar(name, got, ref, cond, ceiling, e_f32=0.0, where="", worst=None):
    """|got - ref| <= ceiling cond + 4 E_f32 per entry (cond = sum |term| of the entry's fp64 terms)."""
    got, ref, cond = got.detach().cpu().double().reshape(-1), ref.double().reshape(-1), cond.double().reshape(-1)
    assert bool(torch.isfinite(got).all()), f"{where}: {name} not finite"
    err, lim = (got - ref).abs(), ceiling * cond + F32_MARGIN * e_f32
    den = ceiling * cond + e_f32
    ratio = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double()).max().item()
    if worst is not None:
        worst[name] = max(worst.get(name, (0.0, 0.0))[0], ratio), max(worst.get(name, (0.0, 0.0))[1], e_f32)
    print(f"{where} {name}: |got-f64| {err.max().item():.3e}  bar {lim.max().item():.3e}  ratio {ratio:.3f}")
    assert bool((err <= lim).all()), f"{where}: {name}: |got - f64| = {err.tolist()[:16]} > {lim.tolist()[:16]}"


def _e32(r32, r64, names):
    return {n: ((r32[n].double() - r64[n].double()).abs().max().item() if r64[n] is not None and r64[n].numel() else 0.0)
            for n in names}


# ---- the ray sampler -----------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox-4x32-10 (Salmon et al., SC'11) in numpy: counter [..., 4], key [..., 2] (uint32 values)
    -> [..., 4] uint32.  One round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2, c = (hi1 ^ c1 ^ k0, lo1,
    hi0 ^ c3 ^ k1, lo0), then the key is bumped by the Weyl constants."""
    import numpy as np
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c0, c1, c2, c3 = (c[..., i] & mask for i in range(4))
    k0, k1 = np.broadcast_to(k[..., 0], c0.shape) & mask, np.broadcast_to(k[..., 1], c0.shape) & mask
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # < 2^64: both factors are below 2^32
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def sample_key(seed: int, counter=None):
    """The Philox key of nerf_sample_rays: the two halves of the seed, xored with the two halves of
    (counter + 1) 0x9E3779B97F4A7C15 mod 2^64 when a seed_counter is given."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    if counter is not None:
        m = ((counter + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        k0, k1 = k0 ^ (m & 0xFFFFFFFF), k1 ^ (m >> 32)
    return k0, k1


def sample_rays_ref(n_pix, R, seed, counter=None, _wrong=None):
    """The draw rule of nerf_sample_rays (include/nerf_hip.h): in round k every pending slot s draws
    v = floor(u n / 2^64), u the first two words (first the high one) of Philox at counter (s, k,
    0x5a4d, 0); a value belongs to the smallest (round, slot) that drew it, every other drawer draws
    again -> (idx int64 [R], rounds)."""
    import numpy as np
    key = np.array(sample_key(seed, counter), dtype=np.uint64)
    idx = np.full(R, -1, dtype=np.int64)
    owned = set()
    pending = np.arange(R, dtype=np.uint64)
    rounds = 0
    while pending.size:
        assert rounds < 64, "sample_rays_ref: 64 rounds did not suffice"
        ctr = np.stack([pending, np.full_like(pending, rounds), np.full_like(pending, 0x5a4d), np.zeros_like(pending)], -1)
        w = philox4x32_10(ctr, key).astype(np.uint64)
        hi, lo, n = w[:, 0], w[:, 1], np.uint64(n_pix)
        v = (hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)      # floor(((hi 2^32 + lo) n) / 2^64), n < 2^31
        again = []
        order = zip(pending.tolist(), v.tolist())
        if _wrong == "larger_slot_wins":
            order = reversed(list(order))
        for s, val in order:
            if val in owned:
                again.append(s)
            else:
                owned.add(val)
                idx[s] = val
        pending = np.array(sorted(again), dtype=np.uint64)
        rounds += 1
    return torch.from_numpy(idx), rounds


def pixels_ref(idx, height, width, dtype=torch.float32):
    """arange_pixels at the drawn indices (common.py:36-39): (2 col / (W - 1) - 1, 2 row / (H - 1) - 1), [R][2]."""
    idx = idx.long()
    col, row = (idx % width).to(dtype), (idx // width).to(dtype)
    return torch.stack([2.0 * col / (width - 1) - 1.0, 2.0 * row / (height - 1) - 1.0], -1)


# ---- the 4x4 chain ------------------------------------------------------------------------------------------
def mat4_edge_batch(n, seed=0):
    """[n][4][4] f32: well-conditioned random matrices with, cycling over the batch, rigid poses, a
    permutation matrix (a pivot swap in every column), a zero leading pivot and one matrix with an entry
    set so that cond is about 1e5 -> (matrices, dict of the indices of each kind)."""
    g = torch.Generator().manual_seed(100 + seed + n)
    A = torch.randn(n, 4, 4, generator=g) + 3 * torch.eye(4)
    kinds = dict(rigid=[], perm=[], zero_pivot=[], ill=[])
    P = torch.zeros(4, 4)
    P[0, 1] = P[1, 2] = P[2, 3] = P[3, 0] = 1.0
    for i in range(n):
        k = i % 8 if n > 1 else 2
        if k == 0:
            A[i] = rigid_c2w(i)
            kinds["rigid"].append(i)
        elif k == 1:
            A[i] = P * (1.0 + 0.25 * (i % 3))
            kinds["perm"].append(i)
        elif k == 2:
            A[i, 0, 0] = 0.0
            kinds["zero_pivot"].append(i)
        elif k == 3:
            A[i] = torch.eye(4) + 0.1 * (A[i] - 3 * torch.eye(4))
            A[i, 1:, 0] = 0.0
            A[i, 0, 3] = 300.0                      # a shear a (the determinant stays near 1): cond about a^2
            kinds["ill"].append(i)
    return A.contiguous(), kinds


def mat4_inv_refs(A, g):
    """linalg.inv and the gradient of sum(inv(A) g) in fp64, with E_f32 of CPU torch.linalg.inv in f32."""
    def run(dt):
        a = A.to(dt).clone().requires_grad_(True)
        y = torch.linalg.inv(a)
        y.backward(g.to(dt))
        return dict(inv=y.detach(), g_a=a.grad)
    r64, r32 = run(torch.float64), run(torch.float32)
    return r64, _e32(r32, r64, ("inv", "g_a"))


def mat4_mul_refs(A, B, g):
    def run(dt):
        a, b = A.to(dt).clone().requires_grad_(True), B.to(dt).clone().requires_grad_(True)
        c = a @ b
        c.backward(g.to(dt))
        return dict(c=c.detach(), g_a=a.grad, g_b=b.grad)
    r64, r32 = run(torch.float64), run(torch.float32)
    return r64, _e32(r32, r64, ("c", "g_a", "g_b"))


def unproject_refs(K, W, S, g):
    """M = (inv(S) inv(W)) inv(K) (common.py:139-141) and its three gradients."""
    def run(dt):
        ins = [x.to(dt).clone().requires_grad_(True) for x in (K, W, S)]
        iv = torch.linalg.inv
        M = (iv(ins[2]) @ iv(ins[1])) @ iv(ins[0])
        M.backward(g.to(dt))
        return dict(M=M.detach(), g_K=ins[0].grad, g_W=ins[1].grad, g_S=ins[2].grad)
    r64, r32 = run(torch.float64), run(torch.float32)
    return r64, _e32(r32, r64, ("M", "g_K", "g_W", "g_S"))


def pose_c2w_ref(r, t, init, g, dtype):
    """[Exp(r) | t; 0 0 0 1] @ init with Exp(r) = I + sin(th)/th [r]x + (1 - cos th)/th^2 [r]x^2,
    th = |r| + 1e-15 (include/nerf_hip.h), and the gradient of sum(c2w g) to r and t by autograd."""
    r = r.detach().to(dtype).clone().requires_grad_(True)
    t = t.detach().to(dtype).clone().requires_grad_(True)
    z = torch.zeros((), dtype=dtype)
    K = torch.stack([torch.stack([z, -r[2], r[1]]), torch.stack([r[2], z, -r[0]]), torch.stack([-r[1], r[0], z])])
    th = r.norm() + 1e-15
    R = torch.eye(3, dtype=dtype) + (torch.sin(th) / th) * K + ((1 - torch.cos(th)) / (th * th)) * (K @ K)
    c2w = torch.cat([torch.cat([R, t[:, None]], 1), torch.tensor([[0, 0, 0, 1]], dtype=dtype)], 0)
    if init is not None:
        c2w = c2w @ init.to(dtype)
    c2w.backward(g.to(dtype))
    return dict(c2w=c2w.detach(), g_r=r.grad, g_t=t.grad)


def pose_c2w_refs(r, t, init, g):
    r64, r32 = pose_c2w_ref(r, t, init, g, torch.float64), pose_c2w_ref(r, t, init, g, torch.float32)
    return r64, _e32(r32, r64, ("c2w", "g_r", "g_t")), r32


# ---- the depth-prior distortion ------------------------------------------------------------------------------
def affine32(d, s, t, shift_first):
    """The f32 torch expression of nerf_depth_affine before the clamp (training.py:259-264, 325-329)."""
    return (d + t) * s if shift_first else d * s + t


def depth_affine_inputs(n, shift_first, lo, seed=0):
    """d [n] in [0, 8) with s = 0.8, t = -0.25 and, for n >= 63, entries at d = 0 and (lo finite) entries
    whose f32 affine image is exactly lo (kept: the clamp is y < lo) and the largest d whose image is
    below lo (clamped), found by scanning the f32 neighbours of the fp64 solution ->
    dict(d, s, t, g, at_lo, below, zero: index lists)."""
    gen = torch.Generator().manual_seed(300 + n + seed)
    d = torch.rand(n, generator=gen) * 8
    s, t = torch.tensor([0.8]), torch.tensor([-0.25])
    idx = dict(at_lo=[], below=[], zero=[])
    if n >= 63:
        kinds = ("zero",)
        if lo != float("-inf"):
            kinds = ("at_lo", "below", "zero")
            d0 = torch.tensor(lo / s.double().item() - t.double().item() if shift_first
                              else (lo - t.double().item()) / s.double().item(), dtype=torch.float32)
            cand = (d0.view(torch.int32) + torch.arange(-32, 33, dtype=torch.int32)).view(torch.float32)
            img = affine32(cand, s, t, shift_first)
            assert bool((img == lo).any()) and bool((img < lo).any())
            d_at, d_below = cand[img == lo][0], cand[img < lo].max()
        for j, i in enumerate(range(3, n, max(1, n // 7))):
            kind = kinds[j % len(kinds)]
            d[i] = d_at if kind == "at_lo" else d_below if kind == "below" else 0.0
            idx[kind].append(i)
    return dict(d=d, s=s, t=t, g=torch.randn(n, generator=gen), **idx)


def depth_affine_ref(d, s, t, shift_first, lo, g, dtype=torch.float64, _wrong=None):
    """y = d s + t (shift_first: (d + t) s), y < lo -> lo; g_s, g_t = the sums over the entries not
    clamped of g dy/ds, g dy/dt, with the sums of |term|.  Which entries are clamped is decided on the
    f32 expression (the decision is the kernel's own, not a matter of precision)."""
    if _wrong == "shift_first_swapped":
        shift_first = not shift_first
    pre32 = affine32(d, s, t, shift_first)
    keep = (pre32 >= lo) if _wrong != "clamped_pass" else torch.ones_like(pre32, dtype=torch.bool)
    dd, ss, tt, gg = (x.to(dtype) for x in (d, s, t, g))
    pre = (dd + tt) * ss if shift_first else dd * ss + tt
    y = torch.where(pre32 < lo, torch.full_like(pre, lo), pre)
    ts = gg * ((dd + tt) if shift_first else dd) * keep
    tt_ = gg * (ss if shift_first else torch.ones_like(ss)) * keep
    return dict(y=y, g_s=ts.sum(), g_t=tt_.sum(), cond_s=ts.abs().sum(), cond_t=tt_.abs().sum(), keep=keep)


def f32_tree_sum(terms, threads=1024):
    """An f32 sum in the order of the one-workgroup kernels (per-thread strided serial sums, then a
    pairwise tree): the honest f32 evaluation the CPU module holds to tree_ceiling."""
    x = terms.float().reshape(-1)
    n = x.numel()
    pad = (-n) % threads
    x = torch.cat([x, x.new_zeros(pad)]).view(-1, threads)
    acc = torch.zeros(threads)
    for row in x:
        acc = acc + row
    while acc.numel() > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


# ---- camera rays ------------------------------------------------------------------------------------------
def camera_inputs(R, seed=0, nonfinite=False):
    """M [4][4] (a rigid pose, a 1.7 scale and a pinhole camera through the fp64 inverses), pixels [R][2]
    in [-1, 1], depth [R] in [1, 8] with zeros and negatives (and, nonfinite, one +inf and one NaN when R
    >= 4), five upstream gradients -> dict."""
    gen = torch.Generator().manual_seed(500 + R + seed)
    K = camera_K(188, 621, 362.5, 362.5)[0].double()
    S = torch.eye(4, dtype=torch.float64)
    S[:3, :3] *= 1.7
    iv = torch.linalg.inv
    M = ((iv(S) @ iv(torch.inverse(rigid_c2w(3)).double())) @ iv(K)).float()
    pix = torch.rand(R, 2, generator=gen) * 2 - 1
    depth = 1.0 + 7.0 * torch.rand(R, generator=gen)
    kinds = dict(zero=list(range(0, R, 5)), neg=[i for i in range(2, R, 7) if i % 5], inf=[], nan=[])
    depth[kinds["zero"]] = 0.0
    depth[kinds["neg"]] = -depth[kinds["neg"]]
    if nonfinite and R >= 4:
        depth[1], depth[3] = float("inf"), float("nan")
        kinds["inf"], kinds["nan"] = [1], [3]
        kinds["neg"] = [i for i in kinds["neg"] if i not in (1, 3)]
        kinds["zero"] = [i for i in kinds["zero"] if i not in (1, 3)]
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    return dict(M=M, pix=pix, depth=depth, g_cam=rn(R, 3), g_ray=rn(R, 3), g_view=rn(R, 3), g_norm=rn(R), g_dsrc=rn(R),
                kinds=kinds)


def camera_rays_ref(M, pix, depth, flags, dtype, grads=None, _wrong=None):
    """nerf_camera_rays by its header: cam = M[:3, 3]; v = M[:3, :3] (x, y, 1); ray_norm = |v|; ray =
    v / |v| (flag 1) else v; d_src = |M[:3, :3] (x d, y d, d)|, divided by |v| without flag 1; d_src = 1
    without a depth under either flag; view = -ray, or 1 with flag 2; mask = isfinite(d_src) & d_src != 0.
    grads: dict of the upstream gradients (g_cam, g_ray, g_view, g_norm, g_dsrc; a missing one is
    absent) -> also gM [4][4], its per-entry sum of |per-ray term| condM, and g_depth [R], by autograd
    with M expanded to one leaf per ray."""
    R = pix.shape[0]
    Mp = M.detach().to(dtype).expand(R, 4, 4).clone().requires_grad_(True)
    x, y = pix[:, 0].to(dtype), pix[:, 1].to(dtype)
    A = Mp[:, :3, :3]
    cam = Mp[:, :3, 3]
    v = A[:, :, 0] * x[:, None] + A[:, :, 1] * y[:, None] + A[:, :, 2]
    n = torch.linalg.norm(v, dim=1)
    normalise = bool(flags & 1)
    ray = v / n[:, None] if normalise else v
    d = None
    if depth is None:
        d_src = torch.ones(R, dtype=dtype)
    else:
        d = depth.detach().to(dtype).clone().requires_grad_(True)
        q = A[:, :, 0] * (x * d)[:, None] + A[:, :, 1] * (y * d)[:, None] + A[:, :, 2] * d[:, None]
        d_src = torch.linalg.norm(q, dim=1)
        if not normalise and _wrong != "dsrc_no_norm_div":
            d_src = d_src / n
    view = torch.ones_like(ray) if flags & 2 else -ray
    out = dict(cam=cam.detach(), ray=ray.detach(), view=view.detach(), ray_norm=n.detach(), d_src=d_src.detach(),
               mask=torch.isfinite(d_src.detach()) & (d_src.detach() != 0))
    if grads is not None:
        vg = view.detach() if _wrong == "view_grad_dropped" else view
        loss = torch.zeros((), dtype=dtype)
        for name, t in (("g_cam", cam), ("g_ray", ray), ("g_view", vg), ("g_norm", n), ("g_dsrc", d_src)):
            if grads.get(name) is not None:
                loss = loss + (t * grads[name].to(dtype)).sum()
        if loss.requires_grad:
            loss.backward()
        gp = torch.zeros_like(Mp) if Mp.grad is None else Mp.grad
        out.update(gM=gp.sum(0), condM=gp.abs().sum(0),
                   g_depth=None if d is None else (torch.zeros_like(d) if d.grad is None else d.grad))
    return out


def camera_rays_refs(M, pix, depth, flags, grads=None):
    r64 = camera_rays_ref(M, pix, depth, flags, torch.float64, grads)
    r32 = camera_rays_ref(M, pix, depth, flags, torch.float32, grads)
    names = ["cam", "ray", "view", "ray_norm", "d_src"] + (["gM"] if grads is not None else []) + \
        (["g_depth"] if grads is not None and depth is not None else [])
    e32 = {}
    for nme in names:
        a, b = r32[nme].double(), r64[nme].double()
        fin = torch.isfinite(b) & torch.isfinite(a)
        e32[nme] = (a - b)[fin].abs().max().item() if bool(fin.any()) else 0.0
    return r64, e32, r32


# ---- the ray loss ---------------------------------------------------------------------------------------------
def f32r(x: float) -> float:
    """A Python float rounded to f32 (what a float argument of the C ABI receives)."""
    return torch.tensor(x, dtype=torch.float32).item()


LOSS_W_RGB, LOSS_W_DEPTH = f32r(1.0), f32r(0.04)
LOSS_GO = dict(total=f32r(1.0), l_rgb=f32r(-0.7), l_depth=f32r(0.45), l2_mean=f32r(0.3))


def ray_loss_inputs(R, n_depth, mask_kind, seed=0):
    """rgb, gt [R][3] in [0, 1) with rgb == gt on every fifth element; dp, dg [n_depth] in [0, 5) with
    dp == dg on every third ray; mask [n_depth] bool or None ("none": no mask, "all", "one": exactly one
    valid ray, "zero": none valid)."""
    gen = torch.Generator().manual_seed(700 + 13 * R + n_depth + seed)
    rgb, gt = torch.rand(R, 3, generator=gen), torch.rand(R, 3, generator=gen)
    rgb.view(-1)[::5] = gt.view(-1)[::5]
    dp, dg = 5 * torch.rand(n_depth, generator=gen), 5 * torch.rand(n_depth, generator=gen)
    dp[::3] = dg[::3]
    mask = None
    if mask_kind != "none":
        mask = torch.zeros(n_depth, dtype=torch.bool)
        if mask_kind == "all":
            mask[:] = True
        elif mask_kind == "one":
            mask[n_depth - 1 if n_depth % 3 != 1 else n_depth // 2] = True
    assert mask_kind in LOSS_MASKS
    return dict(rgb=rgb, gt=gt, dp=dp, dg=dg, mask=mask)


def ray_loss_ref(rgb, gt, dp, dg, mask, l1, w_rgb, w_depth, go, dtype, _wrong=None):
    """nerf_ray_loss by its header: l_rgb = sum |e| (l1) or sum e^2 over rgb [R][3], divided by R;
    l_depth = sum over the mask of |dp - dg| / max(count, 1); l2_mean = mean e^2; total = w_rgb l_rgb +
    w_depth l_depth; and the gradients of sum_k go[k] out[k] (go: dict, a missing entry is absent) by
    autograd.  dp None: no depth term.  sums: the three raw sums (their terms are non-negative, so they
    are their own sums of |term|)."""
    R = rgb.shape[0]
    r = rgb.detach().to(dtype).clone().requires_grad_(True)
    e = r - gt.to(dtype)
    s2, s1 = (e * e).sum(), e.abs().sum()
    l_rgb = (s1 if l1 else s2) / float(3 * R if _wrong == "div_3R" else R)
    l2_mean = s2 / float(3 * R)
    p = q = None
    sd, cnt = torch.zeros((), dtype=dtype), 0.0
    l_depth = torch.zeros((), dtype=dtype)
    if dp is not None:
        p = dp.detach().to(dtype).clone().requires_grad_(True)
        q = dg.detach().to(dtype).clone().requires_grad_(True)
        m = torch.ones(p.shape[0], dtype=torch.bool) if (mask is None or _wrong == "mask_ignored") else mask.bool()
        sd = ((p - q).abs() * m).sum()
        cnt = float(m.sum())
        l_depth = sd / (cnt if _wrong == "cnt_unclamped" else max(cnt, 1.0))
    total = w_rgb * l_rgb + w_depth * l_depth
    out = dict(total=total, l_rgb=l_rgb, l_depth=l_depth, l2_mean=l2_mean)
    loss = torch.zeros((), dtype=dtype)
    for k, w in go.items():
        if w is not None:
            loss = loss + w * out[k]
    if loss.requires_grad:
        loss.backward()
    z = lambda t: None if t is None else (torch.zeros_like(t) if t.grad is None else t.grad)      # noqa: E731
    res = {k: v.detach() for k, v in out.items()}
    res.update(cnt=cnt, g_rgb=z(r), g_dp=z(p), g_dg=z(q), s1=s1.detach(), s2=s2.detach(), sd=sd.detach())
    return res


def ray_loss_refs(inp, l1, go, with_depth=True):
    a = (inp["rgb"], inp["gt"], inp["dp"] if with_depth else None, inp["dg"] if with_depth else None, inp["mask"], l1,
         LOSS_W_RGB, LOSS_W_DEPTH, go)
    r64, r32 = ray_loss_ref(*a, torch.float64), ray_loss_ref(*a, torch.float32)
    return r64, _e32(r32, r64, ("g_rgb",) + (("g_dp", "g_dg") if with_depth else ())), r32


def ray_loss_scalar_bars(r64, R, n_depth, l1):
    """The derived bars of the four scalars: tree_ceiling(n, 1024) of the raw sum over its divisor (the
    ceiling's four spare roundings cover forming a term -- e, e e or |e| -- and the division), and for
    total the weighted bars plus three roundings of |total| (two products and a sum)."""
    c3, cd = tree_ceiling(3 * R, 1024), tree_ceiling(max(n_depth, 1), 1024)
    b_rgb = c3 * (r64["s1"] if l1 else r64["s2"]).item() / R
    b_l2 = c3 * r64["s2"].item() / (3 * R)
    b_dep = cd * r64["sd"].item() / max(r64["cnt"], 1.0)
    b_tot = LOSS_W_RGB * b_rgb + LOSS_W_DEPTH * b_dep + 3 * U24 * abs(r64["total"].item())
    return dict(total=b_tot, l_rgb=b_rgb, l_depth=b_dep, l2_mean=b_l2)


# ---- Adam --------------------------------------------------------------------------------------------------------
def adam_inputs(n, steps=3, seed=0):
    """p [n] ~ N(0, 1) and `steps` gradients whose magnitudes spread over 1e-20 .. 1e4 with exact zeros;
    the last three elements (the n % 4 tail) keep O(1) gradients."""
    gen = torch.Generator().manual_seed(900 + n + seed)
    p = torch.randn(n, generator=gen)
    gs = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen)
        mag = torch.pow(10.0, torch.randint(-20, 5, (n,), generator=gen).float())
        mag[-3:] = 1.0
        g = g * mag
        if n > 8:
            g[torch.randint(0, n - 3, (max(1, n // 16),), generator=gen)] = 0.0
        gs.append(g)
    return p, gs


def adam_ref(p, g_list, hyper, dtype, _wrong=None):
    """torch.optim.Adam (amsgrad off, maximize off) written out, step by step from step 0:
    g += wd p; m = lerp(m, g, 1 - b1); v = b2 v + (1 - b2) g g; p -= lr / (1 - b1^t) m / (sqrt(v) /
    sqrt(1 - b2^t) + eps), the bias corrections in Python doubles -> (p, m, v).  hyper: dict(lr, b1, b2,
    eps, wd) and optionally om2: the 1 - beta2 of slot 6 of the device block, which the kernel uses as given
    whatever beta2 is (a block whose slot 6 is not exactly 1 - slot 3)."""
    import math
    lr, b1, b2, eps, wd = (hyper[k] for k in ("lr", "b1", "b2", "eps", "wd"))
    p = p.detach().to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    n = p.numel()
    live = n if _wrong != "tail_untouched" else n - n % 4
    for t, g in enumerate(g_list, start=0 if _wrong == "step_not_advanced" else 1):
        g = g.to(dtype)
        pn, mn, vn = p.clone(), m.clone(), v.clone()
        if wd != 0:
            g = g + wd * pn
        mn = mn + (g - mn) * (1 - b1)
        vn = vn * b2 + hyper.get("om2", 1 - b2) * (g * g)
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        if bc1 == 0:
            return p * float("nan"), m, v
        denom = vn.sqrt() / math.sqrt(bc2) + eps
        pn = pn - (lr / bc1) * (mn / denom)
        p[:live], m[:live], v[:live] = pn[:live], mn[:live], vn[:live]
    return p, m, v


def adam_refs(p, g_list, hyper):
    r64, r32 = adam_ref(p, g_list, hyper, torch.float64), adam_ref(p, g_list, hyper, torch.float32)
    return r64, [(a.double() - b).abs().max().item() for a, b in zip(r32, r64)], r32


def adam_bar(ref, e_f32):
    """4 E_f32 + 4 2^-24 max|ref|."""
    return F32_MARGIN * e_f32 + 4 * U24 * ref.abs().max().item()


# ---- the weight pack ---------------------------------------------------------------------------------------------
def chain_perm_ref(c, _wrong=None):
    """The chain order of nerf_pack_weights (include/nerf_hip.h): within each 32 columns, image column
    8 g + i holds column 4 g + i for i < 4 and 16 + 4 g + i - 4 otherwise."""
    base, q = c - c % 32, c % 32
    g, i = q // 8, q % 8
    src = 4 * g + i if i < 4 else 16 + 4 * g + i - 4
    if _wrong == "halves_exchanged":
        src = (src + 16) % 32
    return base + src


def chain_perm_index(n, perm_k, _wrong=None):
    """Column index of an n-wide chain image: the first perm_k columns in chain order, the rest in place."""
    return torch.tensor([chain_perm_ref(c, _wrong) if c < perm_k else c for c in range(n)], dtype=torch.long)


def split3_ref(x):
    """x -> (hi, mid, lo) bf16 words, each round-to-nearest-even (torch .bfloat16())."""
    h = x.bfloat16()
    r = x - h.float()
    m = r.bfloat16()
    lo = (r - m.float()).bfloat16()
    return [t.view(torch.int16) for t in (h, m, lo)]


def image_ref(mat):
    """[N][K] f32 -> bf16x3 image [3][K/8][N][8] (nerf_pack_desc.dst_s layout)."""
    N, K = mat.shape
    return torch.stack([p.view(N, K // 8, 8).permute(1, 0, 2) for p in split3_ref(mat)])


def pair_row_exp(mat):
    """The row exponents of the fp16 pair form: e_r with max|row| 2^e_r in [2^14, 2^15); 0 for a zero
    row; 140 for a subnormal row maximum (the largest scale an f32 exponent field gives: 2^140 times a
    subnormal stays below 2^14)."""
    rmax = mat.abs().amax(1).double()
    e = 14 - torch.floor(torch.log2(rmax.clamp_min(1e-300))).long()
    return torch.where(rmax > 0, e.clamp_max(140), torch.zeros_like(e))


def pair_image_ref(mat, perm=None, compact=False):
    """The fp16 pair image of a padded [N][K] f32 matrix (include/nerf_hip.h, mode 2): image column c
    holds matrix column perm[c] (None: c); hi = fp16(x 2^e), lo = fp16(x 2^e - hi), both round to
    nearest even -> dict(hi, lo: int16 [K/8][N][8]; e: int32 [N], the word at plane 2 chunk 0 of each
    row; with compact also ce, the int32 [N] array at chunk 1)."""
    N, K = mat.shape
    m = mat if perm is None else mat[:, perm]
    e = pair_row_exp(m)
    xs = (m.double() * torch.pow(2.0, e.double()).unsqueeze(1)).float()      # exact: a power of two (2^140 needs fp64)
    h = xs.half()
    lo = (xs - h.float()).half()
    lay = lambda t: t.view(torch.int16).view(N, K // 8, 8).permute(1, 0, 2).contiguous()      # noqa: E731
    out = dict(hi=lay(h), lo=lay(lo), e=e.to(torch.int32))
    if compact:
        out["ce"] = e.to(torch.int32)
    return out


def pair_image_read(img, compact=False):
    """The same fields out of a device image [3][K/8][N][8] int16."""
    img = img.detach().cpu()
    N = img.shape[2]
    out = dict(hi=img[0].contiguous(), lo=img[1].contiguous(),
               e=img[2, 0, :, 0:2].contiguous().view(torch.int32).view(N))
    if compact:
        out["ce"] = img[2, 1].contiguous().view(-1)[:2 * N].view(torch.int32)
    return out


def pair_image_value(fields):
    """(hi + lo) 2^-e, [N][K] fp64."""
    h, lo = (fields[k].permute(1, 0, 2).reshape(fields[k].shape[1], -1).view(torch.float16).double() for k in ("hi", "lo"))
    return (h + lo) * torch.pow(2.0, -fields["e"].double()).unsqueeze(1)


def pack_edge_rows(W):
    """Edge rows into a weight [rows][cols] (rows >= 8): row 1 zero, row 2 with maximum exactly 2^-3, row
    3 subnormal, row 4 with maximum 3e38 -> W."""
    W = W.clone()
    W[1] = 0.0
    W[2] = W[2] / W[2].abs().max() * 0.125
    W[3] = W[3] / W[3].abs().max() * 1e-39
    W[4] = W[4] / W[4].abs().max() * 3e38
    return W


# ---- the weight-gradient GEMMs and nerf_slab_reduce: fp64 references, derived ceilings, inputs ----------
# From the text of include/nerf_hip.h (nerf_linear_bwd_weight, nerf_gemm_set_precision, nerf_slab_reduce):
#   slab[split][o][col0 + j] = sum over the split's rows of dy[row, o] x[row, j],  bslab[split][o] = sum dy[row, o]
# and, in precision mode 2, every column of a split scaled by the power of two of its bound (the maximum over
# the split's 128-row groups of the passed column bounds), split into two fp16 words, three products.
WGRAD_KINDS = ("generic", "spread", "zeros", "edge", "loose", "outlier", "exact")
WGRAD_TIGHT = ("generic", "spread", "zeros", "loose")        # the kinds held to tight_bar
F32_TINY = 2.0 ** -149                                       # the smallest f32 subnormal: an output's grid below 2^-126


def wgrad_ref(dy, x, splits, _wrong=None):
    """fp64 per-split slabs [splits][nout][kin], bias partials [splits][nout] and their condition sums
    sum |dy||x| and sum |dy| over the split's rows -> (slab, bias, cond, bcond).
    _wrong="row": the last row of every split left out."""
    dy, x = _f64(dy), _f64(x)
    m = dy.shape[0]
    assert m % splits == 0 and x.shape[0] == m
    D, X = dy.view(splits, m // splits, -1), x.view(splits, m // splits, -1)
    if _wrong == "row":
        D, X = D[:, :-1], X[:, :-1]
    Dt = D.transpose(1, 2)
    return Dt @ X, D.sum(1), Dt.abs() @ X.abs(), D.abs().sum(1)


def wgrad_bounds(cmax, splits):
    """Column bounds per 128-row group [m/128][cols] -> the bound of each split [splits][cols]: the maximum
    over the split's groups (splits of whole groups)."""
    g = cmax.shape[0]
    assert g % splits == 0
    return _f64(cmax).view(splits, g // splits, -1).amax(1)


def wgrad_ceiling(rows, cond, dy_split, x_split, dy_bound=None, x_bound=None):
    """pair_ceiling for one split's slab = dy^T x ([nout][kin], K = rows): the GEMM's operand rows are the
    columns of dy and of x, and their maxima are replaced by the bounds the call was given (dy_bound [nout],
    x_bound [kin]: the maximum over the split's groups of the passed column bounds), since the scales come
    from the bounds -- a loose bound loosens the floor by exactly its slack:
      (6 rows + 16) 2^-24 cond + 2^-37 (dy_bound[o] sum_s |x[s, j]| + sum_s |dy[s, o]| x_bound[j]) + 2^-149.
    Without bounds (the exact-f32 and bf16x3 kernels: no scales, f32's own exponent range) the first term
    alone.  2^-149 is the grid of an f32 output below 2^-126.  A condition, not a measurement."""
    first = (6 * rows + 16) * U24 * cond + F32_TINY
    if dy_bound is None:
        return first
    dy_split, x_split = _f64(dy_split).abs(), _f64(x_split).abs()
    floor = _f64(dy_bound).unsqueeze(1) * x_split.sum(0).unsqueeze(0) + \
        dy_split.sum(0).unsqueeze(1) * _f64(x_bound).unsqueeze(0)
    return first + 2.0 ** -37 * floor


def wgrad_bias_ceiling(rows, bcond):
    """A bias partial is a plain f32 sum of the split's rows: dot_ceiling(rows, sum |dy|)."""
    return dot_ceiling(rows, bcond) + F32_TINY


def wgrad_reduced_ceiling(ceilings, slab_abs_sum, splits):
    """A reduced gradient: the sum of its splits' ceilings plus the reduce's own (splits + 2) 2^-24 sum |slab|."""
    return ceilings.sum(0) + (splits + 2) * U24 * slab_abs_sum


def pair_exp(bound):
    """The header's scale exponent of a bound (f32): 141 - biased exponent, 0 for a zero bound, 140 for a
    subnormal one -- the bound times 2^e lies in [2^14, 2^15)."""
    bits = bound.detach().cpu().float().contiguous().view(torch.int32).long()
    ex = (bits >> 23) & 0xff
    e = torch.where(ex > 0, 141 - ex, torch.full_like(ex, 140))
    return torch.where(bound.detach().cpu().float() == 0, torch.zeros_like(e), e)


def _pair_words(v, e):
    """v (fp64 holding f32 values) scaled by 2^e -> (hi, lo) fp16 words as fp64: hi = fp16(v 2^e), lo =
    fp16 of the remainder (exact in f32)."""
    s = (v * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())).float()
    hi = s.half()
    lo = (s - hi.float()).half()
    return hi.double(), lo.double()


def wgrad_pair_emulate(dy, x, dy_cmax, x_cmax, splits, _wrong=None):
    """The fp16-pair arithmetic of precision mode 2 in fp64, per split: the columns' exponents from the
    bounds (pair_exp of the maximum over the split's groups), the scaled operands as fp16 (hi, lo) words,
    hi.lo + lo.hi + hi.hi formed exactly (fp64 holds every 22-bit product; the sum's own rounding is 2^-53),
    the scales undone -> slabs [splits][nout][kin].  The representation error alone: no f32 accumulation.
    _wrong="drop": the lo.hi product dropped; _wrong="split": the bounds of the next split."""
    dy, x = _f64(dy), _f64(x)
    m = dy.shape[0]
    r = m // splits
    bd, bx = wgrad_bounds(dy_cmax, splits).float(), wgrad_bounds(x_cmax, splits).float()
    if _wrong == "split":
        bd, bx = bd.roll(-1, 0), bx.roll(-1, 0)
    out = []
    for s in range(splits):
        ea, eb = pair_exp(bd[s]), pair_exp(bx[s])
        ah, al = _pair_words(dy[s * r:(s + 1) * r], ea.unsqueeze(0))
        bh, bl = _pair_words(x[s * r:(s + 1) * r], eb.unsqueeze(0))
        acc = ah.t() @ bl + ah.t() @ bh
        if _wrong != "drop":
            acc = acc + al.t() @ bh
        out.append(acc * torch.pow(torch.tensor(2.0, dtype=torch.float64), -(ea.unsqueeze(1) + eb.unsqueeze(0)).double()))
    return torch.stack(out)


def _group_max(t, grp=128):
    return t.abs().view(t.shape[0] // grp, grp, t.shape[1]).amax(1).contiguous()


def _pm1(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def _set_colmax(t, col, value, grp, exact=None):
    """Column `col` scaled by `value` with one element of every group exactly +-exact (default: value), at a
    row that is never the group's first."""
    t[:, col] = t[:, col] * value
    exact = value if exact is None else exact
    for r0 in range(0, t.shape[0], grp):
        t[r0 + (7 * col + 3) % grp, col] = exact if (r0 // grp) % 2 == 0 else -exact


def wgrad_inputs(kind, m, nout, kin, seed, splits=1):
    """(dy [m][nout], x [m][kin], dy_cmax [m/128][nout], x_cmax [m/128][kin]) as f32 CPU tensors; the bounds
    are the exact group maxima unless the kind says otherwise, and None when m is no multiple of 128 (splits
    shorter than a group run without scales).  `splits` places the split-wise zeros of kind "zeros".
      generic  +-1 uniform; x clamped at 0 for an odd seed (a post-ReLU operand).
      spread   column c of dy scaled by 2^k, k cycling through CRAFT_EXPS; x the same scales in another order
               (column j: CRAFT_EXPS[(5 j + j // 6) % 6]), so every tile holds every pairing.
      zeros    dy column 1 / x column 2 dead (zero everywhere, bound 0); dy column 3 / x column 5 zero in every
               group of split 1 only; dy column 6 / x column 7 zero in the first 128-row group; dy entirely zero
               in the last split (splits > 1); the last 5 rows zero in both (padding rows).
      edge     dy: column 0 subnormal (maximum 2^-130), columns 1, 2, 3 with maxima exactly 2^-3, 1, 2^15,
               column 4 zero but for +-3e38 (alternating) at the first row of every 128-row group.  x: column 0
               subnormal, columns 1, 2, 3 with maxima exactly 2^-3, 1, 2^15, the upper half of the columns
               <= 2^-100 (column kin / 2 with maximum exactly 2^-100), and every column <= 2^-100 in the rows
               that carry a 3e38 (so no sum leaves f32's range).
      loose    x: column j scaled by a true maximum in [0.3, 1] with bound 1 (the encoder's sin / cos convention),
               the last column zero with bound 0 (its pad column); dy: bound = 8 x the true maximum.
      outlier  dy[17][0] 2^20 above the rest of its column; x is 0 in the even columns of that row.
      exact    dy[s][o] = 1 where o == s % nout, else 0; x[s][j] = (7 s + j) % 2048: every product and every
               sum is an integer below 2^24, exact in every mode, and differs at every (split, o, j)."""
    g = torch.Generator().manual_seed(seed)
    grp = 128 if m % 128 == 0 else m // splits
    r = m // splits
    dy, x = _pm1(g, m, nout), _pm1(g, m, kin)
    dcm = xcm = None
    if kind == "generic":
        if seed % 2:
            x = x.clamp_min(0)
    elif kind == "spread":
        dy = dy * (2.0 ** torch.tensor([CRAFT_EXPS[c % 6] for c in range(nout)], dtype=torch.float32))
        x = x * (2.0 ** torch.tensor([CRAFT_EXPS[(5 * j + j // 6) % 6] for j in range(kin)], dtype=torch.float32))
    elif kind == "zeros":
        dy[:, 1] = 0
        x[:, 2] = 0
        if splits > 1:
            dy[r:2 * r, 3] = 0
            x[r:2 * r, 5] = 0
            dy[m - r:] = 0
        dy[:grp, 6] = 0
        x[:grp, 7] = 0
        dy[m - 5:] = 0
        x[m - 5:] = 0
    elif kind == "edge":
        big = torch.arange(0, m, grp)
        for t in (dy, x):
            _set_colmax(t, 0, 2.0 ** -130, grp)
            _set_colmax(t, 1, 2.0 ** -3, grp)
            _set_colmax(t, 3, 2.0 ** 15, grp)
            _set_colmax(t, 2, 1.0, grp)
        x[:, kin // 2:] *= 2.0 ** -100
        _set_colmax(x, kin // 2, 1.0, grp, exact=2.0 ** -100)
        x[big] = x[big].clamp(-2.0 ** -100, 2.0 ** -100)
        dy[:, 4] = 0
        dy[big, 4] = 3e38 * (1 - 2 * (torch.arange(len(big)) % 2)).float()
    elif kind == "loose":
        x = x * (0.3 + 0.7 * torch.rand(1, kin, generator=g))
        x[:, kin - 1] = 0
        if m % 128 == 0:
            xcm = torch.ones(m // 128, kin)
            xcm[:, kin - 1] = 0
            dcm = 8 * _group_max(dy)
    elif kind == "outlier":
        dy[17, 0] = 2.0 ** 20
        x[17, 0::2] = 0
    elif kind == "exact":
        s = torch.arange(m)
        dy = (torch.arange(nout).unsqueeze(0) == (s % nout).unsqueeze(1)).float()
        x = ((7 * s.unsqueeze(1) + torch.arange(kin).unsqueeze(0)) % 2048).float()
    else:
        raise ValueError(kind)
    dy, x = dy.float().contiguous(), x.float().contiguous()
    if m % 128 == 0:
        dcm = _group_max(dy) if dcm is None else dcm
        xcm = _group_max(x) if xcm is None else xcm
        assert bool((dcm >= _group_max(dy)).all()) and bool((xcm >= _group_max(x)).all())      # bounds are bounds
    return dy, x, dcm, xcm


def slab_reduce_ref(slab, bslab, nout_ref, kin_ref, gw0=None, gb0=None):
    """nerf_slab_reduce in fp64: slab [splits][nout][ldslab], bslab [splits][nout] (or None) -> (gw, gb,
    cond_w, cond_b), gw [nout_ref][kin_ref] = sum over the splits (+ gw0 when accumulating), the condition
    sums sum |slab| (+ |gw0|) per element."""
    S = _f64(slab)[:, :nout_ref, :kin_ref]
    gw, cw = S.sum(0), S.abs().sum(0)
    if gw0 is not None:
        gw, cw = gw + _f64(gw0), cw + _f64(gw0).abs()
    gb = cb = None
    if bslab is not None:
        B = _f64(bslab)[:, :nout_ref]
        gb, cb = B.sum(0), B.abs().sum(0)
        if gb0 is not None:
            gb, cb = gb + _f64(gb0), cb + _f64(gb0).abs()
    return gw, gb, cw, cb


def slab_reduce_bar(splits, cond):
    """(splits + 2) 2^-24 sum |slab| per element: a sum of `splits` f32 terms in any order, the accumulated
    gradient one more (+ the grid of an f32 output below 2^-126)."""
    return (splits + 2) * U24 * cond + F32_TINY


# ---- the head kernels (nerf_heads_fwd, nerf_heads_bwd_mode, nerf_heads_reduce) ------------------------------
def heads_ref(h8, hr, wd, bd, wc, bc, graw4, dtype=torch.float64, _wrong=None):
    """The header's formulas at a dtype:
      raw4[s] = (h8[s].wd + bd, hr[s].wc[c] + bc[c]),  dyr = (graw4[s, 1:4] @ wc) * (hr > 0),
      gwd = sum_s graw4[s, 0] h8[s], gbd = sum_s graw4[s, 0], gwc[c] = sum_s graw4[s, 1 + c] hr[s],
      gbc[c] = sum_s graw4[s, 1 + c]
    -> dict(raw4, dyr, rmax, cmax (n % 128 == 0, else None), gwd, gbd, gwc, gbc) and the condition sums
    c_raw4, c_dyr, c_gwd, c_gbd, c_gwc, c_gbc (the same sums over absolute values).
    _wrong="gate": the gate read as hr >= 0.  The result lives where hr lives (the 131 k cases: on the device)."""
    c = lambda t: t.detach().to(hr.device, dtype)      # noqa: E731
    h8, hr, wd, bd, wc, bc, G = c(h8), c(hr), c(wd).reshape(1, -1), c(bd).reshape(1), c(wc), c(bc), c(graw4)
    n = hr.shape[0]
    out = dict(raw4=torch.cat([h8 @ wd.t() + bd, hr @ wc.t() + bc], 1),
               c_raw4=torch.cat([h8.abs() @ wd.abs().t() + bd.abs(), hr.abs() @ wc.abs().t() + bc.abs()], 1))
    gate = hr >= 0 if _wrong == "gate" else hr > 0
    out["gate"] = gate
    out["dyr"] = (G[:, 1:] @ wc).masked_fill(~gate, 0.0)
    out["c_dyr"] = (G[:, 1:].abs() @ wc.abs()).masked_fill(~gate, 0.0)
    out["rmax"] = out["dyr"].abs().amax(1)
    out["cmax"] = out["dyr"].abs().view(n // 128, 128, -1).amax(1) if n % 128 == 0 else None
    out["gwd"], out["c_gwd"] = G[:, 0] @ h8, G[:, 0].abs() @ h8.abs()
    out["gbd"], out["c_gbd"] = G[:, 0].sum().reshape(1), G[:, 0].abs().sum().reshape(1)
    out["gwc"], out["c_gwc"] = G[:, 1:].t() @ hr, G[:, 1:].abs().t() @ hr.abs()
    out["gbc"], out["c_gbc"] = G[:, 1:].sum(0), G[:, 1:].abs().sum(0)
    return out


def heads_sum_ceiling(n_pad, blocks, cond):
    """The ceiling of a head-weight or head-bias sum, from the summation order of nerf_heads_bwd_mode 2 / 3
    and nerf_heads_reduce: (chain + c) 2^-24 sum |term|.
      chain = 128 ceil(chunks / (4 blocks)), chunks = ceil(n_pad / 128): a lane adds the rows of its wave's
              128-row chunks to one accumulator, one rounding per row (an fma, or an add for the biases);
      c = ceil(blocks / 8) + 8: the four waves of a block (3 adds), the reduce's walk over the blocks (each of
          its four waves two chains of at most ceil(blocks / 8) partials, joined by 1 add), its four waves
          (2 adds in a tree), the accumulated gradient (1, counted whether or not the call accumulates), and 1 for the
          second-order terms.
    `blocks` is nerf_heads_part_size / (hidden + 3 max(64, hidden / 2) + 4).  A condition, not a measurement."""
    chunks = (n_pad + 127) // 128
    chain = 128 * ((chunks + 4 * blocks - 1) // (4 * blocks))
    c = (blocks + 7) // 8 + 8
    return (chain + c) * U24 * cond + F32_TINY


def heads_inputs(hidden, n_pad, seed, device="cpu"):
    """Head operands with the edge rows and columns of the fp64 head tests, built on `device`:
      hr  post-ReLU (+-1 clamped at 0), columns 3 and HR - 1 dead, and in rows 16 k + 1 .. 16 k + 3 the values
          0.0, -0.0 and the smallest positive subnormal in column 5;
      graw4  N(0, 1), each row scaled by 2^(+-30) or 1 (cycling), rows 16 k + 4 zero, 16 k + 5 sigma only,
          16 k + 6 rgb only.
    -> dict(h8, hr, wd, bd, wc, bc, graw4) f32, HR = max(64, hidden / 2)."""
    HR = max(64, hidden // 2)
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=device) * 2 - 1      # noqa: E731
    h8 = torch.rand(n_pad, hidden, generator=g, device=device)
    hr = rnd(n_pad, HR).clamp_min(0)
    hr[:, 3] = 0
    hr[:, HR - 1] = 0
    hr[1::16, 5] = 0.0
    hr[2::16, 5] = -0.0
    hr[3::16, 5] = F32_TINY
    graw4 = torch.randn(n_pad, 4, generator=g, device=device)
    rows = torch.arange(n_pad, device=device)
    graw4 = graw4 * (2.0 ** (30.0 * ((rows % 3) - 1).float())).unsqueeze(1)
    graw4[4::16] = 0
    graw4[5::16, 1:] = 0
    graw4[6::16, 0] = 0
    return dict(h8=h8, hr=hr, wd=rnd(1, hidden), bd=rnd(1), wc=rnd(3, HR), bc=rnd(3), graw4=graw4.contiguous())


def relu_words(gate):
    """bool [m][n] (n % 32 == 0) -> ReLU words [m][n / 32] int32, bit b of word w = column 32 w + b
    (nerf_linear_fwd's mask_out layout)."""
    m, n = gate.shape
    w = (gate.long().view(m, n // 32, 32) << torch.arange(32, device=gate.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
