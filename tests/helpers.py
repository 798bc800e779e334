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
