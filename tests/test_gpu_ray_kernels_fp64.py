"""The per-ray kernels against fp64 at every sample-count edge (GPU only): the two compositing
families of csrc/render.hip (16 lanes per ray up to 256 samples, a wave per ray up to 1024), the
sample + encoding kernel and its backward, and the nearest-neighbour search of csrc/misc.hip,
called through the C ABI.

Accuracy bar, one rule everywhere: |hip - f64| <= T_project + 4 E_f32 (helpers.f32_bar).  T_project
is the fixed tolerance the suite already holds that quantity to; E_f32 is the error of the same
operation in plain f32 torch on the CPU against fp64, on the very same inputs and tensor -- never
a number taken from the kernels.  Every output is a slice of a larger buffer filled with a
sentinel, the payload 256 bytes in; the sentinel before and after it must survive every call."""
import pytest
import torch

from model import _hip
from oracle import nerf_oracle as orc
from tests import helpers as H
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu

R = H.COMPOSITE_R


def _rand(*s, g=None):
    return torch.rand(*s, generator=g) * 2 - 1


def _pad_rows(n):
    return (n + 127) // 128 * 128


# ---- compositing --------------------------------------------------------------------------------
def _composite_upload(dev, raw, z, R_, S, n_pad):
    raw_p, z_p = torch.zeros(n_pad, 4), torch.zeros(n_pad)
    raw_p[:R_ * S] = raw
    z_p[:R_ * S] = z.reshape(-1)
    return raw_p.to(dev), z_p.to(dev)


def _composite_run(dev, raw_d, z_d, R_, S, flags, g_rgb_d, g_dist_d, n_pad):
    out = dict(rgb=Guarded((R_, 3), dev), dist=Guarded((R_,), dev), alpha=Guarded((R_, S), dev),
               graw=Guarded((n_pad, 4), dev))
    _hip.composite_fwd(raw_d, z_d, R_, S, flags, out["rgb"].t, out["dist"].t, out["alpha"].t)
    _hip.composite_bwd(raw_d, z_d, R_, S, flags, g_rgb_d, g_dist_d, out["graw"].t, n_pad)
    torch.cuda.synchronize()
    for name, gd in out.items():
        assert gd.intact(), f"S={S} flags={flags}: wrote outside {name}"
    return {k: v.t for k, v in out.items()}


@pytest.mark.parametrize("S", H.COMPOSITE_S16 + H.COMPOSITE_SWAVE)
def test_composite_all_samples_all_flags(dev, S):
    """nerf_composite_fwd / _bwd at R = 37 (two whole 16-ray blocks + 5 rays; nine whole 4-ray
    blocks + 1), all eight flag values, generic and saturated inputs, against fp64; plus what must
    hold exactly: zero padding rows, dist_alpha's last sample, the ReLU gate, zero-gradient rays."""
    family = "composite16" if S <= 256 else "composite_wave"
    n = R * S
    n_pad = _pad_rows(n) + 128
    worst = {}
    for kind in H.COMPOSITE_KINDS:
        raw, z, g_rgb, g_dist = H.composite_edge_inputs(R, S, S, kind)
        raw_d, z_d = _composite_upload(dev, raw, z, R, S, n_pad)
        g_rgb_d, g_dist_d = g_rgb.to(dev), g_dist.to(dev)
        zero_rays = ((g_rgb == 0).all(1) & (g_dist == 0)).nonzero().flatten().tolist()
        assert zero_rays
        for flags in range(8):
            ref, e32 = H.composite_refs(raw, z, flags, g_rgb, g_dist)
            o = _composite_run(dev, raw_d, z_d, R, S, flags, g_rgb_d, g_dist_d, n_pad)
            graw = o["graw"].cpu()
            got = dict(rgb=o["rgb"].cpu(), dist=o["dist"].cpu(), alpha=o["alpha"].cpu(), grad=graw[:n])
            where = f"S={S} {kind} flags={flags}"
            for name, t in got.items():
                assert bool(torch.isfinite(t).all()), f"{where}: {name} not finite"
                assert t.shape == ref[name].shape, (where, name)
                err = (t.double() - ref[name]).abs().max().item()
                tp = (H.COMPOSITE_T_GRAD * max(1.0, ref[name].abs().max().item()) if name == "grad"
                      else H.COMPOSITE_T[name])
                ratio = err / (tp + e32[name])
                key = f"{name}-{kind}"
                worst[key] = max(worst.get(key, 0.0), ratio)
                print(f"{where} {name}: |hip-f64| {err:.3e}  E_f32 {e32[name]:.3e}  T {tp:.3e}  ratio {ratio:.3f}")
                assert err <= H.f32_bar(tp, e32[name]), (f"{where}: {name} |hip - f64| = {err:.3e} > "
                                                         f"{tp:.3e} + 4 * {e32[name]:.3e}")
            assert bool((graw[n:] == 0).all()), f"{where}: padding rows of graw4 not zero"
            g3 = got["grad"].view(R, S, 4)
            if flags & 1:
                assert bool((got["alpha"][:, -1] == 1.0).all()), f"{where}: last alpha"
                assert bool((g3[:, -1, 0] == 0.0).all()), f"{where}: last sample's density gradient"
            if flags & 4:
                dead = raw.view(R, S, 4)[:, :, 0] <= 0
                assert bool((g3[:, :, 0][dead] == 0.0).all()), f"{where}: gradient through a closed ReLU"
            assert bool((g3[zero_rays] == 0.0).all()), f"{where}: gradient of a ray without upstream gradient"
    for key, ratio in worst.items():
        H.report_err(f"ray_{family}", f"{key}-S{S}", ratio)


@pytest.mark.parametrize("S", [16, 100, 128, 300])
def test_composite_block_position_independence(dev, S):
    """Ray r alone (R = 1) and as ray r of the R = 37 batch: the same bits in rgb, dist, alpha and
    its graw4 rows -- the staged S == 16 J whole-block path against the generic one, the float4
    against the scalar z loads, DPP rows beside inactive rows against rows beside active ones."""
    n_pad = _pad_rows(R * S) + 128
    n_pad1 = _pad_rows(S) + 128
    for kind in H.COMPOSITE_KINDS:
        raw, z, g_rgb, g_dist = H.composite_edge_inputs(R, S, S, kind)
        raw_d, z_d = _composite_upload(dev, raw, z, R, S, n_pad)
        g_rgb_d, g_dist_d = g_rgb.to(dev), g_dist.to(dev)
        for flags in range(8):
            full = _composite_run(dev, raw_d, z_d, R, S, flags, g_rgb_d, g_dist_d, n_pad)
            for r in (0, 15, 16, 36):
                raw1, z1 = _composite_upload(dev, raw[r * S:(r + 1) * S], z[r:r + 1], 1, S, n_pad1)
                one = _composite_run(dev, raw1, z1, 1, S, flags, g_rgb[r:r + 1].to(dev), g_dist[r:r + 1].to(dev),
                                     n_pad1)
                where = f"S={S} {kind} flags={flags} ray {r}"
                assert torch.equal(one["rgb"][0], full["rgb"][r]), f"{where}: rgb"
                assert torch.equal(one["dist"][0], full["dist"][r]), f"{where}: dist"
                assert torch.equal(one["alpha"][0], full["alpha"][r]), f"{where}: alpha"
                assert torch.equal(one["graw"][:S], full["graw"][r * S:(r + 1) * S]), f"{where}: graw4"
                assert bool((one["graw"][S:] == 0).all()), f"{where}: padding rows"


def test_composite_sample_limit(dev):
    """S = 1025 is refused by both entry points, and nerf_composite_bwd refuses n_pad < R S: host
    checks, nothing launches, the outputs keep their sentinel."""
    R_, S = 2, 1025
    n_pad = _pad_rows(R_ * S) + 128
    raw_d, z_d = torch.zeros(n_pad, 4, device=dev), torch.zeros(n_pad, device=dev)
    g_rgb, g_dist = torch.ones(R_, 3, device=dev), torch.ones(R_, device=dev)
    outs = dict(rgb=Guarded((R_, 3), dev), dist=Guarded((R_,), dev), alpha=Guarded((R_, S), dev),
                graw=Guarded((n_pad, 4), dev))
    with pytest.raises(RuntimeError, match="> 1024"):
        _hip.composite_fwd(raw_d, z_d, R_, S, 0, outs["rgb"].t, outs["dist"].t, outs["alpha"].t)
    with pytest.raises(RuntimeError, match="> 1024"):
        _hip.composite_bwd(raw_d, z_d, R_, S, 0, g_rgb, g_dist, outs["graw"].t, n_pad)
    for S_ok in (1024, 100):      # one sample row short, in either family
        with pytest.raises(RuntimeError, match="bad sizes"):
            _hip.composite_bwd(raw_d, z_d, R_, S_ok, 0, g_rgb, g_dist, outs["graw"].t, R_ * S_ok - 1)
    torch.cuda.synchronize()
    for name, gd in outs.items():
        assert gd.untouched(), name


# ---- samples + encodings -------------------------------------------------------------------------
@pytest.mark.parametrize("R_,S", [(1, 1), (130, 1), (67, 2), (43, 3), (5, 127), (3, 129), (2, 1024), (1, 1000)])
def test_encode_samples_edges(dev, R_, S):
    """nerf_encode_samples without noise, with random noise and with noise at both ends of [0, 1),
    two wholly padded trailing blocks: z bit-equal to the oracle, the encodings against fp64 sin /
    cos of the kernel's own f32 sample point, padding exactly zero, exact row maxima, the column
    bound rules.  S = 1 puts 128 rays (every LDS ray record) in a block."""
    g = torch.Generator().manual_seed(7 + 131 * R_ + S)
    o = _rand(R_, 3, g=g) * 3
    d = torch.nn.functional.normalize(_rand(R_, 3, g=g), dim=-1)
    view = -d
    top = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)).item()
    noises = dict(none=None, random=torch.rand(R_, S, generator=g), zero=torch.zeros(R_, S),
                  top=torch.full((R_, S), top))
    n = R_ * S
    Np = _pad_rows(n) + 256
    od, dd, vd = o.to(dev), d.to(dev), view.to(dev)
    ref_d = orc.encode_position(view.double(), 4)[:, None, :].expand(R_, S, 27).reshape(n, 27)
    e32_d = (orc.encode_position(view, 4).double() - orc.encode_position(view.double(), 4)).abs().max().item()
    worst = 0.0
    for nm, noise in noises.items():
        where = f"R={R_} S={S} noise={nm}"
        G = dict(z=Guarded((Np,), dev), ep=Guarded((Np, 64), dev), ed=Guarded((Np, 64), dev), rp=Guarded((Np,), dev),
                 rd=Guarded((Np,), dev), cp=Guarded((Np // 128, 64), dev), cd=Guarded((Np // 128, 64), dev))
        _hip.encode_samples(od, dd, vd, None if noise is None else noise.to(dev), R_, S, Np, 0.01, 10.0, G["z"].t,
                            G["ep"].t, G["ed"].t, enc_p_rmax=G["rp"].t, enc_d_rmax=G["rd"].t, enc_p_cmax=G["cp"].t,
                            enc_d_cmax=G["cd"].t)
        torch.cuda.synchronize()
        for name, gd in G.items():
            assert gd.intact(), f"{where}: wrote outside {name}"
        z, ep, ed, rp, rd, cp, cd = (G[k].t.cpu() for k in ("z", "ep", "ed", "rp", "rd", "cp", "cd"))
        oz = orc.stratified_z(R_, S, 0.01, 10.0, None if noise is None else noise.view(1, R_, S))[0]
        bad = (z[:n] != oz.reshape(-1)).nonzero().flatten()
        assert bad.numel() == 0, f"{where}: {bad.numel()} z mismatches, first {bad[:8].tolist()}"   # bit-exact samples
        # the coordinates against fp64 o + d z, the sin / cos columns against fp64 at the kernel's own point
        x64 = (o.double()[:, None, :] + d.double()[:, None, :] * oz.double()[..., None]).reshape(n, 3)
        x32 = (o[:, None, :] + d[:, None, :] * oz[..., None]).reshape(n, 3)
        pts = ep[:n, :3]
        e_x = (x32.double() - x64).abs().max().item()
        err_x = (pts.double() - x64).abs().max().item()
        assert err_x <= H.f32_bar(2e-6, e_x), f"{where}: sample points {err_x:.3e} (E_f32 {e_x:.3e})"
        ref_p = orc.encode_position(pts.double(), 10)
        e_p = (orc.encode_position(pts, 10).double() - ref_p).abs().max().item()
        err_p = (ep[:n, :63].double() - ref_p).abs().max().item()
        err_d = (ed[:n, :27].double() - ref_d).abs().max().item()
        print(f"{where}: points {err_x:.3e} (E {e_x:.3e})  enc_p {err_p:.3e} (E {e_p:.3e})  enc_d {err_d:.3e} (E {e32_d:.3e})")
        worst = max(worst, err_x / (2e-6 + e_x), err_p / (2e-6 + e_p), err_d / (2e-6 + e32_d))
        assert err_p <= H.f32_bar(2e-6, e_p), f"{where}: enc_p {err_p:.3e} (E_f32 {e_p:.3e})"
        assert err_d <= H.f32_bar(2e-6, e32_d), f"{where}: enc_d {err_d:.3e} (E_f32 {e32_d:.3e})"
        assert bool(torch.isfinite(ep).all()) and bool(torch.isfinite(ed).all())
        assert ep[:, 63].abs().max().item() == 0 and ed[:, 27:].abs().max().item() == 0, f"{where}: pad columns"
        assert ep[n:].abs().max().item() == 0 and ed[n:].abs().max().item() == 0, f"{where}: pad rows"
        assert z[n:].abs().max().item() == 0, f"{where}: pad z"
        assert torch.equal(rp, ep.abs().amax(1)) and torch.equal(rd, ed.abs().amax(1)), f"{where}: row maxima"
        # column bounds per 128-row group: exact on the coordinates, >= the sin / cos maxima, 0 on the pad
        for c, e in ((cp, ep), (cd, ed)):
            ex = e.abs().view(Np // 128, 128, 64).amax(1)
            assert torch.equal(c[:, :3], ex[:, :3]) and bool((c >= ex).all()), f"{where}: column bounds"
        assert bool((cp[:, 3:63] == 1).all()) and bool((cp[:, 63] == 0).all()), where
        assert bool((cd[:, 3:27] == 1).all()) and bool((cd[:, 27:] == 0).all()), where
    H.report_err("ray_encode_samples", f"R{R_}-S{S}", worst)


@pytest.mark.parametrize("with_p2", [False, True])
@pytest.mark.parametrize("R_,S", [(1, 1), (3, 2), (5, 15), (5, 16), (5, 17), (2, 129), (1, 1024)])
def test_encode_bwd_edges(dev, R_, S, with_p2):
    """nerf_encode_bwd with fewer samples than its 16 waves, a ragged last stride and one sample,
    against fp64 autograd of the oracle's encode_position at the f32 sample points."""
    g = torch.Generator().manual_seed(17 + 31 * R_ + S)
    o = _rand(R_, 3, g=g) * 3
    d = torch.nn.functional.normalize(_rand(R_, 3, g=g), dim=-1)
    view = -d
    z = 0.01 + 9.99 * torch.rand(R_, S, generator=g)
    n = R_ * S
    gp, gp2, gd = torch.zeros(n, 64), torch.zeros(n, 64), torch.zeros(n, 64)
    gp[:, :63] = _rand(n, 63, g=g)
    gp2[:, :63] = _rand(n, 63, g=g)
    gd[:, :27] = _rand(n, 27, g=g)
    outs = [Guarded((R_, 3), dev) for _ in range(3)]
    _hip.encode_bwd(o.to(dev), d.to(dev), view.to(dev), z.reshape(-1).to(dev), gp.to(dev), gd.to(dev), R_, S,
                    *(q.t for q in outs), genc_p2=gp2.to(dev) if with_p2 else None)
    torch.cuda.synchronize()
    assert all(q.intact() for q in outs)
    # the sample points as the kernel forms them (f32 o + d z), differentiated there
    pts32 = (o.unsqueeze(1) + d.unsqueeze(1) * z.unsqueeze(-1)).reshape(-1, 3)
    gsum = gp[:, :63] + (gp2[:, :63] if with_p2 else 0)

    def autograd(dtype):
        p = pts32.to(dtype).clone().requires_grad_(True)
        v = view.to(dtype).clone().requires_grad_(True)
        loss = (orc.encode_position(p, 10) * gsum.to(dtype)).sum()
        loss = loss + (orc.encode_position(v.unsqueeze(1).expand(R_, S, 3).reshape(-1, 3), 4) * gd[:, :27].to(dtype)).sum()
        loss.backward()
        gpt = p.grad.view(R_, S, 3)
        return gpt.sum(1), (gpt * z.to(dtype).unsqueeze(-1)).sum(1), v.grad

    worst = 0.0
    for name, h, r64, r32 in zip(("g_pts_o", "g_pts_d", "g_view"), outs, autograd(torch.float64), autograd(torch.float32)):
        got = h.t.cpu().double()
        assert bool(torch.isfinite(got).all()), name
        e32 = (r32.double() - r64).abs().max().item()
        tp = 2e-5 * r64.abs().max().item()
        err = (got - r64).abs().max().item()
        print(f"R={R_} S={S} p2={with_p2} {name}: |hip-f64| {err:.3e}  E_f32 {e32:.3e}  T {tp:.3e}")
        worst = max(worst, err / (tp + e32))
        assert err <= H.f32_bar(tp, e32), f"R={R_} S={S} {name}: {err:.3e} > {tp:.3e} + 4 * {e32:.3e}"
    H.report_err("ray_encode_bwd", f"R{R_}-S{S}-p2{int(with_p2)}", worst)


# ---- nearest neighbour ---------------------------------------------------------------------------
def _nn(dev, X, Y):
    """X [3][P], Y [3][Q] -> idx [P] of nerf_chamfer_nn, inside a guarded int64 buffer."""
    P = X.shape[1]
    idx = Guarded((P,), dev, dtype=torch.int64, fill=-7)
    _hip.chamfer_nn(X.t().contiguous().to(dev), Y.t().contiguous().to(dev), idx.t)
    torch.cuda.synchronize()
    assert idx.intact()
    return idx.t.cpu()


@pytest.mark.parametrize("Q", [1, 255, 256, 257, 513])
def test_chamfer_nn_lattice_ties(dev, Q):
    """Points on the integer lattice {0..3}^3: every distance is exact, ties are exact and frequent,
    within an LDS tile of 256 reference points and across tiles; the first index wins, as
    torch.argmin in the oracle.  P = 1, a ragged block and two blocks."""
    Y = H.lattice_points(Q, 100 + Q)
    for P in (1, 255, 257):
        X = H.lattice_points(P, 200 + P)
        want = orc.closest_idx(X, Y)
        got = _nn(dev, X, Y)
        bad = (got != want).nonzero().flatten()
        assert bad.numel() == 0, (f"P={P} Q={Q}: {bad.numel()} mismatches, first at {bad[:4].tolist()}: "
                                  f"{got[bad[:4]].tolist()} vs {want[bad[:4]].tolist()}")


def test_chamfer_nn_tie_across_tiles(dev):
    """Q = 600 (three tiles): Y[3] == Y[300] == Y[599] is the unique nearest point of every query;
    index 3, the first tile's, must come back."""
    Q, P = 600, 300
    Y = H.lattice_points(Q, 5)
    target = torch.tensor([6.0, 6.0, 6.0])
    for j in (3, 300, 599):
        Y[:, j] = target
    X = H.lattice_points(P, 6, lo=5, hi=8)           # {5, 6, 7}^3: at most sqrt(3) from the target
    want = orc.closest_idx(X, Y)
    assert bool((want == 3).all())
    assert torch.equal(_nn(dev, X, Y), want)
