"""The fp64 layer reference of the chain kernels (tests/helpers.py) checked on the CPU: composed
over all layers it is the oracle's field and its autograd, and the bars of
tests/test_gpu_chain_fp64.py tell a faithful f32 / fp16-pair GEMM from a subtly wrong one."""
import pytest
import torch

from oracle import nerf_oracle as orc
from tests import helpers as H


def _cpu_inputs(tiny=True):
    """The crafted [384][64] encodings from the oracle's encodings of 5 rays x 50 samples."""
    o, d = H.chain_test_rays()
    z = torch.linspace(0.01, 10.0, 50)
    pts = (o[:, None, :] + d[:, None, :] * z[None, :, None]).reshape(-1, 3)
    view = (-d)[:, None, :].expand(5, 50, 3).reshape(-1, 3)
    enc_p, enc_d = torch.zeros(256, 64), torch.zeros(256, 64)
    enc_p[:250, :63] = orc.encode_position(pts, 10)
    enc_d[:250, :27] = orc.encode_position(view, 4)
    return H.chain_crafted_inputs(enc_p, enc_d, tiny=tiny), pts, view


def test_composed_reference_is_the_oracle():
    """Layer order, masks, the skip and colour concatenations and the rank-one density term: the
    composed forward is OracleNerf.double() and the D_i are its autograd gradients, to 1e-12."""
    net = H.chain_test_net(0, "P1")
    ref = orc.OracleNerf(hidden_dim=256).double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    _, pts, view = _cpu_inputs()
    pts, view = pts.double(), view.double()
    enc_p = torch.cat([orc.encode_position(pts, 10), pts.new_zeros(250, 1)], 1)
    enc_d = torch.cat([orc.encode_position(view, 4), pts.new_zeros(250, 37)], 1)
    params, heads = H.chain_params(net)
    pres, raw4 = H.chain_compose_fwd(params, heads, enc_p, enc_d)
    # the oracle's ten linear outputs and its raw heads, by forward hooks
    lin = [ref.layers0[0], ref.layers0[2], ref.layers0[4], ref.layers0[6], ref.layers1[0], ref.layers1[2],
           ref.layers1[4], ref.layers1[6], ref.fc_feature, ref.rgb_layers[0], ref.fc_density, ref.fc_rgb]
    got = {}
    def keep(n):
        def hook(mod, inp, out):
            out.retain_grad()
            got[n] = out
        return hook
    hooks = [m.register_forward_hook(keep(n)) for n, m in enumerate(lin)]
    rgb, sigma = ref(pts, view)
    for h in hooks:
        h.remove()
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()      # noqa: E731
    for l in range(10):
        assert rel(pres[l], got[l].detach()) < 1e-12, l
    raw_o = torch.cat([got[10], got[11]], 1)
    assert rel(raw4, raw_o.detach()) < 1e-12
    # the oracle's activations too: sigmoid / softplus of the raw heads
    assert rel(torch.sigmoid(raw4[:, 1:]), rgb.detach()) < 1e-12
    graw4 = torch.randn(250, 4, generator=torch.Generator().manual_seed(4)).double()
    (raw_o * graw4).sum().backward()
    D = H.chain_compose_bwd(params, heads, pres, graw4)
    for i in range(10):
        assert bool((D[i] != 0).any()), i
        assert rel(D[i], got[9 - i].grad) < 1e-12, i


def _f32_chunks(x, B, b):
    """A float32 GEMM summed in eight K chunks, left to right."""
    x, B = x.float(), B.float()
    acc = torch.zeros(x.shape[0], B.shape[0])
    for c in range(0, x.shape[1], x.shape[1] // 8):
        acc = acc + x[:, c:c + x.shape[1] // 8] @ B[:, c:c + x.shape[1] // 8].t()
    return acc + b.float()


def _row_exp(m):
    """The power of two that takes a row maximum into [2^14, 2^15) (1 for a zero row)."""
    e = 14 - torch.floor(torch.log2(m.clamp_min(1e-300)))
    return torch.where(m > 0, 2.0 ** e, torch.ones_like(m))


def _pair(x, B, b, lo=True):
    """A faithful row-scaled fp16 pair GEMM: hi.hi + hi.lo + lo.hi in exact arithmetic, rounded to f32
    once (lo=False: the A operand as its fp16 hi word alone)."""
    x, B = x.double(), B.double()
    sx, sb = _row_exp(x.abs().amax(1, keepdim=True)), _row_exp(B.abs().amax(1, keepdim=True))
    xh = (x * sx).half().double()
    xl = (x * sx - xh).half().double() if lo else torch.zeros_like(xh)
    bh = (B * sb).half().double()
    bl = (B * sb - bh).half().double()
    acc = xh @ bh.t() + xh @ bl.t() + xl @ bh.t()
    return (acc / sx / sb.t() + b.double()).float()


@pytest.mark.parametrize("layer", [0, 1])
def test_bars_tell_a_wrong_kernel(layer):
    """The derived ceiling and the tight bar on the crafted rows (P2: small rows stay small):
    a float32 GEMM in another summation order and a faithful fp16 pair GEMM pass; the A operand as
    fp16 hi only, one small row doubled, one row off by 2^-18 fail."""
    net = H.chain_test_net(0, "P2")
    (enc_p, enc_d), _, _ = _cpu_inputs(tiny=False)
    params, heads = H.chain_params(net)
    x1 = enc_p
    for l in range(layer):      # the layer's input: a float32 forward of the layers before it
        x1 = H.chain_act(l, H.chain_fwd_ref(l, x1, None, *params[l])[0]).float()
    W, b = params[layer]
    x, Wp = H.chain_fwd_operands(layer, x1, None, W)
    pre, cond = H.chain_fwd_ref(layer, x1, None, W, b)
    ref = H.chain_act(layer, pre)
    ceil = H.pair_ceiling(H.CHAIN_KPAD[layer], cond, x, Wp)
    act = lambda t: H.chain_act(layer, t)      # noqa: E731
    base = act(x.float() @ Wp.float().t() + b.float())
    e_f32, nz = H.cond_error(base, ref, cond)
    assert nz == 0 and 0 < e_f32 < 64 * H.U24
    bar = H.tight_bar(e_f32)

    def verdict(got):
        e, nz = H.cond_error(got, ref, cond)
        under = bool(((got.double() - ref).abs() <= ceil).all())
        return e <= bar and nz == 0, under, e

    small = next(r for r in H.CRAFT["scaled"] if (r - 256) % 6 == 1 and bool((ref[r] != 0).any()))   # a 2^-30 row
    for name, got in (("f32 in chunks", act(_f32_chunks(x, Wp, b))), ("fp16 pair", act(_pair(x, Wp, b)))):
        tight, under, e = verdict(got)
        print(f"l{layer} {name}: e {e / H.U24:.2f} ulp against the bar {bar / H.U24:.2f} ulp (f32 {e_f32 / H.U24:.2f})")
        assert tight and under, name
    wrong = {"fp16 hi only": act(_pair(x, Wp, b, lo=False))}
    t = base.clone()
    t[small] *= 2
    wrong["small row doubled"] = t
    t = base.clone()
    t[small] *= 1 + 2.0 ** -18
    wrong["row off by 2^-18"] = t
    for name, got in wrong.items():
        tight, under, e = verdict(got)
        print(f"l{layer} {name}: e {e / H.U24:.2f} ulp, under the ceiling: {under}")
        assert not tight, name
    assert not verdict(wrong["fp16 hi only"])[1] and not verdict(wrong["small row doubled"])[1]
    # invisible to a max-normalised error: the doubled small row is 2^-30 of the largest row
    assert ((wrong["small row doubled"].double() - ref).abs().max() / ref.abs().max()).item() < 2e-6


def test_p1_conditions_hold_on_the_reference():
    """P1 on the fp64 reference alone: at least 8 rows are dead from l2 on (every l2 pre-activation
    below -0.5) and at least 8 rows are alive."""
    net = H.chain_test_net(0, "P1")
    (enc_p, enc_d), _, _ = _cpu_inputs()
    params, heads = H.chain_params(net)
    pres, raw4 = H.chain_compose_fwd(params, heads, enc_p, enc_d)
    dead = (pres[2] < -0.5).all(1)
    alive = (pres[2] > 0).any(1)
    print(f"P1: {int(dead.sum())} dead rows, {int(alive.sum())} alive rows")
    assert int(dead.sum()) >= 8 and int(alive.sum()) >= 8
    assert torch.isfinite(raw4).all()
