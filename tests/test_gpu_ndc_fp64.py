"""nerf_ndc_rays / nerf_ndc_rays_bwd (csrc/rays.hip) against the staged fp64 reference of
tests/ndc_ref.py at the launch edges (GPU only), through the C ABI with every output inside sentinel
guards, and through model.rays.ndc_rays with non-contiguous inputs.

Bars (tests/ndc_ref.py): per element |got - f64| <= 2^-23 max|f64| + 4 E_f32, E_f32 the f32 run of the
same reference against its f64 run; the two focal sums get (R - 1) 2^-24 sum |per-ray term| on top."""
import pytest
import torch

from model import _hip
from model import rays as mrays
from tests import ndc_ref as N
from tests.helpers import SENT, Guarded

pytestmark = pytest.mark.gpu

_REFS = {}


def _case(R):
    """Inputs and the (f64, f32) references per gradient combination, computed once per R."""
    if R not in _REFS:
        inp = N.ndc_inputs(R)
        _REFS[R] = (inp, {combo: N.ndc_refs(inp, combo) for combo in N.GRAD_COMBOS})
    return _REFS[R]


def _intact(G, where):
    for name, gd in G.items():
        assert gd.intact(), f"{where}: wrote outside {name}"
        assert not bool((gd.t == SENT).any()), f"{where}: {name} not fully written"


def _forward(dev, inp, with_dsrc=True, where=""):
    R = inp["cam"].shape[0]
    up = {k: v.to(dev) for k, v in inp.items() if torch.is_tensor(v)}
    G = dict(o_ndc=Guarded((R, 3), dev), d_ndc=Guarded((R, 3), dev))
    if with_dsrc:
        G["d_gt"] = Guarded((R,), dev)
    _hip.ndc_rays(up["cam"], up["ray"], up["K"], inp["near"], R, up["d_src"] if with_dsrc else None, G["o_ndc"].t,
                  G["d_ndc"].t, G["d_gt"].t if with_dsrc else None)
    torch.cuda.synchronize()
    _intact(G, f"{where} forward")
    return up, {k: g.t.cpu() for k, g in G.items()}


def _backward(dev, inp, up, combo="all", with_dsrc=True, with_gK=True, where=""):
    R = inp["cam"].shape[0]
    use_o, use_d, use_g = N.GRAD_COMBOS[combo]
    G = dict(g_cam=Guarded((R, 3), dev), g_ray=Guarded((R, 3), dev))
    if with_gK:
        G["gK"] = Guarded((4, 4), dev)
    if with_dsrc:
        G["g_dsrc"] = Guarded((R,), dev)
    t = lambda k: G[k].t if k in G else None      # noqa: E731
    _hip.ndc_rays_bwd(up["cam"], up["ray"], up["K"], inp["near"], R, up["d_src"] if with_dsrc else None,
                      up["g_o"] if use_o else None, up["g_d"] if use_d else None,
                      up["g_dgt"] if (use_g and with_dsrc) else None, G["g_cam"].t, G["g_ray"].t, t("gK"), t("g_dsrc"))
    torch.cuda.synchronize()
    _intact(G, f"{where} backward {combo}")
    return {k: g.t.cpu() for k, g in G.items()}


@pytest.mark.parametrize("R", N.EDGE_RAYS)
def test_ndc_kernels_against_fp64(dev, R):
    """One ray, one wave less / exactly / plus one ray, the forward block (256) and the backward block
    (1024) likewise, and 4097 rays: past the training batch, five forward blocks of 1024."""
    inp, refs = _case(R)
    where = f"R={R}"
    r64, r32 = refs["all"]
    up, fw = _forward(dev, inp, where=where)
    N.check_all(fw, r64, r32, R, where)
    # every optional pointer absent in turn
    _, fw_nd = _forward(dev, inp, with_dsrc=False, where=where)
    assert torch.equal(fw_nd["o_ndc"], fw["o_ndc"]) and torch.equal(fw_nd["d_ndc"], fw["d_ndc"])
    grads = {}
    for combo in N.GRAD_COMBOS:
        g = grads[combo] = _backward(dev, inp, up, combo, where=where)
        N.check_all(g, *refs[combo], R, f"{where} {combo}")
        if combo != "all":      # an absent upstream gradient is a zero one: the cotangents it cannot reach are 0
            if combo == "only_g_dgt":
                assert not bool(g["g_cam"].any()) and not bool(g["g_ray"].any()) and not bool(g["gK"].any())
            else:
                assert not bool(g["g_dsrc"].any())
    gk = grads["all"]["gK"]
    assert bool(gk[0, 0] != 0) and bool(gk[1, 1] != 0) and int((gk != 0).sum()) == 2, "gK: only [0][0], [1][1]"
    again = _backward(dev, inp, up, "all", where=where)
    for k in again:
        assert torch.equal(again[k], grads["all"][k]), f"{where}: {k} differs between two backward runs"
    no_gk = _backward(dev, inp, up, "all", with_gK=False, where=f"{where} gK = NULL")      # the grid-wide launch
    no_ds = _backward(dev, inp, up, "all", with_dsrc=False, where=f"{where} d_src = NULL")
    for k in ("g_cam", "g_ray"):
        assert torch.equal(no_gk[k], grads["all"][k]) and torch.equal(no_ds[k], grads["all"][k]), k
    assert torch.equal(no_gk["g_dsrc"], grads["all"]["g_dsrc"]) and torch.equal(no_ds["gK"], grads["all"]["gK"])


def test_ndc_full_eval_frame(dev):
    """756 x 1008 = 762 048 rays, a whole eval frame: 2977 forward blocks; the backward both ways."""
    R = 756 * 1008
    inp = N.ndc_inputs(R)
    r64, r32 = N.ndc_refs(inp)
    up, fw = _forward(dev, inp, where="frame")
    N.check_all(fw, r64, r32, R, "frame")
    g = _backward(dev, inp, up, "all", where="frame")
    N.check_all(g, r64, r32, R, "frame")
    g2 = _backward(dev, inp, up, "all", with_gK=False, where="frame gK = NULL")
    assert torch.equal(g2["g_cam"], g["g_cam"]) and torch.equal(g2["g_ray"], g["g_ray"])


def test_ndc_saturating_ray(dev):
    """A ray with d_z = 0: its own outputs are non-finite, as the reference's are, and every other
    ray's forward outputs keep their bits."""
    R, bad = 257, 130
    inp, _ = _case(R)
    _, fw = _forward(dev, inp, where="plain")
    sat = dict(inp)
    sat["ray"] = inp["ray"].clone()
    sat["ray"][bad] = torch.tensor([0.6, 0.8, 0.0])
    r32 = N.ndc_ref(sat, torch.float32)
    assert not bool(torch.isfinite(r32["o_ndc"][bad]).all()) and not bool(torch.isfinite(r32["d_ndc"][bad]).all())
    _, fs = _forward(dev, sat, where="saturating")
    keep = torch.arange(R) != bad
    for k in ("o_ndc", "d_ndc"):
        assert torch.equal(torch.isfinite(fs[k][bad]), torch.isfinite(r32[k][bad])), (k, fs[k][bad], r32[k][bad])
        assert torch.equal(fs[k][keep], fw[k][keep]), f"{k}: another ray changed"
    assert torch.equal(fs["d_gt"], fw["d_gt"])


def test_ndc_autograd_function_noncontiguous(dev):
    """model.rays.ndc_rays on strided views (cam, ray columns of a wider tensor, d_src every second
    entry, the camera matrix a transposed view): the same bits as contiguous inputs, gradients of the
    inputs' own shapes, needs_input_grad honoured."""
    R = 65
    inp, refs = _case(R)
    r64, r32 = refs["all"]
    wide = torch.zeros(R, 8, device=dev)
    wide[:, 1:4], wide[:, 4:7] = inp["cam"].to(dev), inp["ray"].to(dev)
    cam, ray = wide[:, 1:4].detach().requires_grad_(True), wide[:, 4:7].detach().requires_grad_(True)
    ds2 = torch.zeros(2 * R, device=dev)
    ds2[::2] = inp["d_src"].to(dev)
    d_src = ds2[::2].detach().requires_grad_(True)
    Km = inp["K"].t().contiguous().to(dev).t().unsqueeze(0).detach().requires_grad_(True)      # [1,4,4], strided
    assert not cam.is_contiguous() and not d_src.is_contiguous() and not Km.is_contiguous()
    o, d, dgt = mrays.ndc_rays(cam, ray, Km, 1.0, d_src)
    got = {"o_ndc": o, "d_ndc": d, "d_gt": dgt}
    N.check_all(got, r64, r32, R, "autograd fwd")
    up, fw = _forward(dev, inp)
    for k in fw:
        assert torch.equal(got[k].detach().cpu(), fw[k]), k
    ((o * up["g_o"]).sum() + (d * up["g_d"]).sum() + (dgt * up["g_dgt"]).sum()).backward()
    assert Km.grad.shape == (1, 4, 4) and cam.grad.shape == (R, 3) and d_src.grad.shape == (R,)
    N.check_all({"g_cam": cam.grad, "g_ray": ray.grad, "g_dsrc": d_src.grad, "gK": Km.grad[0]}, r64, r32, R, "autograd bwd")
    # only the camera matrix wants a gradient; no d_src
    K2 = inp["K"].to(dev).unsqueeze(0).requires_grad_(True)
    o, d, none = mrays.ndc_rays(inp["cam"].to(dev), inp["ray"].to(dev), K2)
    assert none is None
    ((o * up["g_o"]).sum() + (d * up["g_d"]).sum()).backward()
    assert torch.equal(K2.grad[0].cpu(), Km.grad[0].cpu())


def test_ndc_forward_bit_equality_with_torch_on_device(dev, capsys):
    """Observation, not an assertion: whether the forward equals the torch expressions bit for bit,
    evaluated on the device and on the CPU (DESIGN.md records the answer).  Asserted: the bars."""
    R = 1025
    inp, refs = _case(R)
    up, fw = _forward(dev, inp)
    N.check_all(fw, *refs["all"], R, "bit-equality inputs")
    r32 = refs["all"][1]
    cpu_equal = {k: bool(torch.equal(fw[k], r32[k])) for k in fw}
    fxfy = torch.cat([up["K"][None, 0, 0], up["K"][None, 1, 1]])
    from model.common import get_ndc_rays_fxfy
    o_t, d_t = get_ndc_rays_fxfy(fxfy, 1.0, up["cam"], up["ray"])
    dev_t = {"o_ndc": o_t.cpu(), "d_ndc": d_t.cpu(), "d_gt": (1 - 1 / up["d_src"]).cpu()}
    for k in fw:
        n = int((fw[k] != dev_t[k]).sum())
        with capsys.disabled():
            print(f"\nndc forward {k}: {n} of {fw[k].numel()} entries differ from torch on the device, "
                  f"max |diff| {(fw[k] - dev_t[k]).abs().max().item():.3e}; equal to torch on the CPU: {cpu_equal[k]}")
