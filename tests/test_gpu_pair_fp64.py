"""The image-pair kernels of csrc/pair.hip against fp64 at tie, chunk and scatter edges (GPU only),
called through the C ABI (nerf_pair_workspace / _forward / _backward) and, at the end, through
model.pair.pair_losses.

The reference works in stages (tests/helpers.py, checked on the CPU by test_pair_reference_cpu.py), so
that no discontinuous choice is compared across precisions: the points X, Y per element; the
neighbour table against the fp64 neighbours of the kernel's own X, Y (read back from the workspace);
losses and gradients against fp64 autograd with the kernel's own nn and the fp64 decisions, whose
distance to every threshold the reference asserts.  One bar everywhere: |hip - f64| <= T + 4 E_f32
(helpers.f32_bar), E_f32 the error of the same staged reference run in f32 -- never a number taken
from the kernels; T: 2^-23 of the largest entry for X, Y, g_d1, g_d2 (per element), 1e-6 of the
condition sum for each entry of g13, the suite's 1e-5 for the two losses.  Every buffer the kernels
write is a payload inside a sentinel-filled buffer, the workspace at exactly the size
nerf_pair_workspace returns."""
import pytest
import torch

from model import _hip
from model.pair import pair_losses
from tests import helpers as H
from tests.helpers import Guarded

pytestmark = pytest.mark.gpu


def _upload(inp, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _intact(G, where):
    for name, gd in G.items():
        assert gd.intact(), f"{where}: wrote outside {name}"


def _forward(dev, inp, where=""):
    h, w, P = inp["h"], inp["w"], inp["h"] * inp["w"]
    up = _upload(inp, dev)
    nc, nfl = _hip.pair_workspace(P)
    G = dict(work=Guarded((nfl,), dev), nn=Guarded((2 * P,), dev, dtype=torch.int32, fill=-7), out3=Guarded((3,), dev))
    _hip.pair_forward(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], up["img1"], up["img2"],
                      G["work"].t, G["nn"].t, G["out3"].t)
    torch.cuda.synchronize()
    _intact(G, f"{where} forward")
    work = G["work"].t.cpu()
    X, Y = work[:3 * P].view(P, 3), work[3 * P:6 * P].view(P, 3)      # the documented head of the workspace
    assert not bool((X == H.SENT).any()) and not bool((Y == H.SENT).any()), f"{where}: X, Y not written"
    nn = G["nn"].t.cpu().view(2, P)
    assert bool(((nn >= 0) & (nn < P)).all()), f"{where}: nn outside [0, P)"
    return dict(up=up, G=G, X=X, Y=Y, nn=nn, out3=G["out3"].t.cpu(), nc=nc)


def _backward(dev, inp, fw, combo, detach, want_d1=True, want_d2=True, where=""):
    h, w, P = inp["h"], inp["w"], inp["h"] * inp["w"]
    nb = (P + 255) // 256
    up = fw["up"]
    go_pc, go_rgbs = (None if v is None else torch.tensor([v], device=dev) for v in H.PAIR_COMBOS[combo])
    G = dict(gxy=Guarded((12 * P,), dev), g13=Guarded((13,), dev), part=Guarded((13 * nb,), dev))
    if want_d1:
        G["g_d1"] = Guarded((P,), dev)
    if want_d2:
        G["g_d2"] = Guarded((P,), dev)
    assert G["gxy"].t.data_ptr() % 8 == 0
    t = lambda k: G[k].t if k in G else None      # noqa: E731
    _hip.pair_backward(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], up["img1"], up["img2"],
                       int(detach), fw["G"]["work"].t, fw["G"]["nn"].t, fw["G"]["out3"].t, go_pc, go_rgbs, G["gxy"].t,
                       t("g_d1"), t("g_d2"), G["g13"].t, G["part"].t)
    torch.cuda.synchronize()
    _intact(G, f"{where} backward {combo}")
    _intact(fw["G"], f"{where} backward {combo} (forward buffers)")
    return {k: G[k].t.cpu() for k in ("g_d1", "g_d2", "g13", "part") if k in G}


def _same_bits(a, b, names, where):
    for n in names:
        assert torch.equal(a[n], b[n]), f"{where}: {n} differs between two runs"


def _full_check(dev, inp, where, test, generic=True):
    """Forward twice, every option of the backward, the NULL outputs and the repeat -> (ref, fw, grads)."""
    P = inp["h"] * inp["w"]
    ref = H.PairRef(inp, device=dev if P > 8192 else None, generic=generic)
    fw = _forward(dev, inp, where)
    _same_bits(fw, _forward(dev, inp, where), ("X", "Y", "nn", "out3"), where)
    ref.check_points(fw["X"], fw["Y"], where)
    fw["neigh"] = ref.check_nn(fw["X"], fw["Y"], fw["nn"], where)
    ref.check_out3(fw["out3"], fw["nn"], where)
    with_img = inp["img1"] is not None
    grads = {}
    for combo in (H.PAIR_COMBOS if with_img else ("pc",)):
        for detach in ((0, 1) if with_img else (0,)):
            g = grads[combo, detach] = _backward(dev, inp, fw, combo, detach, where=where)
            ref.check_grads(g, fw["nn"], combo, detach, where)
    first = ("both", 0) if with_img else ("pc", 0)
    _same_bits(grads[first], _backward(dev, inp, fw, *first, where=where), ("g_d1", "g_d2", "g13"), where)
    no1 = _backward(dev, inp, fw, *first, want_d1=False, where=where)      # pose-only learning: NULL outputs
    no2 = _backward(dev, inp, fw, *first, want_d2=False, where=where)
    none = _backward(dev, inp, fw, *first, want_d1=False, want_d2=False, where=where)
    _same_bits(grads[first], no1, ("g_d2", "g13"), f"{where} g_d1 = NULL")
    _same_bits(grads[first], no2, ("g_d1", "g13"), f"{where} g_d2 = NULL")
    _same_bits(grads[first], none, ("g13",), f"{where} g_d1 = g_d2 = NULL")
    ref.report(test)
    return ref, fw, grads


# ---- generic inputs at every shape and camera ---------------------------------------------------------
@pytest.mark.parametrize("cam", H.PAIR_CAMERAS)
@pytest.mark.parametrize("h,w", H.PAIR_SHAPES)
def test_pair_kernels_against_fp64(dev, h, w, cam):
    """2x2, one block less one point, one block, one block plus two points, three blocks, four chunks,
    the V_KITTI grid; a diagonal camera, one with a principal point, one with skew."""
    _full_check(dev, H.pair_generic_inputs(h, w, cam), f"{h}x{w}-{cam}", f"pair_{h}x{w}_{cam}")


@pytest.mark.parametrize("h,w", [(19, 27), (3, 85)])
def test_pair_kernels_full_camera(dev, h, w):
    """Every entry of K[:3] non-zero: inverse4 eliminates below and above every pivot, the translation
    column of inv(K) (+ Mi[4 r + 3]) and K[2][c], K[r][3] of the reprojection and its gradient count."""
    _full_check(dev, H.pair_generic_inputs(h, w, "full"), f"{h}x{w}-full", f"pair_{h}x{w}_full")


def test_pair_kernels_large(dev):
    """2x8193 = 16386 points, no images: the fixed-point scale 2^47, 15 chunks of five tiles, the last
    chunk partial (the neighbour reference runs in torch float64 on the device, in row blocks)."""
    inp = H.pair_large_inputs()
    assert _hip.pair_workspace(16386)[0] == 15
    _full_check(dev, inp, "2x8193", "pair_2x8193")


# ---- crafted cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chunks", "tile", "tiles"])
def test_pair_exact_ties_first_index(dev, case):
    """Exactly tied neighbours in different chunks (k_nn_final), inside one 256-point tile and in two
    tiles of one chunk (k_nn_part): the tie is asserted on the kernel's own X, Y, in fp64 and in the
    kernel's f32 expression; the first index must come back."""
    inp, tied, first_want = H.pair_tie_inputs(case)
    ref, fw, _ = _full_check(dev, inp, f"tie-{case}", f"pair_tie_{case}", generic=False)
    first = H.pair_assert_ties(fw["X"], fw["Y"], tied, first_want, fw["neigh"][0])
    got = fw["nn"][0][tied].long()
    assert torch.equal(got, first), (f"tie-{case}: {int((got != first).sum())} of {tied.numel()} tied queries without "
                                     f"the first index, e.g. {got[got != first][:4].tolist()} vs {first[got != first][:4].tolist()}")
    if case == "chunks":
        chunk = 256
        other = fw["neigh"][0][1][tied] + 2 * inp["w"]                       # the tied partner, two rows on
        assert fw["nc"] == 4 and bool((first // chunk != other // chunk).all())
    elif case == "tiles":
        assert fw["nc"] == 15 and first[0].item() // 1280 == 4296 // 1280 and first[0].item() // 256 != 4296 // 256


@pytest.mark.parametrize("h,w", [(47, 155), H.PAIR_LARGE])
def test_pair_many_to_one(dev, h, w):
    """Every X query chooses one Y pixel: P fixed-point terms land on one address (P 2^47 < 2^63 at the
    large shape); g_d2 there and everywhere else per element, bit-identical on a second run."""
    inp, hot = H.pair_many_to_one_inputs(h, w)
    ref, fw, grads = _full_check(dev, inp, f"many-{h}x{w}", f"pair_many_{h}x{w}", generic=False)
    assert bool((fw["neigh"][0][1] == hot).all()) and bool((fw["nn"][0] == hot).all())
    g = grads[("both", 0) if inp["img1"] is not None else ("pc", 0)]
    r64 = ref.refs(fw["nn"], "both" if inp["img1"] is not None else "pc", 0)[0]
    assert r64["g_d2"][hot].abs().item() > 100 * r64["g_d2"].abs().median().item()      # the sum of P terms
    assert g["g_d2"][hot].item() != 0


def test_pair_coincident_points(dev):
    """X_i == Y_i on a patch (Rt the identity, no scale, d1 == d2 there): each is the other's neighbour,
    the distance is 0, everything stays finite, and a patch point that no other query chose has a
    chamfer gradient of exactly 0."""
    inp, patch = H.pair_coincident_inputs()
    ref, fw, grads = _full_check(dev, inp, "coincident", "pair_coincident", generic=False)
    assert torch.equal(fw["X"][patch], fw["Y"][patch])
    for z in range(2):
        assert torch.equal(fw["nn"][z][patch].long(), patch), f"direction {z}"
    g = grads["pc", 0]
    P = inp["h"] * inp["w"]
    alone1 = patch[torch.bincount(fw["nn"][1].long(), minlength=P)[patch] == 1]      # X_i chosen by Y_i only
    alone2 = patch[torch.bincount(fw["nn"][0].long(), minlength=P)[patch] == 1]
    assert alone1.numel() > 0 and alone2.numel() > 0
    assert bool((g["g_d1"][alone1] == 0).all()) and bool((g["g_d2"][alone2] == 0).all())
    assert bool(torch.isfinite(g["g_d1"]).all()) and bool(torch.isfinite(g["g_d2"]).all())
    assert g["g_d1"].abs().max().item() > 0


def test_pair_clamped_and_valid_points(dev):
    """|K00|, |K11| <= 1: the 256 points of the first workgroup are clamped to (nl, nl, nl) and project
    inside the image.  out3[2] counts them; with go_rgbs alone their g_d1 is exactly 0 and the first
    workgroup's partial of dR, dt, ds1 is exactly 0: no gradient through a clamped point."""
    inp, clamped = H.pair_clamped_inputs()
    ref, fw, grads = _full_check(dev, inp, "clamped", "pair_clamped")
    both = ref.dec["bad"] & ref.dec["valid"]
    assert int(both.sum()) >= 3 and bool(both[clamped].all())
    assert fw["out3"][2].item() == 3.0 * int(ref.dec["valid"].sum())
    for detach in (0, 1):
        g = grads["rgbs", detach]
        assert bool((g["g_d1"][clamped] == 0).all())
        assert bool((g["part"][:13] == 0).all()), f"detach={detach}: {g['part'][:13].tolist()}"
        assert g["part"][13:26].abs().max().item() > 0


def test_pair_no_valid_point(dev):
    """Every projection outside [-1, 1]: rgb_s and its count are 0 (no 0 / 0), go_rgbs alone gives
    gradients of exactly 0, and both terms give the pc-only gradients bit for bit."""
    inp = H.pair_no_valid_inputs()
    ref, fw, grads = _full_check(dev, inp, "no-valid", "pair_no_valid")
    assert not bool(ref.dec["valid"].any())
    assert fw["out3"][1].item() == 0.0 and fw["out3"][2].item() == 0.0
    for detach in (0, 1):
        g = grads["rgbs", detach]
        assert all(bool((g[k] == 0).all()) for k in ("g_d1", "g_d2", "g13"))
        _same_bits(grads["both", detach], grads["pc", detach], ("g_d1", "g_d2", "g13"), f"no-valid detach={detach}")


def test_pair_refusals(dev):
    """h = 1 or w = 1, one image without the other, a gXY pointer that is 4 mod 8: host checks, nothing
    launches, every output keeps its sentinel."""
    inp = H.pair_generic_inputs(3, 5, "diag")
    up = _upload(inp, dev)
    P = 15
    G = dict(work=Guarded((_hip.pair_workspace(P)[1],), dev), nn=Guarded((2 * P,), dev, dtype=torch.int32, fill=-7),
             out3=Guarded((3,), dev), gxy=Guarded((12 * P + 1,), dev), g_d1=Guarded((P,), dev), g_d2=Guarded((P,), dev),
             g13=Guarded((13,), dev), part=Guarded((13,), dev))

    def fwd(h, w, img1, img2):
        _hip.pair_forward(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], img1, img2, G["work"].t,
                          G["nn"].t, G["out3"].t)

    def bwd(h, w, img1, img2, gxy):
        one = torch.ones(1, device=dev)
        _hip.pair_backward(up["d1"], up["d2"], h, w, up["K"], up["Rt"], up["s1"], inp["nl"], img1, img2, 0, G["work"].t,
                           G["nn"].t, G["out3"].t, one, one, gxy, G["g_d1"].t, G["g_d2"].t, G["g13"].t, G["part"].t)

    for h, w in ((1, 15), (15, 1)):
        with pytest.raises(RuntimeError, match="resolution"):
            fwd(h, w, up["img1"], up["img2"])
        with pytest.raises(RuntimeError, match="resolution"):
            bwd(h, w, up["img1"], up["img2"], G["gxy"].t)
    for i1, i2 in ((up["img1"], None), (None, up["img2"])):
        with pytest.raises(RuntimeError, match="go together"):
            fwd(3, 5, i1, i2)
        with pytest.raises(RuntimeError, match="go together"):
            bwd(3, 5, i1, i2, G["gxy"].t)
    odd = G["gxy"].t[1:]
    assert odd.data_ptr() % 8 == 4
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        bwd(3, 5, up["img1"], up["img2"], odd)
    with pytest.raises(RuntimeError, match="n_points"):
        _hip.pair_workspace(0)
    torch.cuda.synchronize()
    for name, gd in G.items():
        assert gd.untouched(), name


# ---- at the wrapper ----------------------------------------------------------------------------------
def _wrapper_run(dev, inp, which, d1_grad=True, d1_slice=False, twice=False):
    h, w = inp["h"], inp["w"]
    up = _upload(inp, dev)
    if d1_slice:                                   # a non-contiguous d1: every second element of a larger tensor
        big = torch.zeros(1, 1, h, 2 * w, device=dev)
        big[..., ::2] = up["d1"].view(1, 1, h, w)
        big.requires_grad_(d1_grad)
        d1 = big[..., ::2]
        assert not d1.is_contiguous()
    else:
        big = d1 = up["d1"].view(1, 1, h, w).clone().requires_grad_(d1_grad)
    d2 = up["d2"].view(1, 1, h, w).clone().requires_grad_(True)
    Rt = up["Rt"].view(1, 4, 4).clone().requires_grad_(True)
    s1 = up["s1"].clone().requires_grad_(True)
    l_pc, l_rgbs = pair_losses(d1, d2, up["K"].view(1, 4, 4), Rt, s1, up["img1"][None], up["img2"][None], (h, w), inp["nl"])
    loss = dict(pc=l_pc, rgbs=0.7 * l_rgbs, both=l_pc + 0.7 * l_rgbs)[which]      # the weights of H.PAIR_COMBOS
    loss.backward(retain_graph=twice)
    out = dict(l_pc=l_pc.detach().cpu(), l_rgbs=l_rgbs.detach().cpu(), d1=None if big.grad is None else big.grad.cpu(),
               d2=d2.grad.cpu(), Rt=Rt.grad.cpu(), s1=s1.grad.cpu())
    if twice:
        for t in (big, d2, Rt, s1):
            t.grad = None
        loss.backward()
        out["second"] = dict(d1=big.grad.cpu(), d2=d2.grad.cpu(), Rt=Rt.grad.cpu(), s1=s1.grad.cpu())
    return out


def test_pair_losses_wrapper_options(dev):
    """model.pair.pair_losses with images present: l_pc.backward() alone and l_rgbs.backward() alone
    against the staged reference with the C-level run's nn; d1 without requires_grad; a non-contiguous
    d1; a learned camera matrix raises; backward twice under retain_graph gives equal bits."""
    inp = H.pair_generic_inputs(19, 27, "principal")
    h, w, P = inp["h"], inp["w"], inp["h"] * inp["w"]
    ref = H.PairRef(inp)
    fw = _forward(dev, inp, "wrapper")
    runs = {}
    for which in ("both", "pc", "rgbs"):
        r = runs[which] = _wrapper_run(dev, inp, which, twice=(which == "both"))
        assert torch.equal(r["l_pc"], fw["out3"][0]) and torch.equal(r["l_rgbs"], fw["out3"][1])
        assert r["Rt"].shape == (1, 4, 4) and bool((r["Rt"][0, 3] == 0).all())
        g13 = torch.cat([r["Rt"][0, :3, :3].reshape(9), r["Rt"][0, :3, 3], r["s1"].reshape(1)])
        ref.check_grads(dict(g_d1=r["d1"].reshape(P), g_d2=r["d2"].reshape(P), g13=g13), fw["nn"], which, 0,
                        f"wrapper {which}")
    for k in ("d1", "d2", "Rt", "s1"):
        assert torch.equal(runs["both"][k], runs["both"]["second"][k]), f"second backward: {k}"
    frozen = _wrapper_run(dev, inp, "both", d1_grad=False)
    assert frozen["d1"] is None
    for k in ("d2", "Rt", "s1"):
        assert torch.equal(frozen[k], runs["both"][k]), f"d1 without grad: {k}"
    sliced = _wrapper_run(dev, inp, "both", d1_slice=True)
    assert torch.equal(sliced["d1"][..., ::2], runs["both"]["d1"]) and bool((sliced["d1"][..., 1::2] == 0).all())
    for k in ("d2", "Rt", "s1"):
        assert torch.equal(sliced[k], runs["both"][k]), f"non-contiguous d1: {k}"
    up = _upload(inp, dev)
    with pytest.raises(ValueError, match="camera matrix"):
        pair_losses(up["d1"].view(1, 1, h, w), up["d2"].view(1, 1, h, w), up["K"].view(1, 4, 4).clone().requires_grad_(True),
                    up["Rt"].view(1, 4, 4), up["s1"], up["img1"][None], up["img2"][None], (h, w), inp["nl"])
    ref.report("pair_wrapper")
