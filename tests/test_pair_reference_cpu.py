"""The staged fp64 / f32 reference of the image-pair kernels and the input sets of
tests/test_gpu_pair_fp64.py (tests/helpers.py) checked on the CPU: the reference is the oracle
expression of tests/test_gpu_pair.py; the bars reject wrong kernels (a torch-f32 emulation of the
family passes every check, each of its five wrong variants fails one); every input set keeps its
decisions away from their thresholds and holds the edge it claims."""
import pytest
import torch

from tests import helpers as H
from tests import test_gpu_pair as old


def _as_set(res, with_rgbs, with_scale):
    d1, d2, K, Rt, s1, img1, img2, nl = old._inputs(res, with_rgbs, with_scale)
    sq = lambda t: None if t is None else t[0]      # noqa: E731
    return dict(h=res[0], w=res[1], d1=d1.reshape(-1), d2=d2.reshape(-1), K=K[0], Rt=Rt[0], s1=s1, img1=sq(img1),
                img2=sq(img2), nl=nl)


@pytest.mark.parametrize("res,with_rgbs,with_scale", old.PAIR_CASES)
def test_staged_reference_is_the_oracle_expression(res, with_rgbs, with_scale):
    """On the three configurations of test_gpu_pair.py, in fp64: the staged reference fed its own
    neighbours and decisions gives the values and gradients of that module's _oracle."""
    d1, d2, K, Rt, s1, img1, img2, nl = old._inputs(res, with_rgbs, with_scale)
    o = [x.double().clone().requires_grad_(True) if x is not None else None for x in (d1, d2, Rt, s1)]
    ref = old._oracle(o[0], o[1], K.double(), o[2], o[3], None if img1 is None else img1.double(),
                      None if img2 is None else img2.double(), res, nl)
    (ref["pc"] + (0.7 * ref["rgb_s"] if with_rgbs else 0.0)).backward()

    inp = _as_set(res, with_rgbs, with_scale)
    pts, dec = H.pair_points(inp, torch.float64), H.pair_decisions(inp)
    nn = torch.stack([H.pair_neighbours(pts["X"], pts["Y"])[1], H.pair_neighbours(pts["Y"], pts["X"])[1]])
    st = H.pair_loss_ref(inp, nn, dec["valid"], dec["bad"], 1.0, 0.7 if with_rgbs else None)
    close = lambda a, b: torch.allclose(a.reshape(-1), b.reshape(-1), rtol=1e-10, atol=1e-14)      # noqa: E731
    assert close(st["pc"], ref["pc"].detach())
    if with_rgbs:
        assert close(st["rgb_s"], ref["rgb_s"].detach()) and int(dec["valid"].sum()) == ref["n_valid"]
        assert int((dec["bad"] & ~dec["valid"]).sum()) == 3 and not bool((dec["bad"] & dec["valid"]).any())
    assert close(st["g_d1"], o[0].grad) and close(st["g_d2"], o[1].grad)
    assert close(st["g13"][:9], o[2].grad[0, :3, :3]) and close(st["g13"][9:12], o[2].grad[0, :3, 3])
    if with_scale:
        assert close(st["g13"][12], o[3].grad)
    assert bool((st["cond13"] >= st["g13"].abs()).all())


# ---- a torch-f32 emulation of the family and its wrong variants -------------------------------------
def _emulate(inp, wrong=None):
    """What a correct f32 kernel family returns (X, Y, nn, out3, the gradients of every option), all
    decisions made in f32 on its own points; `wrong` makes it one of the wrong kernels."""
    P = inp["h"] * inp["w"]
    pts = H.pair_points(inp, torch.float32)
    X, Y = pts["X"], pts["Y"]

    def nearest(Q, R):
        d = Q[:, None, :] - R[None, :, :]
        D = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).sqrt()
        return P - 1 - D.flip(1).argmin(1) if wrong == "last_on_ties" else D.argmin(1)

    nn = torch.stack([nearest(X, Y), nearest(Y, X)])
    dec = H.pair_decisions(inp, torch.float32)
    fw = H.pair_loss_ref(inp, nn, dec["valid"], dec["bad"], 1.0, 1.0, False, torch.float32)
    out3 = torch.stack([fw["pc"], fw["rgb_s"], 3.0 * dec["valid"].sum()]).float()
    grads = {}
    for combo in (H.PAIR_COMBOS if inp["img1"] is not None else ("pc",)):
        for detach in ((0, 1) if inp["img1"] is not None else (0,)):
            go_pc, go_rgbs = H.PAIR_COMBOS[combo]
            w = None if wrong == "last_on_ties" else wrong
            grads[combo, detach] = H.pair_loss_ref(inp, nn, dec["valid"], dec["bad"], go_pc, go_rgbs, bool(detach),
                                                   torch.float32, _wrong=w)
    return dict(X=X, Y=Y, nn=nn, out3=out3, grads=grads)


def _check(inp, got, generic=True, ties=None):
    ref = H.PairRef(inp, generic=generic)
    ref.check_points(got["X"], got["Y"])
    neigh = ref.check_nn(got["X"], got["Y"], got["nn"])
    if ties is not None:
        first = H.pair_assert_ties(got["X"], got["Y"], ties[0], ties[1], neigh[0])
        assert torch.equal(got["nn"][0][ties[0]], first), "not the first index on a tie"
    ref.check_out3(got["out3"], got["nn"])
    for (combo, detach), g in got["grads"].items():
        ref.check_grads(g, got["nn"], combo, detach)
    return ref


def _wrong_cases():
    tie = H.pair_tie_inputs("chunks")
    tile = H.pair_tie_inputs("tile")
    return {"last_on_ties": [(tie[0], dict(generic=False, ties=tie[1:])), (tile[0], dict(generic=False, ties=tile[1:]))],
            "clamped_gradient": [(H.pair_clamped_inputs()[0], {})],
            "dropped_term": [(H.pair_generic_inputs(19, 27, "diag"), {})],
            "diagonal_K": [(H.pair_generic_inputs(19, 27, "principal"), {}), (H.pair_generic_inputs(19, 27, "skew"), {})],
            "scale_attached": [(H.pair_generic_inputs(19, 27, "diag"), {})]}


@pytest.mark.parametrize("wrong", ["last_on_ties", "clamped_gradient", "dropped_term", "diagonal_K", "scale_attached"])
def test_bars_reject_a_wrong_kernel(wrong):
    """Last index on ties, a gradient through a clamped point, one dropped scattered term, K taken as
    diagonal in the reprojection's gradient, the scale not detached: the unmodified emulation passes
    every check on the input set, the wrong one fails."""
    for inp, kw in _wrong_cases()[wrong]:
        _check(inp, _emulate(inp), **kw)
        with pytest.raises(AssertionError):
            _check(inp, _emulate(inp, wrong), **kw)


@pytest.mark.parametrize("h,w", [s for s in H.PAIR_SHAPES if s[0] * s[1] <= 900])
def test_emulation_passes_on_the_generic_sets(h, w):
    for cam in H.PAIR_CAMERAS:
        _check(H.pair_generic_inputs(h, w, cam), _emulate(H.pair_generic_inputs(h, w, cam)))


# ---- the input sets -------------------------------------------------------------------------------
def test_conditions_hold_on_every_input_set():
    """No decision within its margin of the threshold (validity 1e-5, nearest limit 1e-6, bilinear cell
    edge, sign of the colour difference), on every set of the GPU module with images."""
    names = []
    for name, inp in H.pair_input_sets():
        H.pair_assert_conditions(inp)
        names.append(name)
    assert len(names) == len(set(names)) == 3 * len(H.PAIR_SHAPES) + 11


def test_generic_sets_have_no_near_ties():
    """At most 0.1 % of the queries per direction within a relative gap of 1e-5 on the torch-f32 points,
    at every generic shape below the large one; no clamped point, both valid and invalid projections."""
    for h, w in H.PAIR_SHAPES:
        for cam in H.PAIR_CAMERAS:
            inp = H.pair_generic_inputs(h, w, cam)
            pts = H.pair_points(inp, torch.float32)
            for Q, R in ((pts["X"], pts["Y"]), (pts["Y"], pts["X"])):
                gap = H.pair_neighbours(Q, R)[2]
                assert int((gap <= H.PAIR_GAP).sum()) <= 1e-3 * h * w, (h, w, cam, gap.min().item())
            dec = H.pair_decisions(inp)
            assert not bool(dec["bad"].any())
            assert h * w == 4 or 0 < int(dec["valid"].sum()) < h * w, (h, w, cam)      # 2x2: four corners, none valid


def test_crafted_sets_hold_their_edges():
    """The premises of the crafted cases on the torch-f32 points (the GPU module asserts them again on
    the kernel's own): exact ties, one neighbour for all, coincident points, clamped and valid points,
    no valid point."""
    for case, n_tied in (("chunks", 300), ("tile", 3)):
        inp, tied, first_want = H.pair_tie_inputs(case)
        pts = H.pair_points(inp, torch.float32)
        first = H.pair_assert_ties(pts["X"], pts["Y"], tied, first_want, H.pair_neighbours(pts["X"], pts["Y"]))
        assert tied.numel() == n_tied and bool((first < inp["w"]).all())
    inp, hot = H.pair_many_to_one_inputs(47, 155)
    pts = H.pair_points(inp, torch.float32)
    assert bool((H.pair_neighbours(pts["X"], pts["Y"])[1] == hot).all())
    inp, patch = H.pair_coincident_inputs()
    pts = H.pair_points(inp, torch.float32)
    assert torch.equal(pts["X"][patch], pts["Y"][patch]) and patch.numel() == 66
    for Q, R in ((pts["X"], pts["Y"]), (pts["Y"], pts["X"])):
        best, first, _ = H.pair_neighbours(Q, R)
        assert bool((best[patch] == 0).all()) and torch.equal(first[patch], patch)
    inp, clamped = H.pair_clamped_inputs()
    dec = H.pair_decisions(inp)
    assert inp["K"][0, 0].abs() <= 1 and inp["K"][1, 1].abs() <= 1
    assert int((dec["bad"] & dec["valid"]).sum()) >= 3 and bool((dec["bad"] & dec["valid"])[clamped].all())
    assert not bool(dec["bad"][256:].any()) and 0 < int((dec["valid"] & ~dec["bad"]).sum())
    dec = H.pair_decisions(H.pair_no_valid_inputs())
    assert not bool(dec["valid"].any()) and dec["d_valid"].min().item() > 0.1


def test_norm_gradient_at_zero_is_zero():
    """torch's gradient of |x| at x = 0 is 0: the kernel's d > 0 branches."""
    x = torch.zeros(2, 3, dtype=torch.float64, requires_grad=True)
    torch.linalg.norm(x, dim=1).sum().backward()
    assert bool((x.grad == 0).all())
