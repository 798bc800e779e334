"""nerf_step_head (csrc/step_head.hip) against the entry points it replaces, bit for bit (GPU only).

The ray block must give exactly what nerf_pose_c2w, nerf_mat4_inv, nerf_unproject_matrix,
nerf_sample_rays, torch.index_select, nerf_depth_affine and nerf_camera_rays give on the same inputs;
the pack blocks exactly what nerf_pack_weights writes.  Nothing here has a tolerance: floats are
compared as their 32-bit patterns (NaNs included).  Every output is a helpers.Guarded buffer."""
import math

import pytest
import torch

from model import _hip
from tests import helpers as H
from tests.helpers import Guarded
from tests.test_gpu_prologue_fp64 import _Desc

pytestmark = pytest.mark.gpu

INT_FILL = -7
F_OUT = dict(c2w=(4, 4), world=(4, 4), M=(4, 4), inverses=(3, 4, 4))


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: differs from the separate entry points"


def _inputs(Hh, W, R, seed=0, r_scale=0.7, with_init=True, holes=True):
    """Device inputs of one step head: a LearnPose delta on a rigid init, a pinhole K, a 1.7 scale
    matrix, an image and a depth map with zeros, negatives, a NaN and an inf."""
    gen = torch.Generator().manual_seed(1000 + 7 * R + seed)
    n = Hh * W
    depth = 1.0 + 7.0 * torch.rand(n, generator=gen)
    if holes:
        depth[::5] = 0.0
        depth[2::7] = -depth[2::7]
        depth[1::11] = float("nan")
        depth[3::13] = float("inf")
    S = torch.eye(4)
    S[:3, :3] *= 1.7
    d = dict(r=(r_scale * torch.tensor(H.POSE_AXIS, dtype=torch.float64)).float(), t=0.1 * torch.randn(3, generator=gen),
             init=H.rigid_c2w(5).float() if with_init else None, K=H.camera_K(Hh, W, 362.5, 362.5)[0].float(),
             scale=S, img=torch.rand(3, Hh, W, generator=gen), depth=depth,
             aff_s=torch.tensor([1.3]), aff_t=torch.tensor([-0.4]))
    return d


def _dev(d, dev):
    return {k: (v.to(dev).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def _separate(dev, d, Hh, W, R, flags, counter=None, c2w_in=None, depth=True, affine=None, lo=float("-inf")):
    """The separate entry points, in the Trainer's order -> dict of plain tensors."""
    e = lambda *s: torch.empty(*s, device=dev)      # noqa: E731
    o = dict(c2w=e(4, 4), world=e(4, 4), M=e(4, 4), inverses=e(3, 4, 4), idx=torch.empty(R, dtype=torch.int64, device=dev),
             pixels=e(R, 2), rgb=e(R, 3), status=torch.empty(1, dtype=torch.int32, device=dev), cam=e(R, 3), ray=e(R, 3),
             view=e(R, 3), ray_norm=e(R), d_src=e(R), mask=torch.empty(R, dtype=torch.uint8, device=dev))
    if c2w_in is None:
        _hip.pose_c2w(d["r"], d["t"], d["init"], o["c2w"])
    else:
        o["c2w"].copy_(c2w_in)
    _hip.mat4_inv(o["c2w"], o["world"])
    _hip.unproject_matrix(d["K"], o["world"], d["scale"], o["M"], o["inverses"])
    _hip.sample_rays(Hh * W, R, H.SAMPLE_SEED, W, Hh, d["img"], o["idx"], o["pixels"], o["rgb"], o["status"], counter)
    dep = None
    if depth:
        dep = o["depth_g"] = torch.index_select(d["depth"], 0, o["idx"])
        if affine is not None:
            dep = o["depth_d"] = e(R)
            _hip.depth_affine(o["depth_g"], d["aff_s"], d["aff_t"], affine, lo, dep)
    _hip.camera_rays(o["M"], o["pixels"], dep, R, flags, o["cam"], o["ray"], o["view"], o["ray_norm"], o["d_src"], o["mask"])
    torch.cuda.synchronize()
    return o


def _ray_bufs(dev, R):
    g = dict(idx=Guarded((R,), dev, torch.int64, INT_FILL), pixels=Guarded((R, 2), dev), rgb=Guarded((R, 3), dev),
             status=Guarded((1,), dev, torch.int32, INT_FILL), depth_g=Guarded((R,), dev), depth_d=Guarded((R,), dev),
             cam=Guarded((R, 3), dev), ray=Guarded((R, 3), dev), view=Guarded((R, 3), dev), ray_norm=Guarded((R,), dev),
             d_src=Guarded((R,), dev), mask=Guarded((R,), dev, torch.uint8, 77))
    g.update({k: Guarded(s, dev) for k, s in F_OUT.items()})
    return g


def _ray_args(d, g, Hh, W, R, flags, counter=None, c2w_in=None, depth=True, affine=None, lo=float("-inf")):
    pose = dict(r=d["r"], t=d["t"], init_c2w=d["init"]) if c2w_in is None else dict(c2w_in=c2w_in)
    return _hip.step_head_rays(
        K=d["K"], scale=d["scale"], img=d["img"], depth_map=d["depth"] if depth else None,
        aff_scale=d["aff_s"] if affine is not None else None, aff_shift=d["aff_t"] if affine is not None else None,
        seed_counter=counter, seed=H.SAMPLE_SEED, n_pix=Hh * W, n_rays=R, width=W, height=Hh,
        shift_first=int(bool(affine)), flags=flags, lo=lo, **pose, **{k: b.t for k, b in g.items()})


def _fused(dev, d, Hh, W, R, flags, descs=(), **kw):
    g = _ray_bufs(dev, R)
    _hip.step_head(_ray_args(d, g, Hh, W, R, flags, **kw), descs)
    torch.cuda.synchronize()
    return g


def _compare(g, o, where, depth=True, affine=None):
    for k, b in g.items():
        assert b.intact(), f"{where}: wrote outside {k}"
        if k in o:
            _same(b.t, o[k].view(b.t.shape), f"{where}: {k}")
        else:       # depth_g without a depth map, depth_d without an affine
            assert (k == "depth_g" and not depth) or (k == "depth_d" and affine is None), k
            assert b.untouched(), f"{where}: {k} written though its input is absent"


@pytest.mark.parametrize("case", range(len(H.SAMPLE_CASES)))
def test_ray_block_equals_the_separate_entries(dev, case):
    """Every sampler shape (the per-thread slot edges, both ends of the dynamic table), a plain call
    and three calls on a device counter; idx and status also equal the table-free reference."""
    Hh, W, R = H.SAMPLE_CASES[case]
    flags = case % 4
    affine = (None, False, True)[case % 3]
    d = _dev(_inputs(Hh, W, R, seed=case), dev)
    where = f"step head {Hh}x{W} R={R} flags={flags} affine={affine}"
    o = _separate(dev, d, Hh, W, R, flags, affine=affine)
    g = _fused(dev, d, Hh, W, R, flags, affine=affine)
    _compare(g, o, where, affine=affine)
    ref_idx, rounds = H.sample_rays_ref(Hh * W, R, H.SAMPLE_SEED)
    assert torch.equal(g["idx"].t.cpu(), ref_idx) and g["status"].t.item() == rounds, where
    c_sep = torch.zeros(1, dtype=torch.int64, device=dev)
    ctr = Guarded((1,), dev, torch.int64, 0)
    for c in range(3):
        o = _separate(dev, d, Hh, W, R, flags, counter=c_sep, affine=affine)
        g = _fused(dev, d, Hh, W, R, flags, counter=ctr.t, affine=affine)
        _compare(g, o, f"{where} counter {c}", affine=affine)
        ref_c, rounds_c = H.sample_rays_ref(Hh * W, R, H.SAMPLE_SEED, counter=c)
        assert torch.equal(g["idx"].t.cpu(), ref_c) and g["status"].t.item() == rounds_c, f"{where} counter {c}"
        assert ctr.t.item() == c + 1 and c_sep.item() == c + 1 and ctr.intact(), f"{where}: counter after call {c}"


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("depth", [True, False])
def test_every_camera_flag_with_and_without_a_depth(dev, flags, depth):
    Hh, W, R = 41, 50, 1025
    d = _dev(_inputs(Hh, W, R), dev)
    _compare(_fused(dev, d, Hh, W, R, flags, depth=depth), _separate(dev, d, Hh, W, R, flags, depth=depth),
             f"flags={flags} depth={depth}", depth=depth)


@pytest.mark.parametrize("shift_first", [False, True])
@pytest.mark.parametrize("lo", [float("-inf"), 2.5])
def test_depth_holes_through_the_affine_and_the_clamp(dev, shift_first, lo):
    """A prior with zeros, negatives, NaN and inf through both affine orders and a finite clamp."""
    Hh, W, R = 33, 62, 1023
    d = _dev(_inputs(Hh, W, R, holes=True), dev)
    o = _separate(dev, d, Hh, W, R, 1, affine=shift_first, lo=lo)
    g = _fused(dev, d, Hh, W, R, 1, affine=shift_first, lo=lo)
    _compare(g, o, f"shift_first={shift_first} lo={lo}", affine=shift_first)
    dg = g["depth_g"].t
    assert bool(torch.isnan(dg).any()) and bool((dg == 0).any()) and bool((dg < 0).any()), "the draw met no hole"
    if lo > 0:
        assert bool((g["depth_d"].t == lo).any()), "nothing was clamped"


@pytest.mark.parametrize("scale", [H.POSE_R_SCALES[0], H.POSE_R_SCALES[2], H.POSE_R_SCALES[5]])
@pytest.mark.parametrize("with_init", [True, False])
def test_pose_range_and_a_handed_in_c2w(dev, scale, with_init):
    assert scale in (0.0, 1e-7, math.pi - 1e-3)
    Hh, W, R = 2, 3, 3
    d = _dev(_inputs(Hh, W, R, r_scale=scale, with_init=with_init, holes=False), dev)
    o = _separate(dev, d, Hh, W, R, 1)
    _compare(_fused(dev, d, Hh, W, R, 1), o, f"pose |r|={scale:g} init={with_init}")
    # the same pose handed in as a matrix: nothing but the copy differs
    c2w_in = o["c2w"].clone()
    o2 = _separate(dev, d, Hh, W, R, 1, c2w_in=c2w_in)
    _compare(_fused(dev, d, Hh, W, R, 1, c2w_in=c2w_in), o2, f"c2w handed in |r|={scale:g}")
    _same(o2["M"], o["M"], "handed-in pose")


# ---- the pack blocks --------------------------------------------------------------------------------
def _descs(dev, hidden, mode):
    """What FieldRunner.pack_descs sends at this hidden size and precision mode (l2 with the edge rows
    of helpers.pack_edge_rows), plus a 40 x 50 edge-row matrix into [64][64] destinations."""
    import model as mdl
    torch.manual_seed(3)
    net = mdl.OfficialStaticNerf(H.make_cfg(hidden=hidden, S=32))
    layers = net.hip_runner().layers
    chain = mode == 2 and hidden == 256
    out = []
    for l in layers:
        Wt = (l.linear.weight.detach() * torch.logspace(-3, 2, l.linear.weight.shape[0]).unsqueeze(1)).contiguous()
        if l.name == "l2":
            Wt = H.pack_edge_rows(Wt)
        out.append((l.name, _Desc(dev, Wt, l.kp, l.kp, l.out_p, l.out_p, images=mode >= 1, chain=chain,
                                  perm_k=l.k1 if l.name != "l0" else 0)))
    for l in layers:
        out.append((l.name + ".bias", _Desc(dev, l.linear.bias.detach().view(1, -1).contiguous(), l.out_p, with_t=False)))
    out.append(("wc", _Desc(dev, net.fc_rgb.weight.detach().contiguous(), max(64, hidden // 2), with_t=False)))
    out.append(("wd", _Desc(dev, net.fc_density.weight.detach().contiguous(), hidden, with_t=False)))
    Wt = H.pack_edge_rows(torch.randn(40, 50, generator=torch.Generator().manual_seed(9)))
    out.append(("padded", _Desc(dev, Wt, 64, 64, 64, 64, images=mode >= 1, chain=mode == 2, perm_k=32)))
    assert len(out) == 23
    return out


def _dest_bufs(descs):
    for name, d in descs:
        for k in ("dst", "dst_t", "s", "ts", "cs", "cts"):
            b = getattr(d, k)
            if b is not None:
                yield f"{name}.{k}", b


def _assert_packs_equal(a, b, where):
    for (na, ba), (nb, bb) in zip(_dest_bufs(a), _dest_bufs(b)):
        assert na == nb and ba.intact(), f"{where}: wrote outside {na}"
        assert torch.equal(ba.buf, bb.buf), f"{where}: {na} differs from nerf_pack_weights"


@pytest.fixture(scope="module")
def packed_ref(dev):
    """nerf_pack_weights' destinations per (hidden, mode), computed once."""
    cache = {}

    def get(hidden, mode):
        if (hidden, mode) not in cache:
            old = _hip.gemm_get_precision()
            _hip.gemm_set_precision(mode)
            try:
                ref = _descs(dev, hidden, mode)
                _hip.pack_weights([d.desc for _, d in ref])
                torch.cuda.synchronize()
            finally:
                _hip.gemm_set_precision(old)
            cache[(hidden, mode)] = ref
        return cache[(hidden, mode)]
    return get


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("hidden", [256, 64])
def test_pack_blocks_equal_pack_weights(dev, packed_ref, hidden, mode):
    ref = packed_ref(hidden, mode)
    got = _descs(dev, hidden, mode)
    _hip.gemm_set_precision(mode)
    _hip.step_head(None, [d.desc for _, d in got])
    torch.cuda.synchronize()
    _assert_packs_equal(got, ref, f"pack only hidden={hidden} mode={mode}")
    if mode == 2:
        for name, d in got:
            d.check(mode, f"step head pack {name}")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_both_parts_together_and_each_alone(dev, packed_ref, mode):
    Hh, W, R = 32, 64, 1024
    d = _dev(_inputs(Hh, W, R), dev)
    ref = packed_ref(256, mode)
    o = _separate(dev, d, Hh, W, R, 1, affine=False)
    _hip.gemm_set_precision(mode)
    where = f"both parts mode={mode}"
    # rays alone: the pack destinations keep their sentinels
    idle = _descs(dev, 256, mode)
    g = _fused(dev, d, Hh, W, R, 1, affine=False)
    _compare(g, o, where + " (rays alone)", affine=False)
    for name, b in _dest_bufs(idle):
        assert b.untouched(), f"{where}: {name} written by a rays-only call"
    # the pack alone: the ray outputs of the call before keep their values
    before = {k: b.buf.clone() for k, b in g.items()}
    _hip.step_head(None, [x.desc for _, x in idle])
    torch.cuda.synchronize()
    _assert_packs_equal(idle, ref, where + " (pack alone)")
    for k, b in g.items():
        assert torch.equal(_bits(b.buf), _bits(before[k])), f"{where}: {k} changed by a pack-only call"
    # both in one launch
    both = _descs(dev, 256, mode)
    g2 = _fused(dev, d, Hh, W, R, 1, descs=[x.desc for _, x in both], affine=False)
    _compare(g2, o, where, affine=False)
    _assert_packs_equal(both, ref, where)
