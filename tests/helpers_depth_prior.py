"""References of the depth-prior kernels: the draw-until-valid sampler (nerf_sample_rays_valid,
nerf_step_head_valid) and the invariant depth loss (nerf_ray_loss_invariant), written from the text of
include/nerf_hip.h and the reference lines it cites.  _wrong=...: the wrong variants of
tests/test_depth_prior_reference_cpu.py, nothing else."""
import numpy as np
import torch

from tests import helpers as H

ATTEMPT_STEP = 0xD1B54A32D192ED03
MAX_ATTEMPTS = 64               # NERF_SAMPLE_MAX_ATTEMPTS
M64 = 0xFFFFFFFFFFFFFFFF

# (n_pix, R) = (100, 4) on a 10 x 10 image whose only valid pixel is the last one: seeds that need
# exactly 1, exactly 2 and at least 5 attempts (found by scan_seeds, asserted by the CPU test)
SMALL = (10, 10, 4)
SMALL_SEEDS = {1: 51, 2: 20, 5: 0}
# 64 x 64, 1024 rays, valid where row % 20 == 0 and col % 20 == 0 (16 pixels): one and two-or-more attempts
STRIPE = (64, 64, 1024)
STRIPE_SEEDS = {1: 0, 2: 74}
CAP = (64, 128, 4096)           # 8192 pixels, 4096 rays (NERF_SAMPLE_MAX_RAYS), all valid
CAP_SEED = 7


def attempt_seed(seed: int, a: int) -> int:
    return (seed + a * ATTEMPT_STEP) & M64


def small_mask():
    m = np.zeros(SMALL[0] * SMALL[1], dtype=np.uint8)
    m[-1] = 1
    return m


def stripe_mask(h=STRIPE[0], w=STRIPE[1], step=20):
    m = np.zeros((h, w), dtype=np.uint8)
    m[::step, ::step] = 1
    return m.reshape(-1)


def sample_rays_valid_ref(n_pix, R, seed, valid, counter=None, _wrong=None):
    """The attempt rule of nerf_sample_rays_valid: attempt a is helpers.sample_rays_ref under the seed
    (seed + a ATTEMPT_STEP) mod 2^64 (the counter mixed in as ever), accepted when any drawn index is
    valid -> (idx, rounds, attempts); attempts = 0 and the last attempt's draw when none of
    MAX_ATTEMPTS is accepted.  valid None: the first attempt is accepted."""
    v = None if valid is None else np.asarray(valid).reshape(-1) != 0
    idx = rounds = None
    for a in range(MAX_ATTEMPTS):
        if _wrong == "same_seed":
            sa, ca = seed, counter
        elif _wrong == "attempt_in_counter":
            sa, ca = seed, (counter or 0) + a
        else:
            sa, ca = attempt_seed(seed, a), counter
        idx, rounds = H.sample_rays_ref(n_pix, R, sa, ca)
        if v is None or v[idx.numpy()].any():
            return idx, rounds, a + 1
    return idx, rounds, 0


def scan_seeds(n_pix, R, valid, want, start=0, stop=2000):
    """The first seed >= start per entry of want = {key: predicate on attempts}."""
    found = {}
    for s in range(start, stop):
        att = sample_rays_valid_ref(n_pix, R, s, valid)[2]
        for k, pred in want.items():
            if k not in found and pred(att):
                found[k] = s
        if len(found) == len(want):
            break
    return found


# ---- the invariant depth loss ------------------------------------------------------------------------------
INV_N = (2, 3, 4, 63, 64, 65, 1023, 1024, 1025, 4096)
INV_MASKS = ("none", "all", "third", "two")
INV_R = 21


def invariant_inputs(n_depth, mask_kind, seed=0, ties=0, R=INV_R):
    """rgb, gt [R][3] in [0, 1); dp, dg [n_depth] in [0.5, 5.5) with dp == dg on every third ray; mask
    [n_depth] bool or None ("none", "all", "third": every third ray, "two": exactly two valid).  ties > 0:
    that many masked entries of dp and of dg are set to the value that is then their median."""
    gen = torch.Generator().manual_seed(900 + 17 * n_depth + seed)
    rgb, gt = torch.rand(R, 3, generator=gen), torch.rand(R, 3, generator=gen)
    rgb.view(-1)[::5] = gt.view(-1)[::5]
    dp, dg = 0.5 + 5 * torch.rand(n_depth, generator=gen), 0.5 + 5 * torch.rand(n_depth, generator=gen)
    dp[::3] = dg[::3]
    mask = None
    if mask_kind != "none":
        mask = torch.zeros(n_depth, dtype=torch.bool)
        if mask_kind == "all":
            mask[:] = True
        elif mask_kind == "third":
            mask[1::3] = True
        elif mask_kind == "two":
            mask[0] = mask[n_depth - 1] = True
    assert mask_kind in INV_MASKS
    if ties:
        sel = torch.arange(n_depth) if mask is None else mask.nonzero().flatten()
        assert sel.numel() >= 2 * ties + 1
        for d in (dp, dg):
            vals = d[sel]
            order = vals.argsort()
            k = (sel.numel() - 1) // 2
            # the `ties` entries around the median rank all take the median's value
            lo = k - (ties - 1) // 2
            d[sel[order[lo:lo + ties]]] = vals[order[k]]
    return dict(rgb=rgb, gt=gt, dp=dp, dg=dg, mask=mask)


def invariant_ref(rgb, gt, dp, dg, mask, l1, w_rgb, w_depth, go, dtype, _wrong=None):
    """nerf_ray_loss_invariant by its header (losses.py:35-58): the rgb terms of helpers.ray_loss_ref; over
    the masked entries t = torch.median (the lower middle value), s = mean |d - t|, l_depth =
    mean(((p - t_p) / s_p - (g - t_g) / s_g)^2); total = w_rgb l_rgb + w_depth l_depth; the gradients of
    sum_k go[k] out[k] by torch autograd (the median's gradient spread evenly over the entries equal to it)."""
    R = rgb.shape[0]
    r = rgb.detach().to(dtype).clone().requires_grad_(True)
    e = r - gt.to(dtype)
    s2, s1 = (e * e).sum(), e.abs().sum()
    l_rgb = (s1 if l1 else s2) / float(R)
    l2_mean = s2 / float(3 * R)
    p = dp.detach().to(dtype).clone().requires_grad_(True)
    q = dg.detach().to(dtype).clone().requires_grad_(True)
    m = torch.ones(p.shape[0], dtype=torch.bool) if mask is None else mask.bool()

    def median(d):
        if _wrong == "upper_median":
            return d.sort().values[d.numel() // 2] if d.numel() else torch.median(d)
        if _wrong == "single_tie":      # the whole gradient on one of the tied entries
            return d[(d == torch.median(d).detach()).nonzero()[0, 0]] if d.numel() else torch.median(d)
        return torch.median(d)

    def norm(d):
        t = median(d)
        s = torch.mean(torch.abs(d - t))
        return (d - t) / s, t, s
    (u, t_p, s_p), (v, t_g, s_g) = norm(p[m]), norm(q[m])
    l_depth = ((u - v) ** 2).mean()
    total = w_rgb * l_rgb + w_depth * l_depth
    out = dict(total=total, l_rgb=l_rgb, l_depth=l_depth, l2_mean=l2_mean)
    loss = torch.zeros((), dtype=dtype)
    for k, w in go.items():
        if w is not None:
            loss = loss + w * out[k]
    if loss.requires_grad:
        loss.backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    res = {k: x.detach() for k, x in out.items()}
    res.update(cnt=float(m.sum()), t_p=t_p.detach(), s_p=s_p.detach(), t_g=t_g.detach(), s_g=s_g.detach(),
               ties_p=float((p[m] == t_p).sum()), ties_g=float((q[m] == t_g).sum()), g_rgb=z(r), g_dp=z(p), g_dg=z(q))
    return res


def invariant_refs(inp, l1, go):
    a = (inp["rgb"], inp["gt"], inp["dp"], inp["dg"], inp["mask"], l1, H.LOSS_W_RGB, H.LOSS_W_DEPTH, go)
    r64, r32 = invariant_ref(*a, torch.float64), invariant_ref(*a, torch.float32)
    names = ("total", "l_rgb", "l_depth", "l2_mean", "g_rgb", "g_dp", "g_dg")
    e32 = {}
    for n in names:
        d = (r32[n].double() - r64[n].double()).abs()
        d = d[torch.isfinite(r64[n].double()).reshape(d.shape)]
        e32[n] = d.max().item() if d.numel() else 0.0
        if e32[n] != e32[n]:
            e32[n] = 0.0
    return r64, e32, r32


def invariant_closed_form(dp, dg, mask, a_dep):
    """The depth part of the kernels as include/nerf_hip.h and csrc/rays.hip state it, in fp64: the median
    by rank (cnt - 1) // 2 of the sorted masked values, and the backward's closed form
      g_p[j] = (a_j - A m_j - B_p (sign_j - S_p m_j) / cnt) / s_p,  a_i = a_dep 2 (u_i - v_i) / cnt,
    with m_j = [d_j == t] / ties -> (l_depth, g_dp, g_dg, stats)."""
    p, g = dp.double(), dg.double()
    m = torch.ones(p.shape[0], dtype=torch.bool) if mask is None else mask.bool()
    cnt = int(m.sum())
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    t_p = p[m].sort().values[(cnt - 1) // 2] if cnt else nan
    t_g = g[m].sort().values[(cnt - 1) // 2] if cnt else nan
    ep, eg = torch.where(m, p - t_p, 0.0), torch.where(m, g - t_g, 0.0)
    n = torch.tensor(float(cnt), dtype=torch.float64)
    s_p, s_g = ep.abs().sum() / n, eg.abs().sum() / n
    ties_p, ties_g = float((m & (p == t_p)).sum()), float((m & (g == t_g)).sum())
    u, v = ep / s_p, eg / s_g
    r = torch.where(m, u - v, 0.0)
    l_depth = (r * r)[m].sum() / n
    a = torch.where(m, a_dep * 2.0 * (u - v) / n, 0.0)
    A, Bp, Bg = a[m].sum(), (a * u)[m].sum(), (a * v)[m].sum()
    Sp, Sg = torch.sign(ep)[m].sum(), torch.sign(eg)[m].sum()
    z = torch.zeros_like(p)       # f64 (a 0-dim f64 factor would not promote an f32 vector)
    mp = torch.where(m & (ep == 0), z + 1.0 / max(ties_p, 1.0), z)
    mg = torch.where(m & (eg == 0), z + 1.0 / max(ties_g, 1.0), z)
    g_p = torch.where(m, (a - A * mp - Bp * (torch.sign(ep) - Sp * mp) / n) / s_p, z)
    g_g = torch.where(m, (-a + A * mg + Bg * (torch.sign(eg) - Sg * mg) / n) / s_g, z)
    return l_depth, g_p, g_g, dict(cnt=float(cnt), t_p=t_p, s_p=s_p, t_g=t_g, s_g=s_g, ties_p=ties_p, ties_g=ties_g)


# ---- pieces shared with the step-head and graph tests --------------------------------------------------------
def step_head_pieces():
    """The input builders and bit-for-bit comparers of tests/test_gpu_step_head.py that the depth-prior GPU
    tests reuse, taken in one place: a rename there fails here, by name, and not somewhere inside a test."""
    import types
    from tests import test_gpu_step_head as T
    names = ("INT_FILL", "_compare", "_dev", "_inputs", "_ray_args", "_ray_bufs", "_same")
    missing = [n for n in names if not hasattr(T, n)]
    assert not missing, f"tests/test_gpu_step_head.py no longer has {missing}"
    return types.SimpleNamespace(**{n.lstrip("_"): getattr(T, n) for n in names})


def capture_graph(step, warm=3):
    """Warm `step` up on a side stream, then capture one call as a graph -> (graph, the call's outputs): the
    recipe of tests/test_gpu_graph.py."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warm):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    return g, out
