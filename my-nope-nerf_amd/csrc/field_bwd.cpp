// Native executor of the field backward (nerf_field_backward): the launch schedule of
// FieldRunner.backward for the D = 256 / colour 128 field in precision mode 2 in one host
// call -- the autograd of official_nerf.py:60-96 and rendering.py:113-141 as launched by
// training.py:92.  The Python schedule issues ~60 ctypes launches, ~20 temporaries and ~10
// cross-stream events per step (0.8 ms of host time at cfg2, profiles/r03/host_split_cfg2.json);
// here the same launches, in the same order on the same two streams, take a few microseconds
// each, so the eager step stays GPU-bound on a slow host core.
//
// Schedule (per layer, from the colour layer down): the input-gradient GEMM on the caller's
// stream, the weight gradient + its split-K slab reduce on the side stream once that layer's
// dy exists (an event), the last `tail_main` layers' weight gradients on the caller's stream
// after the input-gradient chain.  The head-weight partials run first on the side stream,
// dyr (the colour layer's dy, gated by its ReLU words) on the caller's.
//
// Host code only: every launch, argument, stream and event of both entries, under every knob,
// refusal and mid-schedule failure, is pinned by tests/test_field_bwd_trace.py on a CPU.
#include "common.hpp"

#include <cstdlib>
#include <vector>

namespace {

constexpr int L = NERF_BWD_LAYERS;
constexpr int D = 256, HR = 128;
// layer table (FieldRunner.layers): output rows, first-segment K, padded K, second segment
// (0 none, 1 enc_p, 2 enc_d)
constexpr int OUT_P[L] = {D, D, D, D, D, D, D, D, D, HR};
constexpr int K1[L] = {64, D, D, D, D, D, D, D, D, D};
constexpr int KP[L] = {64, D, D, D, D + 64, D, D, D, D, D + 64};
constexpr int SEG[L] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 2};
constexpr int NREF[L] = {D, D, D, D, D, D, D, D, D, HR};
constexpr int KREF[L] = {63, D, D, D, D + 63, D, D, D, D, D + 27};
constexpr int LF = 8, LR = 9;

struct Carve {
    char* base;
    size_t off = 0;
    float* take(size_t n) {
        off = (off + 255) & ~size_t(255);
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += n * sizeof(float);
        return p;
    }
};

struct Work {
    float *graw4, *dyr, *dyr_rm, *dyr_cm, *part, *hpart, *scratch;
    float *dx[L], *dx_rm[L], *dx_cm[L];   // dx[l]: gradient w.r.t. layer l's first input (l = 1..9)
    float *genc_p0, *genc_p4, *genc_d;
    float *slab[L], *bslab[L];
    int splits[L];
};

size_t carve(char* base, int np, int ray_grad, Work& w) {
    Carve c{base};
    w.graw4 = c.take((size_t)np * 4);
    w.dyr = c.take((size_t)np * HR);
    w.dyr_rm = c.take(np);
    w.dyr_cm = c.take((size_t)(np / 128) * HR);
    w.part = c.take((size_t)nerf_heads_part_size(D, np));
    w.hpart = c.take((size_t)nerf::heads_part_blocks(np) * (256 + 384 + 4));
    w.scratch = c.take(512);
    for (int l = 1; l < L; ++l) {
        w.dx[l] = c.take((size_t)np * K1[l]);
        w.dx_rm[l] = c.take(np);
        w.dx_cm[l] = c.take((size_t)(np / 128) * K1[l]);
    }
    w.dx[0] = w.dx_rm[0] = w.dx_cm[0] = nullptr;
    w.genc_p0 = ray_grad ? c.take((size_t)np * 64) : nullptr;
    w.genc_p4 = ray_grad ? c.take((size_t)np * 64) : nullptr;
    w.genc_d = ray_grad ? c.take((size_t)np * 64) : nullptr;
    for (int l = 0; l < L; ++l) w.splits[l] = nerf_linear_bwd_weight_splits(OUT_P[l], K1[l], np);
    for (int l = 0; l < L; ++l) {
        w.slab[l] = c.take((size_t)w.splits[l] * OUT_P[l] * KP[l]);
        w.bslab[l] = c.take((size_t)w.splits[l] * OUT_P[l]);
    }
    return c.off + 256;
}

// the frozen field's ray-only backward: graw4, the three dy the encoding segments read with their
// row maxima, the three encoding gradients
struct RaysWork {
    float *graw4, *d0, *d5, *d9, *rm0, *rm5, *rm9, *genc_p0, *genc_p4, *genc_d;
};

size_t carve_rays(char* base, int np, RaysWork& w) {
    Carve c{base};
    w.graw4 = c.take((size_t)np * 4);
    w.d0 = c.take((size_t)np * HR);
    w.d5 = c.take((size_t)np * D);
    w.d9 = c.take((size_t)np * D);
    w.rm0 = c.take(np);
    w.rm5 = c.take(np);
    w.rm9 = c.take(np);
    w.genc_p0 = c.take((size_t)np * 64);
    w.genc_p4 = c.take((size_t)np * 64);
    w.genc_d = c.take((size_t)np * 64);
    return c.off + 256;
}

// events: a per-thread pool (the autograd engine runs backwards on one thread per device)
struct EventPool {
    std::vector<hipEvent_t> ev;
    size_t next = 0;
    hipEvent_t get() {
        if (next == ev.size()) {
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            ev.push_back(e);
        }
        return ev[next++];
    }
};
thread_local EventPool g_events;

#define RC(x)                \
    do {                     \
        const int rc_ = (x); \
        if (rc_) return rc_; \
    } while (0)

// side waits for everything issued on main so far
int fork(hipStream_t main, hipStream_t side) {
    hipEvent_t e = g_events.get();
    NERF_CHECK(e != nullptr, "nerf_field_backward: hipEventCreate failed");
    NERF_CHECK(hipEventRecord(e, main) == hipSuccess && hipStreamWaitEvent(side, e, 0) == hipSuccess,
               "nerf_field_backward: cross-stream event failed");
    return NERF_OK;
}

// The schedule alternatives, read from the environment on EVERY call (the tests and the A/B
// scripts change them between calls in one process: nothing is cached).
struct Knobs {
    // NERF_WGRAD_SCHED, the chain's weight-gradient schedule: 3 (the default) two k_wgrad_jobs launches,
    // 2.062 vs 2.093 ms/step for 1 (profiles/r05/wgrad_sched_ab.json); 1 the round-4 schedule (r04n);
    // 2 one eight-layer launch with the encoding segments of l4 and l0 together (= 1 in-step)
    int sched;
    // NERF_WGRAD_GROUPS (schedule 3): 2 (the default) both launches as two block groups of 2 S' blocks
    // (S' = S / 2: each job twice the rows per split, half the jobs per block and half the
    // split-K slab bytes written and read back); 1 the second launch only; 0 one job list per
    // launch on 2 S blocks.  1.9125 / 1.9525 / 1.9721 ms per cfg2 step (2 / 1 / 0, fresh
    // processes interleaved, profiles/r06/wgrad_groups_lib_ab.txt)
    int groups;
    // NERF_WGRAD_BATCH1 (schedule 3): the first launch's slab reduces 2 (the default) in ONE reduce
    // launch with the second's, after it; 1 on the caller's stream between the two launches; 0 on the
    // side stream (it can only start once the second launch frees CUs; replayed as a hipGraph the
    // side-stream branch cost ~55 us per step, profiles/r05/batch1_ab.json)
    int batch1;
    // NERF_HEADS_PLACE, the head-weight partials (re-reading h8 and hr) of the chain schedule, on the
    // caller's stream BEFORE the chain: 1 (the default since round 6) k_heads_bwd mode 2 and
    // k_heads_reduce both there (1.8609 vs 1.8665 ms/step against 5 on the round-6 weight-gradient
    // schedule, profiles/r06/heads_place_r06_ab.txt); 5 the reduce (11 blocks, ~13 us) forked to the
    // side stream beside the chain (the round-5 default: 2.009 vs 2.030 ms/step then,
    // profiles/r05/heads_reduce_side_ab.json); 3 by k_heads_part (16-byte buffer loads, 4x the waves:
    // ~62 us in-step) with the reduces in the first slab batch (2.066 vs 2.058 ms/step,
    // profiles/r05/heads_part_ab.json); beside the chain (0, the round-4 placement) the partials and
    // their reduce stretch to ~240 us sharing the CUs with the chain, and the step is 13 us slower than
    // 1 (profiles/r05/heads_place_ab.json; 2 = after the chain: 7 us slower).  The per-layer schedule
    // keeps them on the side stream (0)
    int heads_place;
};

Knobs read_knobs() {
    auto knob = [](const char* name, int dflt) {
        const char* v = std::getenv(name);
        return v ? std::atoi(v) : dflt;
    };
    return Knobs{knob("NERF_WGRAD_SCHED", 3), knob("NERF_WGRAD_GROUPS", 2), knob("NERF_WGRAD_BATCH1", 2),
                 knob("NERF_HEADS_PLACE", 1)};
}

// ---- the layer lookups ------------------------------------------------------------------------
struct Grad {    // a layer's output gradient with its per-128-row-group column maxima and row maxima
    const float *dy, *cm, *rm;
};
struct Input {   // an input segment of a layer with its column maxima
    const float *x, *cm;
};
// layer l's dy as the input-gradient chain saved it (D_0 = dyr, D_i = dx[10 - i])
Grad dy_of(const Work& w, int l) {
    return l == LR ? Grad{w.dyr, w.dyr_cm, w.dyr_rm} : Grad{w.dx[l + 1], w.dx_cm[l + 1], w.dx_rm[l + 1]};
}
// layer l's first input segment (l0: enc_p)
Input x_of(const nerf_field_bwd& a, int l) {
    return l == 0 ? Input{a.enc_p, a.enc_p_cmax} : Input{a.act[l - 1], a.cmax[l - 1]};
}
// the 64-wide encoding segment of l4 (enc_p) and the colour layer (enc_d), at slab column K1[l]
Input enc_of(const nerf_field_bwd& a, int l) {
    return SEG[l] == 1 ? Input{a.enc_p, a.enc_p_cmax} : Input{a.enc_d, a.enc_d_cmax};
}
// where the gradient of the encoding that enters layer l (lr, l4, l0) goes
template <class W>
float* genc_of(const W& w, int l) { return l == LR ? w.genc_d : l == 4 ? w.genc_p4 : w.genc_p0; }

// ---- the pieces every schedule shares (A: nerf_field_bwd or nerf_field_bwd_rays) ----------------
// the upstream gradient: the given graw4, or g_rgb / g_dist through the composite backward
template <class A>
int upstream(const A& a, float* ws_graw4, void* stream, const float*& graw4) {
    graw4 = a.graw4;
    if (graw4) return NERF_OK;
    graw4 = ws_graw4;
    return nerf_composite_bwd(a.raw4, a.z, a.n_rays, a.n_samples, a.flags, a.g_rgb, a.g_dist, ws_graw4, a.n_pad, stream);
}

// the nerf_chain_bwd descriptor but for the D_i to store: D_0 = dyr, D_i the gradient at the
// output of layer 9 - i
template <class A>
nerf_chain_bwd chain_desc(const A& a, const float* graw4) {
    nerf_chain_bwd c{};
    c.graw4 = graw4;
    c.hr_mask = a.mask[LR];
    c.ld_hr_mask = HR / 32;
    c.wd = a.wd;
    c.wc = a.wc;
    for (int i = 0; i < 9; ++i) {
        const int l = LR - i;
        c.wt_img[i] = a.wt_cimg[l];   // the chain image: K in chain order (ABI 13)
        c.wt_img_rows[i] = KP[l];
        c.in_mask[i] = l == LR ? nullptr : a.mask[l - 1];
        c.ld_in_mask[i] = OUT_P[l - 1 < 0 ? 0 : l - 1] / 32;
    }
    c.n_pad = a.n_pad;
    return c;
}

// d enc (ray gradients: lr, l4, l0): the encoding segment's rows of W^T (l0: all of them) against
// layer l's dy
template <class A, class W>
int enc_rows(const A& a, const W& w, int l, const float* dy, const float* dy_rm, void* stream) {
    const int op = OUT_P[l];
    const int k0 = l == 0 ? 0 : K1[l];
    return nerf_linear_bwd_data(dy, op, op, a.wt[l] + (size_t)k0 * op, a.wt_img[l] + (size_t)k0 * 8, KP[l], nullptr, 0,
                                nullptr, nullptr, 0, genc_of(w, l), 64, a.n_pad, 64, dy_rm, nullptr, nullptr, stream);
}

template <class A, class W>
int encode_bwd(const A& a, const W& w, void* stream) {
    return nerf_encode_bwd(a.pts_o, a.pts_d, a.view, a.z, w.genc_p0, w.genc_p4, w.genc_d, a.n_rays, a.n_samples,
                           a.g_pts_o, a.g_pts_d, a.g_view, stream);
}

// the checks both entries make, under the name `who` their messages print
int check_precision(const char* who) {
    NERF_CHECK(nerf::gemm_precision() == 2, "%s: the native backward runs GEMM precision mode 2", who);
    return NERF_OK;
}
template <class A>
int check_layer(const A& a, int l, bool chain, const char* who) {
    NERF_CHECK(!chain || l == 0 || a.wt_cimg[l], "%s: layer %d: the input-gradient chain needs the chain image of "
               "W^T (wt_cimg)", who, l);
    NERF_CHECK((l == LF) == (a.mask[l] == nullptr), "%s: layer %d: ReLU words (none for the feature layer)", who, l);
    return NERF_OK;
}

// ---- the pieces of nerf_field_backward's schedules ------------------------------------------------
// the head-weight partials (k_heads_bwd mode 2) on `sp`, their reduce on `sr`: forked behind the
// partials where that is the other stream
int heads(const nerf_field_bwd& a, const Work& w, const float* graw4, hipStream_t sp, hipStream_t sr) {
    RC(nerf_heads_bwd_mode(2, graw4, a.act[7], D, a.act[LR], HR, nullptr, 0, D, a.wc, nullptr, 0, w.part, a.n_pad,
                           nullptr, nullptr, sp));
    if (sr != sp) RC(fork(sp, sr));
    return nerf_heads_reduce(w.part, D, a.n_pad, a.g_wd, a.g_bd, a.g_wc, a.g_bc, 0, sr);
}

// the weight-gradient launch of layer l (both segments of l4 / the colour layer) into its slab
int wgrad_launch(const nerf_field_bwd& a, const Work& w, int l, const float* dy, const float* dy_cm, void* s) {
    const Input x = x_of(a, l);
    if (!SEG[l])
        return nerf_linear_bwd_weight(dy, OUT_P[l], OUT_P[l], x.x, K1[l], K1[l], a.n_pad, w.splits[l], w.slab[l], KP[l], 0,
                                      w.bslab[l], dy_cm, x.cm, s);
    const Input e = enc_of(a, l);
    return nerf_linear_bwd_weight_seg(dy, OUT_P[l], OUT_P[l], x.x, K1[l], K1[l], e.x, 64, 64, a.n_pad, w.splits[l],
                                      w.slab[l], KP[l], w.bslab[l], dy_cm, x.cm, e.cm, s);
}

// split-K slab reduces batched into one launch
struct SlabBatch {
    nerf::SlabJobDesc jobs[nerf::kSlabJobsMax];
    int n = 0;
    void add(const nerf_field_bwd& a, const Work& w, int l) {   // layer l's, at its split count as of now
        jobs[n++] = nerf::SlabJobDesc{w.slab[l], w.splits[l], OUT_P[l], KP[l], NREF[l], KREF[l], w.bslab[l], a.gw[l],
                                      a.gb[l]};
    }
    int flush(hipStream_t main, hipStream_t s) {   // on s: the caller's stream, or the side stream behind an event
        if (s != main) RC(fork(main, s));
        RC(nerf::slab_reduce_jobs(jobs, n, s));
        n = 0;
        return NERF_OK;
    }
};

// The per-layer schedule (bwd_chain = 0): see the head of the file.
int per_layer_schedule(const nerf_field_bwd& a, const Work& w, const float* graw4, void* stream, void* side_stream) {
    const int np = a.n_pad;
    hipStream_t main = nerf::as_stream(stream), side = nerf::as_stream(side_stream);
    RC(nerf_heads_bwd_mode(1, graw4, nullptr, 0, nullptr, 0, a.mask[LR], HR / 32, D, a.wc, w.dyr, HR, nullptr, np,
                           w.dyr_rm, w.dyr_cm, stream));
    // weight + bias gradient of layer l on stream s
    auto weight_grad = [&](int l, const float* dy, const float* dy_cm, void* s) -> int {
        RC(wgrad_launch(a, w, l, dy, dy_cm, s));
        return nerf_slab_reduce(w.slab[l], w.splits[l], OUT_P[l], KP[l], NREF[l], KREF[l], w.bslab[l], a.gw[l], a.gb[l],
                                0, s);
    };
    const float *dy = w.dyr, *dy_rm = w.dyr_rm, *dy_cm = w.dyr_cm;
    int deferred[L], nd = 0;
    const float *def_dy[L], *def_cm[L];
    for (int step = 0; step < L; ++step) {
        const int l = L - 1 - step;   // lr, lf, l7, ..., l0
        if (step >= L - a.tail_main) {
            deferred[nd] = l; def_dy[nd] = dy; def_cm[nd] = dy_cm; ++nd;
        } else {
            RC(fork(main, side));
            RC(weight_grad(l, dy, dy_cm, side_stream));
        }
        if ((SEG[l] || l == 0) && a.ray_grad) RC(enc_rows(a, w, l, dy, dy_rm, stream));
        if (l == 0) break;
        // input gradient: dx = (dy W) masked by the ReLU words of the layer's input; at the feature
        // layer + the density path: d sigma_raw (graw4[:, 0]) x w_density, rank one
        const uint32_t* mask = l == LR ? nullptr : a.mask[l - 1];
        RC(nerf_linear_bwd_data(dy, OUT_P[l], OUT_P[l], a.wt[l], a.wt_img[l], KP[l], l == LF ? graw4 : nullptr,
                                l == LF ? 4 : 0, l == LF ? a.wd : nullptr, mask, OUT_P[l - 1] / 32, w.dx[l], K1[l], np,
                                K1[l], dy_rm, w.dx_rm[l], w.dx_cm[l], stream));
        dy = w.dx[l]; dy_rm = w.dx_rm[l]; dy_cm = w.dx_cm[l];
    }
    for (int i = 0; i < nd; ++i) RC(weight_grad(deferred[i], def_dy[i], def_cm[i], stream));
    // join: the side stream's gradients are complete before the caller's stream goes on
    RC(fork(side, main));
    if (a.ray_grad) RC(encode_bwd(a, w, stream));
    return NERF_OK;
}

// The schedule with the input-gradient chain (bwd_chain): dyr and the nine input gradients in
// one launch (nerf_mlp_chain_bwd) on the caller's stream; then every layer's weight gradient on
// the caller's stream (each 4-wave TN launch fills the chip on its own) with its split-K
// reduce on the side stream behind an event, so a reduce runs beside the next layer's TN; the
// ray gradients (pose learning) as three input-gradient GEMMs over the saved dy of the colour
// layer, l4 and l0.  The head-weight partials were placed before the chain (but NERF_HEADS_PLACE=2);
// `batch` holds placement 3's two head-weight reduces: they ride in the first slab batch.
int chain_schedule(const nerf_field_bwd& a, Work& w, const float* graw4, void* stream, void* side_stream,
                   const Knobs& k, SlabBatch& batch) {
    const int np = a.n_pad;
    hipStream_t main = nerf::as_stream(stream), side = nerf::as_stream(side_stream);
    nerf_chain_bwd c = chain_desc(a, graw4);
    c.dy[0] = w.dyr; c.lddy[0] = HR; c.dy_cmax[0] = w.dyr_cm; c.dy_rmax[0] = w.dyr_rm;
    for (int i = 1; i < 10; ++i) {   // every D_i is stored: the weight gradients read them (dy_of)
        const int l = 10 - i;
        c.dy[i] = w.dx[l]; c.lddy[i] = K1[l]; c.dy_cmax[i] = w.dx_cm[l]; c.dy_rmax[i] = w.dx_rm[l];
    }
    c.scratch = w.scratch;
    RC(nerf_mlp_chain_bwd(&c, stream));
    if (k.heads_place == 2) RC(heads(a, w, graw4, main, main));   // (A/B only) behind the chain
    auto enc = [&](int l) -> int {
        const Grad g = dy_of(w, l);
        return a.ray_grad ? enc_rows(a, w, l, g.dy, g.rm, stream) : NERF_OK;
    };
    if (k.sched == 3) {
        // every weight gradient as a job of one of two k_wgrad_jobs launches (2 S blocks, S the
        // 256 x 256 layers' split count; the narrow tiles fill the same grid instead of a launch
        // of their own): the colour layer's two segments + l_f .. l5, then l4's two segments +
        // l3 .. l1 + l0.  Same splits and slab columns as schedule 1, so the same slabs.  Each
        // launch's slab reduces follow it on the caller's stream.
        nerf_wgrad_tile_job tj[nerf::kWgradJobsMax];
        int tgrp[nerf::kWgradJobsMax];
        int nt = 0, cur_grp = 0;
        // layer l's main segment (x = its input; l0: enc_p) and, for l4 / the colour layer, the
        // 64-wide encoding segment at slab column K1[l]
        auto tiles = [&](int l) {
            const Grad g = dy_of(w, l);
            const Input x = x_of(a, l);
            const int op = OUT_P[l];
            tgrp[nt] = cur_grp;
            tj[nt++] = nerf_wgrad_tile_job{g.dy, op, op, x.x, K1[l], K1[l], w.splits[l], w.slab[l], KP[l], 0, w.bslab[l],
                                           g.cm, x.cm};
            if (SEG[l]) {
                const Input e = enc_of(a, l);
                tgrp[nt] = cur_grp;
                tj[nt++] = nerf_wgrad_tile_job{g.dy, op, op, e.x, 64, 64, w.splits[l], w.slab[l], KP[l], K1[l], nullptr,
                                               g.cm, e.cm};
            }
            batch.add(a, w, l);
        };
        // one launch.  Grouped, at S / 2 splits: `seg` (lr or l4: a layer with an encoding segment) and
        // the layers of `g0` as group 0, seg's encoding segment and the layers of `g1` as group 1; else one
        // job list, `flat`
        const int s2 = w.splits[LF] / 2;
        auto launch = [&](bool grouped, int seg, std::initializer_list<int> g0, std::initializer_list<int> g1,
                          std::initializer_list<int> flat) -> int {
            if (grouped) {
                tiles(seg);
                tgrp[nt - 1] = 1;   // the job just added: seg's encoding segment
                for (int l : g0) tiles(l);
                cur_grp = 1;
                for (int l : g1) tiles(l);
                cur_grp = 0;
                RC(nerf_linear_bwd_weight_job_groups(tj, tgrp, nt, np, s2, 2, stream));
            } else {
                for (int l : flat) tiles(l);
                RC(nerf_linear_bwd_weight_jobs(tj, nt, np, w.splits[LF], stream));
            }
            nt = 0;
            return NERF_OK;
        };
        const int groups = w.splits[LF] % 16 == 0 ? k.groups : 0;
        // a grouped launch halves its layers' split counts in place first; the slab buffers are sized
        // for S: room to spare
        if (groups >= 2) {
            for (int l : {LF, 7, 6, 5}) w.splits[l] = s2;
            w.splits[LR] = 2 * s2;
        }
        // group 0 the colour layer's f segment + l_f + l7, group 1 its enc_d segment + l6 + l5
        // (5 vs 4.5 1024-row tile-times per block against 4.75 in one list, three jobs each
        // instead of six)
        RC(launch(groups >= 2, LR, {LF, 7}, {6, 5}, {LR, LF, 7, 6, 5}));
        if (k.batch1 != 2) RC(batch.flush(main, k.batch1 == 0 ? side : main));
        RC(enc(LR));
        if (groups >= 1) {
            for (int l : {1, 2, 3, 4}) w.splits[l] = s2;
            w.splits[0] = 2 * s2;
        }
        // group 0 l4's h3 segment + l3 + l0, group 1 l4's enc_p segment + l2 + l1 (4.83 / 5
        // tile-times): with groups k_wgrad_jobs runs a group's narrow jobs before its pairs, so the
        // two reads of l4's dy start together (group 0's first job and group 1's): 1.8580 vs 1.8677
        // ms per cfg2 step (profiles/r06/wgrad_l4_groups_ab.txt); ungrouped l4's h3 job is the last
        // 256 x 256 one: its enc_p job follows
        RC(launch(groups >= 1, 4, {3, 0}, {2, 1}, {3, 2, 1, 4, 0}));
        RC(batch.flush(main, main));
        RC(enc(4));
        RC(enc(0));
    } else if (k.sched == 2) {
        // the weight gradients back to back on the caller's stream (each needs only the chain's
        // saved dy): the colour layer's two segments (f, enc_d) as two launches; l_f .. l1 -- with
        // l4's h3 segment -- as ONE launch (k_wgrad_pairs: a block walks the eight 256 x 256
        // layers); l4's enc_p segment and l0 as one launch (both 256 x 64 over enc_p). The slab
        // reduces: every layer but l4 and l0 on the side stream after the eight-layer launch (beside
        // the last one), l4's and l0's on the caller's stream at the end (a cross-stream event costs
        // ~7 us of idle on the stream that records it; one fork per layer was ~80 us per step)
        {   // the colour layer: [f | enc_d]
            const Grad g = dy_of(w, LR);
            RC(nerf_linear_bwd_weight(g.dy, HR, HR, a.act[LF], K1[LR], K1[LR], np, w.splits[LR], w.slab[LR], KP[LR], 0,
                                      w.bslab[LR], g.cm, a.cmax[LF], stream));
            RC(nerf_linear_bwd_weight(g.dy, HR, HR, a.enc_d, 64, 64, np, w.splits[LR], w.slab[LR], KP[LR], K1[LR], nullptr,
                                      g.cm, a.enc_d_cmax, stream));
            batch.add(a, w, LR);
            RC(enc(LR));
        }
        {   // l_f .. l1 (l4: its h3 segment) in one launch
            nerf_wgrad_job wj[nerf::kWgradPairsMax];
            int n = 0;
            for (int l = LF; l >= 1; --l) {
                const Grad g = dy_of(w, l);
                NERF_CHECK(OUT_P[l] == D && K1[l] == D && w.splits[l] == w.splits[LF], "layer %d", l);
                wj[n++] = nerf_wgrad_job{g.dy, D, a.act[l - 1], D, w.slab[l], KP[l], w.bslab[l], g.cm, a.cmax[l - 1]};
                if (l != 4) batch.add(a, w, l);
            }
            RC(nerf_linear_bwd_weight_multi(wj, n, np, w.splits[LF], stream));
        }
        RC(batch.flush(main, side));
        {   // l4's enc_p segment and l0 in one launch
            const Grad g4 = dy_of(w, 4), g0 = dy_of(w, 0);
            RC(nerf::wgrad_narrow_pair(g4.dy, D, a.enc_p, 64, w.splits[4], w.slab[4], KP[4], K1[4], nullptr, g4.cm,
                                       a.enc_p_cmax, g0.dy, D, a.enc_p, 64, w.splits[0], w.slab[0], KP[0], 0, w.bslab[0],
                                       g0.cm, a.enc_p_cmax, np, main));
            batch.add(a, w, 4);
            batch.add(a, w, 0);
            RC(enc(4));
            RC(enc(0));
        }
        RC(batch.flush(main, main));
    } else {
        // the weight gradients back to back on the caller's stream (each needs only the chain's
        // saved dy): the colour layer (two segments), l_f .. l5 in one launch, l4 (two segments),
        // l3 .. l1 in one launch, l0. Their slab reduces are batched: lr .. l5 on the side stream
        // after l5's (beside l4 .. l1's), l4 .. l1 on the side stream after l1's (beside l0's),
        // l0's on the caller's stream at the end (a cross-stream event costs ~7 us of idle on the
        // stream that records it, and the join another; one fork per layer was ~80 us per step)
        // one layer's weight gradient (+ its encoding-row input gradient for ray gradients)
        auto single = [&](int l) -> int {
            const Grad g = dy_of(w, l);
            RC(wgrad_launch(a, w, l, g.dy, g.cm, stream));
            batch.add(a, w, l);
            return enc(l);
        };
        // the 256 x 256 layers hi .. lo (descending) in one launch
        auto pairs = [&](int hi, int lo) -> int {
            nerf_wgrad_job wj[nerf::kWgradPairsMax];
            int n = 0;
            for (int l = hi; l >= lo; --l) {
                const Grad g = dy_of(w, l);
                const Input x = x_of(a, l);
                NERF_CHECK(!SEG[l] && OUT_P[l] == D && K1[l] == D && w.splits[l] == w.splits[hi], "layer %d", l);
                wj[n++] = nerf_wgrad_job{g.dy, OUT_P[l], x.x, K1[l], w.slab[l], KP[l], w.bslab[l], g.cm, x.cm};
                batch.add(a, w, l);
            }
            return nerf_linear_bwd_weight_multi(wj, n, np, w.splits[hi], stream);
        };
        RC(single(LR));
        RC(pairs(LF, 5));
        RC(batch.flush(main, side));
        RC(single(4));
        RC(pairs(3, 1));
        RC(batch.flush(main, side));
        RC(single(0));
        RC(batch.flush(main, main));
    }
    if (a.ray_grad) RC(encode_bwd(a, w, stream));
    RC(fork(side, main));
    return NERF_OK;
}

// nerf_field_backward but for its error exit; its messages print this function's name
int schedule(const nerf_field_bwd& a, void* stream, void* side_stream) {
    const int np = a.n_pad;
    NERF_CHECK(np > 0 && np % 128 == 0 && a.workspace && side_stream && stream != side_stream,
               "%s: n_pad=%d (a positive multiple of 128), a workspace and a second stream are required", __func__, np);
    RC(check_precision(__func__));
    NERF_CHECK(a.tail_main >= 0 && a.tail_main <= L, "%s: tail_main=%d", __func__, a.tail_main);
    NERF_CHECK(a.graw4 || (a.g_rgb && a.g_dist && a.z && a.raw4), "%s: need graw4 or (g_rgb, g_dist, raw4, z)",
               __func__);
    for (int l = 0; l < L; ++l) {
        NERF_CHECK(a.act[l] && a.wt[l] && a.wt_img[l] && a.gw[l] && a.gb[l], "%s: layer %d: missing tensor", __func__,
                   l);
        RC(check_layer(a, l, a.bwd_chain, __func__));
        NERF_CHECK((l == LR) == (a.cmax[l] == nullptr), "%s: layer %d: column maxima (none for the colour layer)",
                   __func__, l);
    }
    NERF_CHECK(a.enc_p && a.enc_d && a.enc_p_cmax && a.enc_d_cmax && a.wd && a.wc && a.g_wd && a.g_bd && a.g_wc &&
                   a.g_bc,
               "%s: missing encoding / head tensor", __func__);
    NERF_CHECK(!a.ray_grad || (a.pts_o && a.pts_d && a.view && a.z && a.g_pts_o && a.g_pts_d && a.g_view),
               "%s: ray gradients need pts_o / pts_d / view / z and their gradient outputs", __func__);
    Work w;
    carve(reinterpret_cast<char*>(a.workspace), np, a.ray_grad, w);
    hipStream_t main = nerf::as_stream(stream), side = nerf::as_stream(side_stream);
    g_events.next = 0;

    const float* graw4;
    RC(upstream(a, w.graw4, stream, graw4));
    if (!a.bwd_chain) {
        RC(fork(main, side));
        RC(heads(a, w, graw4, side, side));
        return per_layer_schedule(a, w, graw4, stream, side_stream);
    }
    const Knobs k = read_knobs();
    SlabBatch batch;
    if (k.heads_place == 0) {
        RC(fork(main, side));
        RC(heads(a, w, graw4, side, side));
    } else if (k.heads_place == 1) {
        RC(heads(a, w, graw4, main, main));
    } else if (k.heads_place == 5) {
        RC(heads(a, w, graw4, main, side));
    } else if (k.heads_place == 3) {
        nerf::SlabJobDesc hjobs[2];   // the partials by k_heads_part; their reduces ride in the first slab batch
        RC(nerf::heads_partials(graw4, a.act[7], D, a.act[LR], HR, np, w.hpart, a.g_wd, a.g_bd, a.g_wc, a.g_bc, hjobs,
                                main));
        for (const nerf::SlabJobDesc& j : hjobs) batch.jobs[batch.n++] = j;
    }
    return chain_schedule(a, w, graw4, stream, side_stream, k, batch);
}

}  // namespace

extern "C" size_t nerf_field_bwd_workspace_bytes(int n_pad, int ray_grad) {
    if (n_pad <= 0 || n_pad % 128) return 0;
    Work w;
    return carve(nullptr, n_pad, ray_grad, w);
}

extern "C" int nerf_field_backward(const nerf_field_bwd* ap, void* stream, void* side_stream) {
    NERF_CHECK_PTR(ap);
    const int rc = schedule(*ap, stream, side_stream);
    if (rc == NERF_OK || !side_stream || stream == side_stream) return rc;
    // a launch failed part-way: the side stream may still run weight-gradient kernels on the
    // workspace; join it into the caller's stream on this exit too, so the caller's allocator
    // cannot hand the workspace out again while they write it (the error code is kept)
    hipEvent_t e = g_events.get();
    if (e && hipEventRecord(e, nerf::as_stream(side_stream)) == hipSuccess)
        (void)hipStreamWaitEvent(nerf::as_stream(stream), e, 0);
    return rc;
}

// ---------------------------------------------------------------------------
// The ray-gradient-only backward of a frozen field (nerf_field_backward_rays): the part of
// chain_schedule that reaches pts_o / pts_d / view, for a step that optimises only what
// produces the rays (test-time pose refinement: eval_pose_one_epoch.py:30-76 steps
// optimizer_pose alone).  No weight gradient, slab reduce or head-weight partial runs, so
// nothing reads a saved layer output or a column maximum: the chain stores only the three dy
// the encoding segments read and everything is on the caller's stream.
extern "C" size_t nerf_field_bwd_rays_workspace_bytes(int n_pad) {
    if (n_pad <= 0 || n_pad % 128) return 0;
    RaysWork w;
    return carve_rays(nullptr, n_pad, w);
}

extern "C" int nerf_field_backward_rays(const nerf_field_bwd_rays* ap, void* stream) {
    NERF_CHECK_PTR(ap);
    const nerf_field_bwd_rays& a = *ap;
    const int np = a.n_pad;
    NERF_CHECK(np > 0 && np % 128 == 0 && a.workspace, "%s: n_pad=%d (a positive multiple of 128) and a workspace "
               "(nerf_field_bwd_rays_workspace_bytes) are required", __func__, np);
    RC(check_precision(__func__));
    NERF_CHECK(a.graw4 || (a.g_rgb && a.g_dist && a.raw4), "%s: need graw4 or (g_rgb, g_dist, raw4)", __func__);
    for (int l = 0; l < L; ++l) RC(check_layer(a, l, true, __func__));
    for (int l : {0, 4, LR})
        NERF_CHECK(a.wt[l] && a.wt_img[l], "%s: layer %d: W^T and its fp16 pair image (the encoding rows' operand)",
                   __func__, l);
    NERF_CHECK(a.wd && a.wc, "%s: missing head weights", __func__);
    NERF_CHECK(a.pts_o && a.pts_d && a.view && a.z && a.g_pts_o && a.g_pts_d && a.g_view,
               "%s: pts_o / pts_d / view / z and the three gradient outputs are required", __func__);
    RaysWork w;
    carve_rays(reinterpret_cast<char*>(a.workspace), np, w);

    const float* graw4;
    RC(upstream(a, w.graw4, stream, graw4));
    nerf_chain_bwd c = chain_desc(a, graw4);
    // D_0 = dyr, D_5 the gradient at l4's output, D_9 at l0's
    c.dy[0] = w.d0; c.lddy[0] = HR; c.dy_rmax[0] = w.rm0;
    c.dy[5] = w.d5; c.lddy[5] = D; c.dy_rmax[5] = w.rm5;
    c.dy[9] = w.d9; c.lddy[9] = D; c.dy_rmax[9] = w.rm9;
    RC(nerf_mlp_chain_bwd_rays(&c, stream));
    RC(enc_rows(a, w, LR, w.d0, w.rm0, stream));
    RC(enc_rows(a, w, 4, w.d5, w.rm5, stream));
    RC(enc_rows(a, w, 0, w.d9, w.rm9, stream));
    return encode_bwd(a, w, stream);
}
