// Launch-trace harness of the field backward executor (csrc/field_bwd.cpp): a stand-alone host
// program, compiled host-only together with that file and linked WITHOUT the HIP runtime.  Every
// nerf_* entry, nerf:: internal and HIP event function the executor calls is a stub here that
// prints one line -- the callee, the stream (main / side), scalars in decimal, pointers
// symbolically (null, ws+<bytes> inside the workspace, <name>+<bytes> from a table of fake,
// widely spaced, never dereferenced addresses).  The driver runs a fixed list of cases in one
// process (the event pool's reuse across calls is part of the behaviour) and prints
//   == <case>            the trace lines            return rc=<rc> launches=<n>
// tests/test_field_bwd_trace.py compares the output case by case with tests/golden/.
#include "../../my-nope-nerf_amd/csrc/common.hpp"

#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace {

// ---- fake addresses ---------------------------------------------------------------------
constexpr uintptr_t kFakeBase = uintptr_t(1) << 44, kFakeStride = uintptr_t(1) << 36;
constexpr uintptr_t kWsBase = uintptr_t(3) << 45;
std::vector<std::string> g_names;
size_t g_ws_bytes = 0;
void* const kMain = reinterpret_cast<void*>(0x1000);
void* const kSide = reinterpret_cast<void*>(0x2000);

template <class T>
T* fake(const std::string& name) {
    g_names.push_back(name);
    return reinterpret_cast<T*>(kFakeBase + (g_names.size() - 1) * kFakeStride);
}

std::string sym(const void* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (!a) return "null";
    if (a >= kWsBase && a < kWsBase + g_ws_bytes) return "ws+" + std::to_string(a - kWsBase);
    if (a >= kFakeBase && a < kFakeBase + g_names.size() * kFakeStride)
        return g_names[(a - kFakeBase) / kFakeStride] + "+" + std::to_string((a - kFakeBase) % kFakeStride);
    return "?" + std::to_string(a);
}

std::string strm(const void* s) { return s == kMain ? "main" : s == kSide ? "side" : s ? "?stream" : "null"; }

// ---- the trace --------------------------------------------------------------------------
int g_launches = 0;       // launch stubs called in this case
int g_fail_at = 0;        // the k-th launch stub of the case returns NERF_ELAUNCH (0: none)
int g_splits = 64;        // nerf_linear_bwd_weight_splits of the 256 x 256 layers
int g_precision = 2;
bool g_fail_event_create = false;
int g_event_records = 0, g_fail_event_record_at = 0;
int g_events_made = 0;
bool g_quiet = false;     // the driver's own size queries print nothing

struct Line {
    std::string s;
    explicit Line(const char* callee) : s(callee) {}
    Line(const char* callee, const void* stream) : s(callee) { s += " " + strm(stream); }
    Line& i(const char* k, long long v) { s += std::string(" ") + k + "=" + std::to_string(v); return *this; }
    Line& p(const char* k, const void* v) { s += std::string(" ") + k + "=" + sym(v); return *this; }
    Line& t(const std::string& text) { s += " " + text; return *this; }
    ~Line() {
        if (!g_quiet) std::puts(s.c_str());
    }
};

int launched() {
    ++g_launches;
    if (g_launches == g_fail_at) {
        std::puts("  -> NERF_ELAUNCH");
        return NERF_ELAUNCH;
    }
    return NERF_OK;
}

std::string ev_name(hipEvent_t e) { return "ev" + std::to_string(reinterpret_cast<uintptr_t>(e) - 0xE0000); }

void put_slab_job(int i, const nerf::SlabJobDesc& d) {
    Line("  slab_job").i("#", i).p("slab", d.slab).i("splits", d.splits).i("nout", d.nout).i("ldslab", d.ldslab)
        .i("nout_ref", d.nout_ref).i("kin_ref", d.kin_ref).p("bslab", d.bslab).p("gw", d.gw).p("gb", d.gb);
}

void put_tile_job(int i, const nerf_wgrad_tile_job& j, int group) {
    Line("  tile_job").i("#", i).i("group", group).p("dy", j.dy).i("lddy", j.lddy).i("nout", j.nout).p("x", j.x)
        .i("ldx", j.ldx).i("kin", j.kin).i("splits", j.splits).p("slab", j.slab).i("ldslab", j.ldslab).i("col0", j.col0)
        .p("bslab", j.bslab).p("dy_cmax", j.dy_cmax).p("x_cmax", j.x_cmax);
}

void put_chain(const nerf_chain_bwd* c) {
    if (!c) return;
    Line("  chain").p("graw4", c->graw4).p("hr_mask", c->hr_mask).i("ld_hr_mask", c->ld_hr_mask).p("wd", c->wd)
        .p("wc", c->wc).p("scratch", c->scratch).i("n_pad", c->n_pad);
    for (int i = 0; i < 9; ++i)
        Line("  chain.layer").i("#", i).p("wt_img", c->wt_img[i]).i("wt_img_rows", c->wt_img_rows[i])
            .p("in_mask", c->in_mask[i]).i("ld_in_mask", c->ld_in_mask[i]);
    for (int i = 0; i < 10; ++i)
        Line("  chain.dy").i("#", i).p("dy", c->dy[i]).i("lddy", c->lddy[i]).p("dy_cmax", c->dy_cmax[i])
            .p("dy_rmax", c->dy_rmax[i]);
}

}  // namespace

// ---- entry-point stubs (signatures from include/nerf_hip.h) -----------------------------
extern "C" {

int nerf_composite_bwd(const float* raw4, const float* z, int n_rays, int n_samples, int flags, const float* grad_rgb,
                       const float* grad_dist, float* graw4, int n_pad, void* stream) {
    Line("nerf_composite_bwd", stream).p("raw4", raw4).p("z", z).i("n_rays", n_rays).i("n_samples", n_samples)
        .i("flags", flags).p("grad_rgb", grad_rgb).p("grad_dist", grad_dist).p("graw4", graw4).i("n_pad", n_pad);
    return launched();
}

int nerf_encode_bwd(const float* pts_o, const float* pts_d, const float* view, const float* z, const float* genc_p,
                    const float* genc_p2, const float* genc_d, int n_rays, int n_samples, float* g_pts_o,
                    float* g_pts_d, float* g_view, void* stream) {
    Line("nerf_encode_bwd", stream).p("pts_o", pts_o).p("pts_d", pts_d).p("view", view).p("z", z).p("genc_p", genc_p)
        .p("genc_p2", genc_p2).p("genc_d", genc_d).i("n_rays", n_rays).i("n_samples", n_samples).p("g_pts_o", g_pts_o)
        .p("g_pts_d", g_pts_d).p("g_view", g_view);
    return launched();
}

int nerf_heads_bwd_mode(int mode, const float* graw4, const float* h8, int ld8, const float* hr, int ldr,
                        const uint32_t* hr_mask, int ldm, int hidden, const float* wc, float* dyr, int lddyr,
                        float* part, int n_pad, float* dyr_rmax, float* dyr_cmax, void* stream) {
    Line("nerf_heads_bwd_mode", stream).i("mode", mode).p("graw4", graw4).p("h8", h8).i("ld8", ld8).p("hr", hr)
        .i("ldr", ldr).p("hr_mask", hr_mask).i("ldm", ldm).i("hidden", hidden).p("wc", wc).p("dyr", dyr)
        .i("lddyr", lddyr).p("part", part).i("n_pad", n_pad).p("dyr_rmax", dyr_rmax).p("dyr_cmax", dyr_cmax);
    return launched();
}

int nerf_heads_reduce(const float* part, int hidden, int n_pad, float* gwd, float* gbd, float* gwc, float* gbc,
                      int accumulate, void* stream) {
    Line("nerf_heads_reduce", stream).p("part", part).i("hidden", hidden).i("n_pad", n_pad).p("gwd", gwd).p("gbd", gbd)
        .p("gwc", gwc).p("gbc", gbc).i("accumulate", accumulate);
    return launched();
}

int nerf_heads_part_size(int hidden, int n_pad) {
    const int r = (n_pad + 255) / 256 * (hidden * 5 / 2 + 4);
    Line("nerf_heads_part_size").i("hidden", hidden).i("n_pad", n_pad).i("->", r);
    return r;
}

int nerf_linear_bwd_data(const float* dy, int lddy, int k, const float* wt, const uint16_t* wt_split, int wt_split_rows,
                         const float* u, int ldu, const float* v, const uint32_t* mask, int ldmask, float* dx, int lddx,
                         int m, int n, const float* dy_rmax, float* dx_rmax, float* dx_cmax, void* stream) {
    Line("nerf_linear_bwd_data", stream).p("dy", dy).i("lddy", lddy).i("k", k).p("wt", wt).p("wt_split", wt_split)
        .i("wt_split_rows", wt_split_rows).p("u", u).i("ldu", ldu).p("v", v).p("mask", mask).i("ldmask", ldmask)
        .p("dx", dx).i("lddx", lddx).i("m", m).i("n", n).p("dy_rmax", dy_rmax).p("dx_rmax", dx_rmax)
        .p("dx_cmax", dx_cmax);
    return launched();
}

int nerf_linear_bwd_weight(const float* dy, int lddy, int nout, const float* x, int ldx, int kin, int m, int splits,
                           float* slab, int ldslab, int col0, float* bslab, const float* dy_cmax, const float* x_cmax,
                           void* stream) {
    Line("nerf_linear_bwd_weight", stream).p("dy", dy).i("lddy", lddy).i("nout", nout).p("x", x).i("ldx", ldx)
        .i("kin", kin).i("m", m).i("splits", splits).p("slab", slab).i("ldslab", ldslab).i("col0", col0)
        .p("bslab", bslab).p("dy_cmax", dy_cmax).p("x_cmax", x_cmax);
    return launched();
}

int nerf_linear_bwd_weight_seg(const float* dy, int lddy, int nout, const float* x1, int ldx1, int k1, const float* x2,
                               int ldx2, int k2, int m, int splits, float* slab, int ldslab, float* bslab,
                               const float* dy_cmax, const float* x1_cmax, const float* x2_cmax, void* stream) {
    Line("nerf_linear_bwd_weight_seg", stream).p("dy", dy).i("lddy", lddy).i("nout", nout).p("x1", x1).i("ldx1", ldx1)
        .i("k1", k1).p("x2", x2).i("ldx2", ldx2).i("k2", k2).i("m", m).i("splits", splits).p("slab", slab)
        .i("ldslab", ldslab).p("bslab", bslab).p("dy_cmax", dy_cmax).p("x1_cmax", x1_cmax).p("x2_cmax", x2_cmax);
    return launched();
}

int nerf_linear_bwd_weight_multi(const nerf_wgrad_job* jobs, int n, int m, int splits, void* stream) {
    Line("nerf_linear_bwd_weight_multi", stream).i("n", n).i("m", m).i("splits", splits);
    for (int i = 0; jobs && i < n; ++i)
        Line("  wgrad_job").i("#", i).p("dy", jobs[i].dy).i("lddy", jobs[i].lddy).p("x", jobs[i].x).i("ldx", jobs[i].ldx)
            .p("slab", jobs[i].slab).i("ldslab", jobs[i].ldslab).p("bslab", jobs[i].bslab)
            .p("dy_cmax", jobs[i].dy_cmax).p("x_cmax", jobs[i].x_cmax);
    return launched();
}

int nerf_linear_bwd_weight_jobs(const nerf_wgrad_tile_job* jobs, int n, int m, int splits, void* stream) {
    Line("nerf_linear_bwd_weight_jobs", stream).i("n", n).i("m", m).i("splits", splits);
    for (int i = 0; jobs && i < n; ++i) put_tile_job(i, jobs[i], 0);
    return launched();
}

int nerf_linear_bwd_weight_job_groups(const nerf_wgrad_tile_job* jobs, const int* group, int n, int m, int splits,
                                      int n_groups, void* stream) {
    Line("nerf_linear_bwd_weight_job_groups", stream).i("n", n).i("m", m).i("splits", splits).i("n_groups", n_groups)
        .t(group ? "group=given" : "group=null");
    for (int i = 0; jobs && i < n; ++i) put_tile_job(i, jobs[i], group ? group[i] : 0);
    return launched();
}

int nerf_linear_bwd_weight_splits(int nout, int kin, int m) {
    const int r = nout == 256 && kin == 256 ? g_splits : 2 * g_splits;
    Line("nerf_linear_bwd_weight_splits").i("nout", nout).i("kin", kin).i("m", m).i("->", r);
    return r;
}

int nerf_slab_reduce(const float* slab, int splits, int nout, int ldslab, int nout_ref, int kin_ref, const float* bslab,
                     float* gw, float* gb, int accumulate, void* stream) {
    Line("nerf_slab_reduce", stream).p("slab", slab).i("splits", splits).i("nout", nout).i("ldslab", ldslab)
        .i("nout_ref", nout_ref).i("kin_ref", kin_ref).p("bslab", bslab).p("gw", gw).p("gb", gb)
        .i("accumulate", accumulate);
    return launched();
}

int nerf_mlp_chain_bwd(const nerf_chain_bwd* a, void* stream) {
    Line("nerf_mlp_chain_bwd", stream).t(a ? "a=given" : "a=null");
    put_chain(a);
    return launched();
}

int nerf_mlp_chain_bwd_rays(const nerf_chain_bwd* a, void* stream) {
    Line("nerf_mlp_chain_bwd_rays", stream).t(a ? "a=given" : "a=null");
    put_chain(a);
    return launched();
}

// ---- HIP event stubs ----------------------------------------------------------------------
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags) {
    if (g_fail_event_create) {
        Line("hipEventCreateWithFlags").i("flags", flags).t("-> hipErrorOutOfMemory");
        return hipErrorOutOfMemory;
    }
    *event = reinterpret_cast<hipEvent_t>(uintptr_t(0xE0000 + g_events_made++));
    Line("hipEventCreateWithFlags").t(ev_name(*event)).i("flags", flags);
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    Line l("hipEventRecord", stream);
    l.t(ev_name(event));
    if (++g_event_records == g_fail_event_record_at) {
        l.t("-> hipErrorInvalidValue");
        return hipErrorInvalidValue;
    }
    return hipSuccess;
}

hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned flags) {
    Line("hipStreamWaitEvent", stream).t(ev_name(event)).i("flags", flags);
    return hipSuccess;
}

}  // extern "C"

// ---- internal stubs (csrc/common.hpp) -------------------------------------------------------
namespace nerf {

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::printf("set_error \"%s\"\n", buf);
}

int gemm_precision() {
    Line("gemm_precision").i("->", g_precision);
    return g_precision;
}

int heads_part_blocks(int n) {
    const int r = (n + 1023) / 1024;
    Line("heads_part_blocks").i("n", n).i("->", r);
    return r;
}

int heads_partials(const float* graw4, const float* h8, int ld8, const float* hr, int ldr, int n, float* part, float* gwd,
                   float* gbd, float* gwc, float* gbc, SlabJobDesc (&jobs)[2], hipStream_t s) {
    Line("heads_partials", s).p("graw4", graw4).p("h8", h8).i("ld8", ld8).p("hr", hr).i("ldr", ldr).i("n", n)
        .p("part", part).p("gwd", gwd).p("gbd", gbd).p("gwc", gwc).p("gbc", gbc);
    jobs[0] = SlabJobDesc{part, 7001, 7002, 7003, 7004, 7005, part + 1, gwd, gbd};
    jobs[1] = SlabJobDesc{part + 2, 7011, 7012, 7013, 7014, 7015, part + 3, gwc, gbc};
    return launched();
}

int slab_reduce_jobs(const SlabJobDesc* d, int n, hipStream_t s) {
    Line("slab_reduce_jobs", s).i("n", n);
    for (int i = 0; d && i < n; ++i) put_slab_job(i, d[i]);
    return launched();
}

int wgrad_narrow_pair(const float* dy_a, int lddy_a, const float* x_a, int ldx_a, int splits_a, float* slab_a,
                      int ldslab_a, int col0_a, float* bslab_a, const float* dcm_a, const float* xcm_a, const float* dy_b,
                      int lddy_b, const float* x_b, int ldx_b, int splits_b, float* slab_b, int ldslab_b, int col0_b,
                      float* bslab_b, const float* dcm_b, const float* xcm_b, int m, hipStream_t s) {
    Line("wgrad_narrow_pair", s).p("dy_a", dy_a).i("lddy_a", lddy_a).p("x_a", x_a).i("ldx_a", ldx_a)
        .i("splits_a", splits_a).p("slab_a", slab_a).i("ldslab_a", ldslab_a).i("col0_a", col0_a).p("bslab_a", bslab_a)
        .p("dcm_a", dcm_a).p("xcm_a", xcm_a).p("dy_b", dy_b).i("lddy_b", lddy_b).p("x_b", x_b).i("ldx_b", ldx_b)
        .i("splits_b", splits_b).p("slab_b", slab_b).i("ldslab_b", ldslab_b).i("col0_b", col0_b).p("bslab_b", bslab_b)
        .p("dcm_b", dcm_b).p("xcm_b", xcm_b).i("m", m);
    return launched();
}

}  // namespace nerf

// ---- the driver -----------------------------------------------------------------------------
namespace {

constexpr int L = NERF_BWD_LAYERS;
constexpr int kRays = 520, kSamples = 128, kNp = kRays * kSamples;   // 66560: no power of two

std::string idx(const char* name, int l) { return std::string(name) + "[" + std::to_string(l) + "]"; }

nerf_field_bwd g_full;        // every pointer set (mask[8] and cmax[9] null, as the entry wants)
nerf_field_bwd_rays g_rays;

void make_args() {
    nerf_field_bwd& a = g_full;
    a = nerf_field_bwd{};
    a.n_pad = kNp; a.n_rays = kRays; a.n_samples = kSamples; a.flags = 5;
    a.z = fake<float>("z"); a.raw4 = fake<float>("raw4");
    a.enc_p = fake<float>("enc_p"); a.enc_d = fake<float>("enc_d");
    a.enc_p_cmax = fake<float>("enc_p_cmax"); a.enc_d_cmax = fake<float>("enc_d_cmax");
    for (int l = 0; l < L; ++l) {
        a.act[l] = fake<float>(idx("act", l));
        a.mask[l] = l == 8 ? nullptr : fake<uint32_t>(idx("mask", l));
        a.cmax[l] = l == 9 ? nullptr : fake<float>(idx("cmax", l));
        a.wt[l] = fake<float>(idx("wt", l));
        a.wt_img[l] = fake<uint16_t>(idx("wt_img", l));
        a.wt_cimg[l] = fake<uint16_t>(idx("wt_cimg", l));
        a.gw[l] = fake<float>(idx("gw", l));
        a.gb[l] = fake<float>(idx("gb", l));
    }
    a.pts_o = fake<float>("pts_o"); a.pts_d = fake<float>("pts_d"); a.view = fake<float>("view");
    a.wd = fake<float>("wd"); a.wc = fake<float>("wc");
    a.g_rgb = fake<float>("g_rgb"); a.g_dist = fake<float>("g_dist"); a.graw4 = fake<float>("graw4");
    a.g_wd = fake<float>("g_wd"); a.g_bd = fake<float>("g_bd"); a.g_wc = fake<float>("g_wc"); a.g_bc = fake<float>("g_bc");
    a.g_pts_o = fake<float>("g_pts_o"); a.g_pts_d = fake<float>("g_pts_d"); a.g_view = fake<float>("g_view");
    a.workspace = reinterpret_cast<void*>(kWsBase);

    nerf_field_bwd_rays& r = g_rays;
    r = nerf_field_bwd_rays{};
    r.n_pad = kNp; r.n_rays = kRays; r.n_samples = kSamples; r.flags = 5;
    r.z = a.z; r.raw4 = a.raw4; r.pts_o = a.pts_o; r.pts_d = a.pts_d; r.view = a.view;
    for (int l = 0; l < L; ++l) {
        r.mask[l] = a.mask[l]; r.wt[l] = a.wt[l]; r.wt_img[l] = a.wt_img[l]; r.wt_cimg[l] = a.wt_cimg[l];
    }
    r.wd = a.wd; r.wc = a.wc; r.g_rgb = a.g_rgb; r.g_dist = a.g_dist; r.graw4 = a.graw4;
    r.g_pts_o = a.g_pts_o; r.g_pts_d = a.g_pts_d; r.g_view = a.g_view;
    r.workspace = a.workspace;
}

const char* const kKnobs[] = {"NERF_WGRAD_SCHED", "NERF_WGRAD_GROUPS", "NERF_WGRAD_BATCH1", "NERF_HEADS_PLACE"};

// knobs: "SCHED=3 GROUPS=1" style (names without the NERF_ / NERF_WGRAD_ prefix); unset otherwise
void set_knobs(const std::string& spec) {
    for (const char* k : kKnobs) unsetenv(k);
    size_t at = 0;
    while (at < spec.size()) {
        size_t end = spec.find(' ', at);
        if (end == std::string::npos) end = spec.size();
        const std::string kv = spec.substr(at, end - at);
        const size_t eq = kv.find('=');
        const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
        setenv((k == "HEADS_PLACE" ? "NERF_" + k : "NERF_WGRAD_" + k).c_str(), v.c_str(), 1);
        at = end + 1;
    }
}

struct Case {
    int splits = 64, precision = 2, fail_at = 0;
    bool fail_event_create = false;
    int fail_event_record_at = 0;
    std::string knobs;
};

void begin(const std::string& name, const Case& c) {
    std::printf("== %s\n", name.c_str());
    g_splits = c.splits; g_precision = c.precision; g_fail_at = c.fail_at;
    g_fail_event_create = c.fail_event_create;
    g_fail_event_record_at = c.fail_event_record_at;
    g_event_records = 0;
    g_launches = 0;
    set_knobs(c.knobs);
}

void end(int rc) { std::printf("return rc=%d launches=%d\n", rc, g_launches); }

// the workspace extent the pointers are printed against: what the size entry reports at this case's splits
void size_ws(const nerf_field_bwd& a) {
    g_quiet = true;
    g_ws_bytes = a.n_pad > 0 && a.n_pad % 128 == 0 ? nerf_field_bwd_workspace_bytes(a.n_pad, a.ray_grad) : 0;
    g_quiet = false;
}

int run_full(const std::string& name, const Case& c, const nerf_field_bwd* a, void* stream = kMain, void* side = kSide) {
    begin(name, c);
    if (a) size_ws(*a);
    const int rc = nerf_field_backward(a, stream, side);
    end(rc);
    return rc;
}

int run_rays(const std::string& name, const Case& c, const nerf_field_bwd_rays* a) {
    begin(name, c);
    g_quiet = true;
    g_ws_bytes = a && a->n_pad > 0 && a->n_pad % 128 == 0 ? nerf_field_bwd_rays_workspace_bytes(a->n_pad) : 0;
    g_quiet = false;
    const int rc = nerf_field_backward_rays(a, kMain);
    end(rc);
    return rc;
}

nerf_field_bwd full(int chain, int ray_grad, bool graw4, int tail_main = 0) {
    nerf_field_bwd a = g_full;
    a.bwd_chain = chain; a.ray_grad = ray_grad; a.tail_main = tail_main;
    if (!graw4) a.graw4 = nullptr;
    return a;
}

nerf_field_bwd_rays rays(bool graw4) {
    nerf_field_bwd_rays a = g_rays;
    if (!graw4) a.graw4 = nullptr;
    return a;
}

std::string tag(const std::string& knobs) {
    std::string t = knobs.empty() ? "unset" : knobs;
    for (char& ch : t)
        if (ch == ' ') ch = ',';
    return t;
}

// fail the k-th launch for k = 1, 2, ... until the schedule runs through: every error exit of it
void sweep_full(const std::string& name, Case c, const nerf_field_bwd& a) {
    for (int k = 1;; ++k) {
        c.fail_at = k;
        if (run_full(name + "/fail@" + std::to_string(k), c, &a) == NERF_OK) break;
    }
}

}  // namespace

int main() {
    make_args();
    Case dflt;

    // event creation fails (first: the pool is still empty), then a failing record
    {
        Case c; c.fail_event_create = true; c.knobs = "HEADS_PLACE=5";
        const nerf_field_bwd a = full(1, 1, false);
        run_full("events/create-fails", c, &a);
        Case r; r.fail_event_record_at = 1; r.knobs = "HEADS_PLACE=5";
        run_full("events/record-fails", r, &a);
    }

    // nerf_field_backward, per-layer schedule
    for (int rg : {0, 1})
        for (int given : {1, 0})
            for (int tail : {0, 2, 3, 10}) {
                const nerf_field_bwd a = full(0, rg, given, tail);
                run_full("layer/rg" + std::to_string(rg) + (given ? "/graw4" : "/composite") + "/tail" + std::to_string(tail),
                         dflt, &a);
            }
    {   // it needs no chain image
        nerf_field_bwd a = full(0, 1, false, 2);
        for (int l = 0; l < L; ++l) a.wt_cimg[l] = nullptr;
        run_full("layer/no-wt_cimg", dflt, &a);
    }

    // nerf_field_backward, chain schedule
    for (int splits : {64, 8}) {
        const std::string sp = "chain/s" + std::to_string(splits) + "/";
        std::vector<std::string> knobs = {"", "SCHED=1", "SCHED=2", "SCHED=3"};
        for (const char* g : {"", "GROUPS=0", "GROUPS=1", "GROUPS=2"})
            for (const char* b : {"", "BATCH1=0", "BATCH1=1", "BATCH1=2"}) {
                std::string k = "SCHED=3";
                if (*g) k += std::string(" ") + g;
                if (*b) k += std::string(" ") + b;
                if (*g || *b) knobs.push_back(k);
            }
        for (const char* h : {"0", "1", "2", "3", "5"}) knobs.push_back(std::string("HEADS_PLACE=") + h);
        for (const char* h : {"0", "2", "3", "5"})   // the head placements under the other weight-gradient schedules
            for (const char* s : {"1", "2"}) knobs.push_back(std::string("SCHED=") + s + " HEADS_PLACE=" + h);
        for (const std::string& k : knobs)
            for (int rg : {0, 1}) {
                Case c; c.splits = splits; c.knobs = k;
                const nerf_field_bwd a = full(1, rg, false);
                run_full(sp + tag(k) + "/rg" + std::to_string(rg), c, &a);
            }
        Case c; c.splits = splits;
        nerf_field_bwd a = full(1, 1, true, 7);   // a given graw4; tail_main is ignored here
        run_full(sp + "unset/rg1/graw4", c, &a);
        a.wt_cimg[0] = nullptr;                   // l0 has no chain image
        run_full(sp + "unset/rg1/no-wt_cimg0", c, &a);
    }

    // nerf_field_backward_rays
    for (int given : {1, 0}) {
        const nerf_field_bwd_rays a = rays(given);
        run_rays(given ? "rays/graw4" : "rays/composite", dflt, &a);
    }
    {
        nerf_field_bwd_rays a = rays(false);   // what it never reads may be absent
        a.wt_cimg[0] = nullptr;
        for (int l : {1, 2, 3, 5, 6, 7, 8}) { a.wt[l] = nullptr; a.wt_img[l] = nullptr; }
        run_rays("rays/minimal", dflt, &a);
    }

    // workspace sizes
    for (int splits : {64, 8})
        for (int np : {0, 100, 128, 65536, 131072}) {
            Case c; c.splits = splits;
            begin("size/s" + std::to_string(splits) + "/np" + std::to_string(np), c);
            for (int rg : {0, 1})
                Line("nerf_field_bwd_workspace_bytes").i("n_pad", np).i("ray_grad", rg)
                    .i("->", (long long)nerf_field_bwd_workspace_bytes(np, rg));
            Line("nerf_field_bwd_rays_workspace_bytes").i("n_pad", np).i("->", (long long)nerf_field_bwd_rays_workspace_bytes(np));
            end(0);
        }

    // refusals of nerf_field_backward: every check once
    {
        using Edit = std::function<void(nerf_field_bwd&)>;
        run_full("refuse/full/null-struct", dflt, nullptr);
        auto refuse = [&](const std::string& name, int chain, int rg, bool graw4, const Edit& edit, void* stream = kMain,
                          void* side = kSide, int precision = 2) {
            nerf_field_bwd a = full(chain, rg, graw4);
            edit(a);
            Case c; c.precision = precision;
            run_full("refuse/full/" + name, c, &a, stream, side);
        };
        refuse("n_pad=0", 1, 0, false, [](nerf_field_bwd& a) { a.n_pad = 0; });
        refuse("n_pad=-128", 1, 0, false, [](nerf_field_bwd& a) { a.n_pad = -128; });
        refuse("n_pad=100", 1, 0, false, [](nerf_field_bwd& a) { a.n_pad = 100; });
        refuse("no-workspace", 1, 0, false, [](nerf_field_bwd& a) { a.workspace = nullptr; });
        refuse("no-side-stream", 1, 0, false, [](nerf_field_bwd&) {}, kMain, nullptr);
        refuse("equal-streams", 1, 0, false, [](nerf_field_bwd&) {}, kMain, kMain);
        refuse("precision=1", 1, 0, false, [](nerf_field_bwd&) {}, kMain, kSide, 1);
        refuse("precision=0", 0, 0, false, [](nerf_field_bwd&) {}, kMain, kSide, 0);
        refuse("tail_main=-1", 0, 0, false, [](nerf_field_bwd& a) { a.tail_main = -1; });
        refuse("tail_main=11", 1, 0, false, [](nerf_field_bwd& a) { a.tail_main = 11; });
        refuse("no-g_rgb", 1, 0, false, [](nerf_field_bwd& a) { a.g_rgb = nullptr; });
        refuse("no-g_dist", 1, 0, false, [](nerf_field_bwd& a) { a.g_dist = nullptr; });
        refuse("no-z", 1, 0, false, [](nerf_field_bwd& a) { a.z = nullptr; });
        refuse("no-raw4", 1, 0, false, [](nerf_field_bwd& a) { a.raw4 = nullptr; });
        refuse("no-act3", 1, 0, false, [](nerf_field_bwd& a) { a.act[3] = nullptr; });
        refuse("no-wt0", 0, 0, false, [](nerf_field_bwd& a) { a.wt[0] = nullptr; });
        refuse("no-wt_img9", 1, 0, false, [](nerf_field_bwd& a) { a.wt_img[9] = nullptr; });
        refuse("no-gw5", 1, 0, false, [](nerf_field_bwd& a) { a.gw[5] = nullptr; });
        refuse("no-gb8", 1, 0, false, [](nerf_field_bwd& a) { a.gb[8] = nullptr; });
        refuse("no-wt_cimg4", 1, 0, false, [](nerf_field_bwd& a) { a.wt_cimg[4] = nullptr; });
        refuse("no-wt_cimg9", 1, 0, false, [](nerf_field_bwd& a) { a.wt_cimg[9] = nullptr; });
        refuse("mask8-given", 1, 0, false, [](nerf_field_bwd& a) { a.mask[8] = a.mask[7]; });
        refuse("no-mask2", 1, 0, false, [](nerf_field_bwd& a) { a.mask[2] = nullptr; });
        refuse("no-mask9", 0, 0, false, [](nerf_field_bwd& a) { a.mask[9] = nullptr; });
        refuse("cmax9-given", 1, 0, false, [](nerf_field_bwd& a) { a.cmax[9] = a.cmax[8]; });
        refuse("no-cmax1", 1, 0, false, [](nerf_field_bwd& a) { a.cmax[1] = nullptr; });
        refuse("no-enc_p", 1, 0, false, [](nerf_field_bwd& a) { a.enc_p = nullptr; });
        refuse("no-enc_d", 1, 0, false, [](nerf_field_bwd& a) { a.enc_d = nullptr; });
        refuse("no-enc_p_cmax", 1, 0, false, [](nerf_field_bwd& a) { a.enc_p_cmax = nullptr; });
        refuse("no-enc_d_cmax", 1, 0, false, [](nerf_field_bwd& a) { a.enc_d_cmax = nullptr; });
        refuse("no-wd", 1, 0, false, [](nerf_field_bwd& a) { a.wd = nullptr; });
        refuse("no-wc", 1, 0, false, [](nerf_field_bwd& a) { a.wc = nullptr; });
        refuse("no-g_wd", 1, 0, false, [](nerf_field_bwd& a) { a.g_wd = nullptr; });
        refuse("no-g_bd", 1, 0, false, [](nerf_field_bwd& a) { a.g_bd = nullptr; });
        refuse("no-g_wc", 1, 0, false, [](nerf_field_bwd& a) { a.g_wc = nullptr; });
        refuse("no-g_bc", 1, 0, false, [](nerf_field_bwd& a) { a.g_bc = nullptr; });
        refuse("rg/no-pts_o", 1, 1, false, [](nerf_field_bwd& a) { a.pts_o = nullptr; });
        refuse("rg/no-pts_d", 1, 1, false, [](nerf_field_bwd& a) { a.pts_d = nullptr; });
        refuse("rg/no-view", 0, 1, false, [](nerf_field_bwd& a) { a.view = nullptr; });
        refuse("rg/no-z", 1, 1, true, [](nerf_field_bwd& a) { a.z = nullptr; });
        refuse("rg/no-g_pts_o", 1, 1, false, [](nerf_field_bwd& a) { a.g_pts_o = nullptr; });
        refuse("rg/no-g_pts_d", 1, 1, false, [](nerf_field_bwd& a) { a.g_pts_d = nullptr; });
        refuse("rg/no-g_view", 1, 1, false, [](nerf_field_bwd& a) { a.g_view = nullptr; });
        // what is allowed to be absent: the ray tensors without ray gradients, the composite's with graw4
        refuse("ok/no-ray-tensors", 1, 0, true, [](nerf_field_bwd& a) {
            a.pts_o = a.pts_d = a.view = a.z = a.raw4 = a.g_rgb = a.g_dist = nullptr;
            a.g_pts_o = a.g_pts_d = a.g_view = nullptr;
        });
    }
    // refusals of nerf_field_backward_rays
    {
        using Edit = std::function<void(nerf_field_bwd_rays&)>;
        run_rays("refuse/rays/null-struct", dflt, nullptr);
        auto refuse = [&](const std::string& name, bool graw4, const Edit& edit, int precision = 2) {
            nerf_field_bwd_rays a = rays(graw4);
            edit(a);
            Case c; c.precision = precision;
            run_rays("refuse/rays/" + name, c, &a);
        };
        refuse("n_pad=0", false, [](nerf_field_bwd_rays& a) { a.n_pad = 0; });
        refuse("n_pad=100", false, [](nerf_field_bwd_rays& a) { a.n_pad = 100; });
        refuse("no-workspace", false, [](nerf_field_bwd_rays& a) { a.workspace = nullptr; });
        refuse("precision=1", false, [](nerf_field_bwd_rays&) {}, 1);
        refuse("no-g_rgb", false, [](nerf_field_bwd_rays& a) { a.g_rgb = nullptr; });
        refuse("no-g_dist", false, [](nerf_field_bwd_rays& a) { a.g_dist = nullptr; });
        refuse("no-raw4", false, [](nerf_field_bwd_rays& a) { a.raw4 = nullptr; });
        refuse("no-wt_cimg1", false, [](nerf_field_bwd_rays& a) { a.wt_cimg[1] = nullptr; });
        refuse("no-wt_cimg9", false, [](nerf_field_bwd_rays& a) { a.wt_cimg[9] = nullptr; });
        refuse("mask8-given", false, [](nerf_field_bwd_rays& a) { a.mask[8] = a.mask[7]; });
        refuse("no-mask0", false, [](nerf_field_bwd_rays& a) { a.mask[0] = nullptr; });
        refuse("no-wt0", false, [](nerf_field_bwd_rays& a) { a.wt[0] = nullptr; });
        refuse("no-wt_img4", false, [](nerf_field_bwd_rays& a) { a.wt_img[4] = nullptr; });
        refuse("no-wt9", false, [](nerf_field_bwd_rays& a) { a.wt[9] = nullptr; });
        refuse("no-wd", false, [](nerf_field_bwd_rays& a) { a.wd = nullptr; });
        refuse("no-wc", false, [](nerf_field_bwd_rays& a) { a.wc = nullptr; });
        refuse("no-pts_o", false, [](nerf_field_bwd_rays& a) { a.pts_o = nullptr; });
        refuse("no-pts_d", false, [](nerf_field_bwd_rays& a) { a.pts_d = nullptr; });
        refuse("no-view", false, [](nerf_field_bwd_rays& a) { a.view = nullptr; });
        refuse("no-z", true, [](nerf_field_bwd_rays& a) { a.z = nullptr; });
        refuse("no-g_pts_o", false, [](nerf_field_bwd_rays& a) { a.g_pts_o = nullptr; });
        refuse("no-g_pts_d", false, [](nerf_field_bwd_rays& a) { a.g_pts_d = nullptr; });
        refuse("no-g_view", false, [](nerf_field_bwd_rays& a) { a.g_view = nullptr; });
        refuse("ok/graw4-only", true, [](nerf_field_bwd_rays& a) { a.g_rgb = a.g_dist = a.raw4 = nullptr; });
    }

    // mid-schedule failures: every launch of a schedule failed in turn (the error-exit join: a
    // record on side, a wait on main, the error code unchanged)
    {
        const nerf_field_bwd per_layer = full(0, 1, false, 2), chain = full(1, 1, false);
        sweep_full("fail/layer", dflt, per_layer);
        for (const char* k : {"", "SCHED=1", "SCHED=2", "SCHED=3 GROUPS=0 BATCH1=0", "SCHED=3 GROUPS=1 BATCH1=1",
                              "HEADS_PLACE=0", "HEADS_PLACE=2", "HEADS_PLACE=3", "HEADS_PLACE=5"}) {
            Case c; c.knobs = k;
            sweep_full("fail/chain/" + tag(k), c, chain);
        }
        const nerf_field_bwd_rays r = rays(false);
        for (int k = 1;; ++k) {
            Case c; c.fail_at = k;
            if (run_rays("fail/rays/fail@" + std::to_string(k), c, &r) == NERF_OK) break;
        }
    }
    set_knobs("");
    return 0;
}
