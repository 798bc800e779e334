// The per-ray logic of the geometry visualisation (rendering_technique 'phong_renderer',
// rendering.py:199-468): sphere intersection and the segmented sample set-up, the first sign
// change of occupancy - tau, the secant update and the headlight Phong shading.  The field
// evaluations between them are the launches of render.hip / chain.hip (model/geometry.py);
// every kernel here is dense over the frame's rays, so nothing depends on how many rays hit.
#include "common.hpp"
#include "samples.hpp"

#include <cmath>

namespace nerf {

// one thread per ray: d_far in f64 from the f32 inputs (u cancels near a tangent ray), then
// the ray's G pseudo-rays.  c = cam[0] for every ray (the reference passes ray0[:, 0])
__global__ __launch_bounds__(256) void k_march_rays(const float* __restrict__ cam, const float* __restrict__ ray,
                                                    int R, float rad, float d0, int n_steps, int seg,
                                                    float* __restrict__ d_far, float* __restrict__ o_seg,
                                                    float* __restrict__ d_seg) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const double cx = cam[0], cy = cam[1], cz = cam[2];
    const double dx = ray[3 * r], dy = ray[3 * r + 1], dz = ray[3 * r + 2];
    const double b = dx * cx + dy * cy + dz * cz;
    const double u = b * b - ((cx * cx + cy * cy + cz * cz) - (double)rad * (double)rad);
    const float far_f = u > 0.0 ? (float)fmax(sqrt(u) - b, 0.0) : 0.f;
    d_far[r] = far_f;
    const double ox = cam[3 * r], oy = cam[3 * r + 1], oz = cam[3 * r + 2];
    const double span = (double)far_f - (double)d0, inv = 1.0 / (double)(n_steps - 1);
    const double len = span * (double)(seg - 1) * inv;
    const int G = n_steps / seg;
    for (int g = 0; g < G; ++g) {
        const double a = (double)d0 + span * (double)(g * seg) * inv;
        const size_t e = 3 * ((size_t)r * G + g);
        o_seg[e] = (float)(ox + dx * a);
        o_seg[e + 1] = (float)(oy + dy * a);
        o_seg[e + 2] = (float)(oz + dz * a);
        d_seg[e] = (float)(dx * len);
        d_seg[e + 1] = (float)(dy * len);
        d_seg[e + 2] = (float)(dz * len);
    }
}

// one wave per ray, four rays per block: lanes stride over the pairs (j, j + 1), a ballot per
// 64 pairs finds the first negative product (the ballot is wave-uniform, so is the exit).  A NaN
// product is not negative: torch.sign gives 0 for it, no change at that pair
constexpr int SELECT_RAYS = 4;
__global__ __launch_bounds__(64 * SELECT_RAYS) void k_march_select(
    const float* __restrict__ occ, int R, int n, const float* __restrict__ d_far, float d0, float tau,
    uint8_t* __restrict__ state, float* __restrict__ f_low, float* __restrict__ f_high, float* __restrict__ d_low,
    float* __restrict__ d_high) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * SELECT_RAYS + (threadIdx.x >> 6);
    if (r >= R) return;                       // a whole wave leaves together
    const int lane = lane_id();
    const float* v = occ + (size_t)r * n;
    int first = -1;
    for (int base = 0; base < n - 1; base += kWave) {
        const int j = base + lane;
        bool neg = false;
        if (j < n - 1) neg = (v[j] - tau) * (v[j + 1] - tau) < 0.f;
        const unsigned long long m = __ballot(neg);
        if (m) {
            first = base + __ffsll((long long)m) - 1;
            break;
        }
    }
    if (lane != 0) return;
    const float v0 = v[0] - tau;
    int st = NERF_MARCH_NONE;
    float fl = 0.f, fh = 0.f, dl = 0.f, dh = 0.f;
    if (!(v0 < 0.f)) {
        st = NERF_MARCH_INSIDE;
    } else if (first >= 0 && (v[first] - tau) < 0.f) {
        st = NERF_MARCH_BRACKET;
        const float fz = d_far[r];
        fl = v[first] - tau;
        fh = v[first + 1] - tau;
        // in f64, as nerf_march_rays places the samples: 1 - t cancels in f32 when d0 carries the distance
        const double inv = 1.0 / (double)(n - 1);
        const double tl = (double)first * inv, th = (double)(first + 1) * inv;
        dl = (float)((double)d0 * (1.0 - tl) + (double)fz * tl);
        dh = (float)((double)d0 * (1.0 - th) + (double)fz * th);
    }
    state[r] = (uint8_t)st;
    f_low[r] = fl; f_high[r] = fh; d_low[r] = dl; d_high[r] = dh;
}

// OfficialStaticNerf._density with the accurate library functions torch runs
__device__ __forceinline__ float occupancy_f(float raw, int flags) {
    const float sigma = (flags & F_RELU) ? fmaxf(raw, 0.f) : softplus_f(raw);
    return (flags & F_DIST_ALPHA) ? sigma : 1.f - expf(-1.0f * sigma);
}

__device__ __forceinline__ float secant_pred(float fl, float fh, float dl, float dh) {
#pragma clang fp contract(off)
    return -fl * (dh - dl) / (fh - fl) + dl;
}

// one thread per ray
__global__ __launch_bounds__(256) void k_secant_step(int first, const float* __restrict__ raw4, int flags, float tau,
                                                     const uint8_t* __restrict__ state,
                                                     const float* __restrict__ cam, const float* __restrict__ ray,
                                                     int R, float* __restrict__ f_low, float* __restrict__ f_high,
                                                     float* __restrict__ d_low, float* __restrict__ d_high,
                                                     float* __restrict__ d_pred, float* __restrict__ p_mid,
                                                     float* __restrict__ d_i) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int st = state[r];
    float fl = f_low[r], fh = f_high[r], dl = d_low[r], dh = d_high[r];
    float dp;
    if (first) {
        dp = secant_pred(fl, fh, dl, dh);
    } else {
        dp = d_pred[r];
        if (isfinite(dp)) {
            const float fm = occupancy_f(raw4[4 * (size_t)r], flags) - tau;
            if (fm < 0.f) { dl = dp; fl = fm; }
            else { dh = dp; fh = fm; }
            f_low[r] = fl; f_high[r] = fh; d_low[r] = dl; d_high[r] = dh;
            dp = secant_pred(fl, fh, dl, dh);
        }
    }
    d_pred[r] = dp;
    const bool go = st == NERF_MARCH_BRACKET && isfinite(dp);
    const float z = go ? dp : 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float o = cam[3 * (size_t)r + k];
        p_mid[3 * (size_t)r + k] = go ? ray_point(o, ray[3 * (size_t)r + k], z) : o;
    }
    d_i[r] = st == NERF_MARCH_BRACKET ? dp : (st == NERF_MARCH_INSIDE ? 0.f : INFINITY);
}

// one thread per ray
__global__ __launch_bounds__(256) void k_phong_shade(const float* __restrict__ g, const float* __restrict__ raw4,
                                                     const uint8_t* __restrict__ state,
                                                     const float* __restrict__ d_i, const float* __restrict__ cam,
                                                     int R, float* __restrict__ rgb, float* __restrict__ rgb_surf) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    float shade = 1.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (state[r] == NERF_MARCH_BRACKET && isfinite(d_i[r])) {
        const float lx = cam[0], ly = cam[1], lz = cam[2];
        const float ln = sqrtf(lx * lx + ly * ly + lz * lz);
        const float gx = g[3 * (size_t)r], gy = g[3 * (size_t)r + 1], gz = g[3 * (size_t)r + 2];
        const float gn = sqrtf(gx * gx + gy * gy + gz * gz);
        const float dot = (gx / gn) * (lx / ln) + (gy / gn) * (ly / ln) + (gz / gn) * (lz / ln);
        shade = fminf(0.3f + 0.7f * fmaxf(dot, 0.f), 1.f);
        if (dot != dot) shade = dot;          // a zero gradient gives NaN, as the reference's clamps do
        const float4 q = *reinterpret_cast<const float4*>(raw4 + 4 * (size_t)r);
        s0 = sigmoid_f(q.y); s1 = sigmoid_f(q.z); s2 = sigmoid_f(q.w);
    }
    float* c = rgb + 3 * (size_t)r;
    float* s = rgb_surf + 3 * (size_t)r;
    c[0] = shade; c[1] = shade; c[2] = shade;
    s[0] = s0; s[1] = s1; s[2] = s2;
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_march_rays(const float* cam, const float* ray, int n_rays, float rad, float d0, int n_steps,
                               int seg, float* d_far, float* o_seg, float* d_seg, void* stream) {
    NERF_CHECK_PTR(cam); NERF_CHECK_PTR(ray); NERF_CHECK_PTR(d_far); NERF_CHECK_PTR(o_seg); NERF_CHECK_PTR(d_seg);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK(n_steps >= 2 && seg >= 2 && n_steps % seg == 0, "%s: seg=%d must be >= 2 and divide n_steps=%d",
               __func__, seg, n_steps);
    NERF_CHECK((int64_t)n_rays * n_steps <= (int64_t)1 << 30, "%s: too many samples", __func__);
    hipLaunchKernelGGL(k_march_rays, dim3((n_rays + 255) / 256), dim3(256), 0, as_stream(stream), cam, ray, n_rays,
                       rad, d0, n_steps, seg, d_far, o_seg, d_seg);
    return check_launch(__func__);
}

extern "C" int nerf_march_select(const float* occ, int n_rays, int n, const float* d_far, float d0, float tau,
                                 uint8_t* state, float* f_low, float* f_high, float* d_low, float* d_high,
                                 void* stream) {
    NERF_CHECK_PTR(occ); NERF_CHECK_PTR(d_far); NERF_CHECK_PTR(state);
    NERF_CHECK_PTR(f_low); NERF_CHECK_PTR(f_high); NERF_CHECK_PTR(d_low); NERF_CHECK_PTR(d_high);
    NERF_CHECK(n_rays > 0 && n >= 2, "%s: n_rays=%d, n=%d (n >= 2)", __func__, n_rays, n);
    hipLaunchKernelGGL(k_march_select, dim3((n_rays + SELECT_RAYS - 1) / SELECT_RAYS), dim3(64 * SELECT_RAYS), 0,
                       as_stream(stream), occ, n_rays, n, d_far, d0, tau, state, f_low, f_high, d_low, d_high);
    return check_launch(__func__);
}

extern "C" int nerf_secant_step(int first, const float* raw4, int flags, float tau, const uint8_t* state,
                                const float* cam, const float* ray, int n_rays, float* f_low, float* f_high,
                                float* d_low, float* d_high, float* d_pred, float* p_mid, float* d_i, void* stream) {
    NERF_CHECK(first || raw4 != nullptr, "%s: raw4 is required after the first step", __func__);
    NERF_CHECK_PTR(state); NERF_CHECK_PTR(cam); NERF_CHECK_PTR(ray);
    NERF_CHECK_PTR(f_low); NERF_CHECK_PTR(f_high); NERF_CHECK_PTR(d_low); NERF_CHECK_PTR(d_high);
    NERF_CHECK_PTR(d_pred); NERF_CHECK_PTR(p_mid); NERF_CHECK_PTR(d_i);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK((flags & ~(F_DIST_ALPHA | F_RELU)) == 0, "%s: unknown flags %d", __func__, flags);
    hipLaunchKernelGGL(k_secant_step, dim3((n_rays + 255) / 256), dim3(256), 0, as_stream(stream), first, raw4, flags,
                       tau, state, cam, ray, n_rays, f_low, f_high, d_low, d_high, d_pred, p_mid, d_i);
    return check_launch(__func__);
}

extern "C" int nerf_phong_shade(const float* g, const float* raw4, const uint8_t* state, const float* d_i,
                                const float* cam, int n_rays, float* rgb, float* rgb_surf, void* stream) {
    NERF_CHECK_PTR(g); NERF_CHECK_PTR(raw4); NERF_CHECK_PTR(state); NERF_CHECK_PTR(d_i); NERF_CHECK_PTR(cam);
    NERF_CHECK_PTR(rgb); NERF_CHECK_PTR(rgb_surf);
    NERF_CHECK_ALIGN16(raw4);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    hipLaunchKernelGGL(k_phong_shade, dim3((n_rays + 255) / 256), dim3(256), 0, as_stream(stream), g, raw4, state, d_i,
                       cam, n_rays, rgb, rgb_surf);
    return check_launch(__func__);
}
