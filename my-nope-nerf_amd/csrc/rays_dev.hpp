// Device functions of the ray prologue shared by its separate kernels (rays.hip) and the step
// head (step_head.hip): both compile the same arithmetic, each stage under the floating-point
// contraction it has always had, so their results agree bit for bit.
#pragma once
#include "common.hpp"
#include "mat4.hpp"

#include <cmath>

namespace nerf {

// ------------------------------------------------------------------------------------
// Philox-4x32-10 (Salmon et al., SC'11), the counter-based generator torch's CUDA/HIP RNG
// also uses; keyed by the host seed, counter = (ray slot, round, stream, 0).
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += W0;
        k.y += W1;
    }
    return c;
}

// uniform integer in [0, n) from 64 random bits: floor(u * n / 2^64) (bias < n / 2^64)
__device__ __forceinline__ uint32_t uniform_below(uint4 r, uint32_t n) {
    const uint64_t u = ((uint64_t)r.x << 32) | r.y;
    return (uint32_t)__umul64hi(u, (uint64_t)n);
}

constexpr int SR_THREADS = 1024;
constexpr int SR_LOG_TABLE = 14;
constexpr int SR_TABLE = 1 << SR_LOG_TABLE;     // hash slots; load factor <= 1/4 at SR_MAX
constexpr int SR_PER_THREAD = NERF_SAMPLE_MAX_RAYS / SR_THREADS;
constexpr uint32_t SR_EMPTY = 0xFFFFFFFFu;
constexpr int SR_MAX_ROUNDS = NERF_SAMPLE_MAX_ROUNDS;

// the device step counter's share of the Philox key (graph replays)
__device__ __forceinline__ uint2 sample_key_mix(uint2 key, unsigned long long c) {
    const unsigned long long m = (c + 1) * 0x9E3779B97F4A7C15ull;
    key.x ^= (uint32_t)m;
    key.y ^= (uint32_t)(m >> 32);
    return key;
}

// R distinct pixel indices drawn uniformly from [0, n_pix) -- the set randperm(n)[:R]
// returns, with its own (deterministic) generator.  Each pending ray slot draws a
// candidate, inserts it into an LDS hash set (linear probing), and the slot whose
// (round, slot) key is smallest owns the value; the others draw again next round.  The
// outcome depends only on (seed, n, R), never on wave timing or the table size (2^log_table
// slots each of table / owner, at least 4 R).  One workgroup of THREADS; returns the status
// word (rounds used, 0 = gave up); thread tid's slots are tid + q THREADS.
template <int THREADS>
__device__ __forceinline__ int sample_draw(int n_pix, int R, uint2 key, uint32_t* table, uint32_t* owner,
                                           int log_table, uint32_t (&val)[NERF_SAMPLE_MAX_RAYS / THREADS],
                                           bool (&pend)[NERF_SAMPLE_MAX_RAYS / THREADS]) {
    constexpr int PER = NERF_SAMPLE_MAX_RAYS / THREADS;
    const int tid = threadIdx.x;
    const int n_table = 1 << log_table;
    for (int i = tid; i < n_table; i += THREADS) {
        table[i] = SR_EMPTY;
        owner[i] = 0xFFFFFFFFu;
    }
    __syncthreads();
    uint32_t pos[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) pend[q] = (tid + q * THREADS) < R;
    int round = 0, done = 0;
    for (; round < SR_MAX_ROUNDS; ++round) {
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (!pend[q]) continue;
            const uint32_t slot = tid + q * THREADS;
            const uint32_t v = uniform_below(philox4x32_10(make_uint4(slot, round, 0x5a4d, 0), key), n_pix);
            val[q] = v;
            uint32_t h = (v * 2654435761u) >> (32 - log_table);
            while (true) {
                const uint32_t old = atomicCAS(&table[h], SR_EMPTY, v);
                if (old == SR_EMPTY || old == v) break;
                h = (h + 1) & (n_table - 1);
            }
            pos[q] = h;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; ++q)
            if (pend[q]) atomicMin(&owner[pos[q]], (uint32_t)(round * NERF_SAMPLE_MAX_RAYS + tid + q * THREADS));
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            if (!pend[q]) continue;
            if (owner[pos[q]] == (uint32_t)(round * NERF_SAMPLE_MAX_RAYS + tid + q * THREADS)) pend[q] = false;
            else any = 1;
        }
        if (!__syncthreads_or(any)) { done = 1; break; }
    }
    return done ? round + 1 : 0;
}

// Draw until a drawn pixel has a valid depth (training.py:275-283's `while not m[ray_idx].any()`):
// attempt a = 0, 1, ... is sample_draw with the seed seed + a SR_ATTEMPT_STEP (mod 2^64), its key
// mixed with the device counter as ever, the hash set cleared per attempt (sample_draw clears it).
// An attempt is accepted when any drawn index v has valid[v] != 0 (valid == NULL: always) -- one
// block-wide OR, so every thread leaves the loop in the same attempt.  Returns the status word of
// the accepted (or last) attempt; attempts = its 1-based number, 0 when none of
// NERF_SAMPLE_MAX_ATTEMPTS was accepted (val / pend then hold the last attempt's draw).
constexpr unsigned long long SR_ATTEMPT_STEP = 0xD1B54A32D192ED03ull;
template <int THREADS>
__device__ __forceinline__ int sample_draw_valid(int n_pix, int R, unsigned long long seed, bool has_ctr,
                                                 unsigned long long c, const uint8_t* __restrict__ valid,
                                                 uint32_t* table, uint32_t* owner, int log_table,
                                                 uint32_t (&val)[NERF_SAMPLE_MAX_RAYS / THREADS],
                                                 bool (&pend)[NERF_SAMPLE_MAX_RAYS / THREADS], int& attempts) {
    constexpr int PER = NERF_SAMPLE_MAX_RAYS / THREADS;
    const int tid = threadIdx.x;
    int st = 0;
    attempts = 0;
    for (int a = 0; a < NERF_SAMPLE_MAX_ATTEMPTS; ++a) {
        const unsigned long long sa = seed + (unsigned long long)a * SR_ATTEMPT_STEP;
        uint2 key = make_uint2((uint32_t)sa, (uint32_t)(sa >> 32));
        if (has_ctr) key = sample_key_mix(key, c);
        st = sample_draw<THREADS>(n_pix, R, key, table, owner, log_table, val, pend);
        int hit = valid == nullptr;
#pragma unroll
        for (int q = 0; q < PER; ++q)
            if (!hit && tid + q * THREADS < R && valid[pend[q] ? 0u : val[q]] != 0) hit = 1;
        if (__syncthreads_or(hit)) {   // uniform: the OR is the same in every thread
            attempts = a + 1;
            break;
        }
    }
    return st;
}

// the pixel and colour gathers of ray slot j at pixel index v (common.py:36-39, training.py:284-287)
__device__ __forceinline__ void sample_gather(int j, uint32_t v, int width, int height,
                                              const float* __restrict__ img, int64_t* __restrict__ idx,
                                              float* __restrict__ pix, float* __restrict__ rgb, float& px,
                                              float& py) {
    const int hw = width * height;
    idx[j] = v;
    if (pix != nullptr) {   // arange_pixels: 2*col/(W-1) - 1, 2*row/(H-1) - 1 (common.py:36-39)
        const int row = v / width, col = v - row * width;
        px = 2.f * (float)col / (float)(width - 1) - 1.f;
        py = 2.f * (float)row / (float)(height - 1) - 1.f;
        pix[2 * j] = px;
        pix[2 * j + 1] = py;
    }
    if (rgb != nullptr) {   // img.view(1,3,H*W).permute(0,2,1)[:, idx]
        rgb[3 * j] = img[v];
        rgb[3 * j + 1] = img[hw + v];
        rgb[3 * j + 2] = img[2 * hw + v];
    }
}

// c2w = [Exp(r) | t; 0 0 0 1] @ init (common.py:290-310, poses.py:27-30);
// Exp(r) = I + sin(th)/th [r]x + (1 - cos th)/th^2 [r]x^2,  th = |r| + 1e-15
__device__ __forceinline__ void pose_c2w_eval(const float* __restrict__ r, const float* __restrict__ t,
                                              const float* __restrict__ init, float o[16]) {
#pragma clang fp contract(off)
    const float x = r[0], y = r[1], z = r[2];
    const float th = sqrtf(x * x + y * y + z * z) + 1e-15f;
    const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
    float KK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) KK[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
    const float s = sinf(th) / th, c = (1.f - cosf(th)) / (th * th);
    float m[16];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) m[4 * i + j] = ((i == j ? 1.f : 0.f) + s * K[3 * i + j]) + c * KK[3 * i + j];
        m[4 * i + 3] = t[i];
    }
    m[12] = 0.f; m[13] = 0.f; m[14] = 0.f; m[15] = 1.f;
    if (init != nullptr) {
        float b[16];
        load4(init, b);
        matmul4(m, b, o);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = m[i];
    }
}

// M = (inv(scale) @ inv(world)) @ inv(K)  (common.py:139-141) and the three inverses
__device__ __forceinline__ void unproject_eval(const float K[16], const float world[16], const float scale[16],
                                               float m[16], float ki[16], float wi[16], float si[16]) {
    float t[16];
    inverse4(K, ki);
    inverse4(world, wi);
    inverse4(scale, si);
    matmul4(si, wi, t);
    matmul4(t, ki, m);
}

// depth-prior distortion of one gathered value (training.py:259-264, 325-329, 346-347)
__device__ __forceinline__ float depth_affine_eval(float d, float sc, float sh, int shift_first, float lo) {
#pragma clang fp contract(off)
    const float v = shift_first ? (d + sh) * sc : d * sc + sh;
    return v < lo ? lo : v;
}

// camera ray r at pixel (x, y) with prior depth d (rendering.py:52-80; see k_camera_rays)
__device__ __forceinline__ void camera_ray_eval(const float M[16], float x, float y, bool has_depth, float d,
                                                int r, int flags, float* __restrict__ cam,
                                                float* __restrict__ ray, float* __restrict__ view,
                                                float* __restrict__ ray_norm, float* __restrict__ d_src,
                                                uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
    float v[3], n2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] = (M[4 * i] * x + M[4 * i + 1] * y) + M[4 * i + 2];
        n2 = n2 + v[i] * v[i];
    }
    const float n = sqrtf(n2);
    const bool normalise = flags & NERF_RAYS_NORMALISE;
    float ds = 1.f;   // no depth prior: d_src = 1 under either flag (the backward takes it as constant)
    if (has_depth) {
        const float xd = x * d, yd = y * d;
        float q2 = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float pi = (M[4 * i] * xd + M[4 * i + 1] * yd) + M[4 * i + 2] * d;
            q2 = q2 + pi * pi;
        }
        ds = sqrtf(q2);
        if (!normalise) ds = ds / n;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float di = normalise ? v[i] / n : v[i];
        cam[3 * r + i] = M[4 * i + 3];
        ray[3 * r + i] = di;
        if (view != nullptr) view[3 * r + i] = (flags & NERF_RAYS_VIEW_ONES) ? 1.f : -di;
    }
    ray_norm[r] = n;
    d_src[r] = ds;
    if (mask != nullptr) mask[r] = (isfinite(ds) && ds != 0.f) ? 1 : 0;
}

}  // namespace nerf
