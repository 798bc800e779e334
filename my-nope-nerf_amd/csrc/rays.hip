// Ray prologue and loss epilogue of the training step.
//
// Everything the reference runs around the per-sample work of one step, as a handful of
// launches instead of ~150 ATen ones:
//   * k_sample_rays   : randperm(H*W)[:R] + the pixel / colour gathers (training.py:277-283,
//                       common.py:13-40) -- one workgroup, a deterministic LDS hash set;
//   * k_mat4          : batched 4x4 inverse, SO(3) x R^3 pose composition (common.py:277-310,
//                       poses.py:23-31) and the unprojection matrix
//                       inv(scale) @ inv(world) @ inv(K) (common.py:139-141, 205-208);
//   * k_camera_rays   : origin, unit direction, |P1 - o|, d_src and the depth mask per ray
//                       (rendering.py:52-80) and its backward (pose / distortion learning);
//   * k_ndc_rays(_bwd): the NDC warp of those rays for sample_option 'ndc' (common.py:632-675,
//                       rendering.py:169-181) with d_gt = 1 - 1 / d_src (rendering.py:158-159);
//   * k_ray_loss(_bwd): rgb l1/l2 + masked depth l1 + l2_mean and their gradients
//                       (losses.py:28-33, 60-66, 164-228);
//   * k_sample_rays_valid: the draw repeated until a drawn pixel has a valid depth
//                       (training.py:275-283's host loop over img.depth_mask, inside the launch);
//   * k_ray_loss_inv(_bwd): the same with depth_loss_type 'invariant' (losses.py:35-58): both
//                       medians selected in the launch, no boolean indexing, no host sync.
// All are launch-latency bound (a few KB per step); the point is the launch count.
#include "common.hpp"
#include "mat4.hpp"
#include "rays_dev.hpp"

#include <cmath>

namespace nerf {

// One workgroup: the draw (rays_dev.hpp sample_draw, the hash set in 2 x 64 KB of LDS), then the
// pixel / colour gathers.
__global__ __launch_bounds__(SR_THREADS) void k_sample_rays(int n_pix, int R, uint2 key, int width, int height,
                                                            const float* __restrict__ img,
                                                            int64_t* __restrict__ idx, float* __restrict__ pix,
                                                            float* __restrict__ rgb, int* __restrict__ status,
                                                            unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t table[SR_TABLE];
    __shared__ uint32_t owner[SR_TABLE];
    const int tid = threadIdx.x;
    // device step counter (graph replays): the key mixes in the counter, thread 0 advances it
    // once every thread has read it (the kernel is a single workgroup)
    const unsigned long long c = ctr ? *ctr : 0ull;
    if (ctr) key = sample_key_mix(key, c);
    uint32_t val[SR_PER_THREAD];
    bool pend[SR_PER_THREAD];
    const int st = sample_draw<SR_THREADS>(n_pix, R, key, table, owner, SR_LOG_TABLE, val, pend);
    if (tid == 0 && status != nullptr) *status = st;   // rounds used, 0 = gave up
#pragma unroll
    for (int q = 0; q < SR_PER_THREAD; ++q) {
        const int j = tid + q * SR_THREADS;
        if (j >= R) continue;
        float px, py;
        sample_gather(j, pend[q] ? 0u : val[q], width, height, img, idx, pix, rgb, px, py);
    }
    if (ctr != nullptr) {
        __syncthreads();
        if (tid == 0) *ctr = c + 1;
    }
}

// k_sample_rays with the draw repeated until a drawn pixel has a valid depth (rays_dev.hpp
// sample_draw_valid); the gathers run once, on the accepted (or last) attempt.
__global__ __launch_bounds__(SR_THREADS) void k_sample_rays_valid(int n_pix, int R, unsigned long long seed,
                                                                  int width, int height,
                                                                  const float* __restrict__ img,
                                                                  const uint8_t* __restrict__ valid,
                                                                  int64_t* __restrict__ idx, float* __restrict__ pix,
                                                                  float* __restrict__ rgb, int* __restrict__ status,
                                                                  int* __restrict__ attempts,
                                                                  unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t table[SR_TABLE];
    __shared__ uint32_t owner[SR_TABLE];
    const int tid = threadIdx.x;
    const unsigned long long c = ctr ? *ctr : 0ull;
    uint32_t val[SR_PER_THREAD];
    bool pend[SR_PER_THREAD];
    int att;
    const int st = sample_draw_valid<SR_THREADS>(n_pix, R, seed, ctr != nullptr, c, valid, table, owner,
                                                 SR_LOG_TABLE, val, pend, att);
    if (tid == 0 && status != nullptr) *status = st;
    if (tid == 0 && attempts != nullptr) *attempts = att;
#pragma unroll
    for (int q = 0; q < SR_PER_THREAD; ++q) {
        const int j = tid + q * SR_THREADS;
        if (j >= R) continue;
        float px, py;
        sample_gather(j, pend[q] ? 0u : val[q], width, height, img, idx, pix, rgb, px, py);
    }
    if (ctr != nullptr) {
        __syncthreads();
        if (tid == 0) *ctr = c + 1;
    }
}

__global__ void k_mat4_inv(const float* __restrict__ a, int n, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float m[16], r[16];
    load4(a + 16 * (size_t)i, m);
    inverse4(m, r);
    store4(out + 16 * (size_t)i, r);
}

// c2w = [Exp(r) | t; 0 0 0 1] @ init (rays_dev.hpp pose_c2w_eval), one thread
__global__ void k_pose_c2w(const float* __restrict__ r, const float* __restrict__ t,
                           const float* __restrict__ init, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float o[16];
    pose_c2w_eval(r, t, init, o);
    store4(out, o);
}

// Backward of k_pose_c2w (the closed form of torch autograd through common.py:277-310):
// G = g @ init^T is the gradient of [R | t]; g_t = G[:3, 3];
//   dL/dK = s G_R + c (G_R K^T + K^T G_R),  dL/dth = s'(th) <G_R, K> + c'(th) <G_R, K^2>,
//   s = sin th / th, c = (1 - cos th) / th^2, dth/dr = r / |r| (0 at r = 0, torch's norm
//   subgradient), K = [r]x so dL/dx = dK[2][1] - dK[1][2] etc.  Evaluated in f64.
__global__ void k_pose_c2w_bwd(const float* __restrict__ r, const float* __restrict__ init,
                               const float* __restrict__ g, float* __restrict__ gr, float* __restrict__ gt) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double G[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            if (init != nullptr) {
                for (int k = 0; k < 4; ++k) s += (double)g[4 * i + k] * (double)init[4 * j + k];
            } else {
                s = g[4 * i + j];
            }
            G[4 * i + j] = s;
        }
    if (gt != nullptr)
        for (int i = 0; i < 3; ++i) gt[i] = (float)G[4 * i + 3];
    if (gr == nullptr) return;
    const double x = r[0], y = r[1], z = r[2];
    const double nr = sqrt(x * x + y * y + z * z);
    const double th = (double)(float)((float)nr + 1e-15f);
    const double K[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};
    double KK[9], GR[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            KK[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
            GR[3 * i + j] = G[4 * i + j];
        }
    const double sn = sin(th), cs = cos(th);
    const double s = sn / th, c = (1.0 - cs) / (th * th);
    const double ds = cs / th - sn / (th * th);
    const double dc = sn / (th * th) - 2.0 * (1.0 - cs) / (th * th * th);
    double dK[9], gk = 0.0, gkk = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = 0.0, b = 0.0;   // (G_R K^T)_ij, (K^T G_R)_ij
            for (int k = 0; k < 3; ++k) {
                a += GR[3 * i + k] * K[3 * j + k];
                b += K[3 * k + i] * GR[3 * k + j];
            }
            dK[3 * i + j] = s * GR[3 * i + j] + c * (a + b);
            gk += GR[3 * i + j] * K[3 * i + j];
            gkk += GR[3 * i + j] * KK[3 * i + j];
        }
    const double dth = ds * gk + dc * gkk;
    const double w = nr > 0.0 ? dth / nr : 0.0;
    gr[0] = (float)(dK[7] - dK[5] + w * x);
    gr[1] = (float)(dK[2] - dK[6] + w * y);
    gr[2] = (float)(dK[3] - dK[1] + w * z);
}

// d inv(A) = -Y dA Y  ->  gA = -Y^T g Y^T, batched ([n][4][4])
__global__ void k_mat4_inv_bwd(const float* __restrict__ y, const float* __restrict__ g, int n,
                               float* __restrict__ ga) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float Y[16], Yt[16], G[16], t[16], o[16];
    load4(y + 16 * (size_t)i, Y);
    load4(g + 16 * (size_t)i, G);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) Yt[4 * a + b] = Y[4 * b + a];
    matmul4(Yt, G, t);
    matmul4(t, Yt, o);
#pragma unroll
    for (int k = 0; k < 16; ++k) o[k] = -o[k];
    store4(ga + 16 * (size_t)i, o);
}

// C = A @ B (batched [n][4][4]) and its backward gA = g B^T, gB = A^T g (either optional)
__global__ void k_mat4_mul(const float* __restrict__ a, const float* __restrict__ b, int n, float* __restrict__ c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float A[16], B[16], C[16];
    load4(a + 16 * (size_t)i, A);
    load4(b + 16 * (size_t)i, B);
    matmul4(A, B, C);
    store4(c + 16 * (size_t)i, C);
}
__global__ void k_mat4_mul_bwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ g,
                               int n, float* __restrict__ ga, float* __restrict__ gb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float A[16], B[16], G[16], T[16], O[16];
    load4(g + 16 * (size_t)i, G);
    if (ga != nullptr) {
        load4(b + 16 * (size_t)i, B);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) T[4 * p + q] = B[4 * q + p];
        matmul4(G, T, O);
        store4(ga + 16 * (size_t)i, O);
    }
    if (gb != nullptr) {
        load4(a + 16 * (size_t)i, A);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) T[4 * p + q] = A[4 * q + p];
        matmul4(T, G, O);
        store4(gb + 16 * (size_t)i, O);
    }
}

// Backward of k_unproject: M = Si Wi Ki with Xi = inv(X) and d inv(A) = -Ai dA Ai:
//   gK = -Ki^T ((Si Wi)^T g) Ki^T,  gW = -Wi^T (Si^T g Ki^T) Wi^T,  gS = -Si^T (g (Wi Ki)^T) Si^T
// (each output optional; inverses = {Ki, Wi, Si} from the forward)
__global__ void k_unproject_bwd(const float* __restrict__ inverses, const float* __restrict__ g,
                                float* __restrict__ gK, float* __restrict__ gW, float* __restrict__ gS) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float Ki[16], Wi[16], Si[16], G[16], A[16], B[16], T[16], O[16];
    load4(inverses, Ki);
    load4(inverses + 16, Wi);
    load4(inverses + 32, Si);
    load4(g, G);
    auto tr = [](const float (&x)[16], float (&y)[16]) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) y[4 * p + q] = x[4 * q + p];
    };
    auto neg_sandwich = [&](const float (&Xi)[16], const float (&inner)[16], float* out) {
        float Xt[16], t1[16], t2[16];
        tr(Xi, Xt);
        matmul4(Xt, inner, t1);
        matmul4(t1, Xt, t2);
#pragma unroll
        for (int k = 0; k < 16; ++k) t2[k] = -t2[k];
        store4(out, t2);
    };
    if (gK != nullptr) {
        matmul4(Si, Wi, A);
        tr(A, T);
        matmul4(T, G, O);
        neg_sandwich(Ki, O, gK);
    }
    if (gW != nullptr) {
        tr(Si, T);
        matmul4(T, G, A);
        tr(Ki, T);
        matmul4(A, T, O);
        neg_sandwich(Wi, O, gW);
    }
    if (gS != nullptr) {
        matmul4(Wi, Ki, B);
        tr(B, T);
        matmul4(G, T, O);
        neg_sandwich(Si, O, gS);
    }
}

// Depth-prior distortion on gathered prior values (training.py:259-264, 325-329, 346-347):
// y = d s + t (or (d + t) s with shift_first), then y < lo -> lo (the pc resize's
// d[d < nearest_limit] = nearest_limit; lo = -inf for none).  Backward: the clamped entries
// pass no gradient; g_s = sum g (d [+ t]), g_t = sum g (x s with shift_first) -- one
// workgroup, a fixed-order tree (deterministic).
constexpr int AF_THREADS = 1024;
__global__ __launch_bounds__(AF_THREADS) void k_depth_affine(const float* __restrict__ d, int n,
                                                             const float* __restrict__ s, const float* __restrict__ t,
                                                             int shift_first, float lo, float* __restrict__ y) {
    const float sc = s[0], sh = t[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        y[i] = depth_affine_eval(d[i], sc, sh, shift_first, lo);
}
__global__ __launch_bounds__(AF_THREADS) void k_depth_affine_bwd(const float* __restrict__ d, int n,
                                                                 const float* __restrict__ s,
                                                                 const float* __restrict__ t, int shift_first,
                                                                 float lo, const float* __restrict__ g,
                                                                 float* __restrict__ gs, float* __restrict__ gt) {
#pragma clang fp contract(off)
    __shared__ float red[2][AF_THREADS / 64];
    const float sc = s[0], sh = t[0];
    float as = 0.f, at = 0.f;
    for (int i = threadIdx.x; i < n; i += AF_THREADS) {
        const float v = shift_first ? (d[i] + sh) * sc : d[i] * sc + sh;
        if (v < lo) continue;
        const float gi = g[i];
        as += shift_first ? gi * (d[i] + sh) : gi * d[i];
        at += shift_first ? gi * sc : gi;
    }
    as = wave_sum(as);
    at = wave_sum(at);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = as; red[1][w] = at; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f;
        for (int k = 0; k < AF_THREADS / 64; ++k) { a += red[0][k]; b += red[1][k]; }
        if (gs) gs[0] = a;
        if (gt) gt[0] = b;
    }
}

// M = (inv(scale) @ inv(world)) @ inv(K)  (common.py:139-141); inverses kept for backward
__global__ void k_unproject(const float* __restrict__ K, const float* __restrict__ world,
                            const float* __restrict__ scale, float* __restrict__ M, float* __restrict__ inverses) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float k[16], w[16], sc[16], ki[16], wi[16], si[16], m[16];
    load4(K, k);
    load4(world, w);
    load4(scale, sc);
    unproject_eval(k, w, sc, m, ki, wi, si);
    store4(M, m);
    if (inverses != nullptr) {
        store4(inverses, ki);
        store4(inverses + 16, wi);
        store4(inverses + 32, si);
    }
}

// ------------------------------------------------------------------------------------
// camera rays (rendering.py:52-80 with transform_to_world / origin_to_world, common.py:112-215):
//   o = M[:3,3];  v = M[:3,:3] (x, y, 1) = P1 - o;  |v|;  P_d - o = M[:3,:3] (x d, y d, d)
//   normalise: dir = v/|v|, d_src = |P_d - o|;  else dir = v, d_src = |P_d - o| / |v|
//   mask = isfinite(d_src) & d_src != 0;  view = -dir (use_ray_dir) or 1
constexpr int CR_THREADS = 256;

__global__ __launch_bounds__(CR_THREADS) void k_camera_rays(const float* __restrict__ Mg, const float* __restrict__ pix,
                                                            const float* __restrict__ depth, int R, int flags,
                                                            float* __restrict__ cam, float* __restrict__ ray,
                                                            float* __restrict__ view, float* __restrict__ ray_norm,
                                                            float* __restrict__ d_src, uint8_t* __restrict__ mask) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    float M[16];
    load4(Mg, M);
    camera_ray_eval(M, pix[2 * r], pix[2 * r + 1], depth != nullptr, depth != nullptr ? depth[r] : 0.f, r, flags,
                    cam, ray, view, ray_norm, d_src, mask);
}

// Backward: gradient of (cam, ray, view, ray_norm, d_src) w.r.t. M (16, rows 3 stay 0) and
// depth.  One workgroup; per-thread partial sums over a fixed ray stride, then a fixed-order
// tree (deterministic).  Rays with d = 0 contribute nothing through d_src, as torch's norm
// backward at 0.
__global__ __launch_bounds__(1024) void k_camera_rays_bwd(const float* __restrict__ Mg, const float* __restrict__ pix,
                                                          const float* __restrict__ depth, int R, int flags,
                                                          const float* __restrict__ g_cam,
                                                          const float* __restrict__ g_ray,
                                                          const float* __restrict__ g_view,
                                                          const float* __restrict__ g_norm,
                                                          const float* __restrict__ g_dsrc,
                                                          float* __restrict__ gM, float* __restrict__ g_depth) {
    __shared__ float red[16][12];
    float M[16];
    load4(Mg, M);
    const bool normalise = flags & NERF_RAYS_NORMALISE;
    float acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.f;
    for (int r = threadIdx.x; r < R; r += blockDim.x) {
        const float x = pix[2 * r], y = pix[2 * r + 1];
        float v[3], n2 = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v[i] = M[4 * i] * x + M[4 * i + 1] * y + M[4 * i + 2];
            n2 += v[i] * v[i];
        }
        const float n = sqrtf(n2), inv_n = 1.f / n;
        float gv[3] = {0.f, 0.f, 0.f};
        // direction (and view = -direction)
        float gd[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gd[i] = g_ray ? g_ray[3 * r + i] : 0.f;
            if (g_view && !(flags & NERF_RAYS_VIEW_ONES)) gd[i] -= g_view[3 * r + i];
        }
        if (normalise) {
            const float dot = (gd[0] * v[0] + gd[1] * v[1] + gd[2] * v[2]) * inv_n;
#pragma unroll
            for (int i = 0; i < 3; ++i) gv[i] += (gd[i] - v[i] * inv_n * dot) * inv_n;
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) gv[i] += gd[i];
        }
        if (g_norm) {
            const float g = g_norm[r] * inv_n;
#pragma unroll
            for (int i = 0; i < 3; ++i) gv[i] += g * v[i];
        }
        float gdep = 0.f;
        if (depth != nullptr && g_dsrc != nullptr) {
            const float d = depth[r], g = g_dsrc[r];
            if (d != 0.f) {
                const float ad = fabsf(d), sd = d > 0.f ? 1.f : -1.f;
                if (normalise) {            // d_src = |d| |v|
                    gdep = g * sd * n;
                    const float gg = g * ad * inv_n;
#pragma unroll
                    for (int i = 0; i < 3; ++i) gv[i] += gg * v[i];
                } else {                    // d_src = |d| |v| / |v|
                    gdep = g * sd;
                }
            }
        }
        if (g_depth != nullptr) g_depth[r] = gdep;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            acc[3 * i] += gv[i] * x;
            acc[3 * i + 1] += gv[i] * y;
            acc[3 * i + 2] += gv[i];
            if (g_cam) acc[9 + i] += g_cam[3 * r + i];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const float s = wave_sum(acc[i]);
        if (lane == 0) red[wv][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int e = threadIdx.x, row = e >> 2, col = e & 3;
        float s = 0.f;
        if (row < 3) {
            const int slot = col < 3 ? 3 * row + col : 9 + row;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w][slot];
        }
        gM[e] = s;
    }
}

// ------------------------------------------------------------------------------------
// NDC warp of the LLFF configs (common.py:632-675 called from rendering.py:169-181 with near = 1,
// and rendering.py:158-159's d_gt = 1 - 1 / d_src), one thread per ray:
//   t = -(near + o_z) / d_z;  p = o + t d (the origin shifted to the near plane, p_z = -near);
//   ox = p_x / p_z, oy = p_y / p_z, o2 = 1 + 2 near / p_z;  a = -1 / (1 / fx), b = -1 / (1 / fy);
//   o_ndc = (a ox, b oy, o2);  d_ndc = (a (d_x / d_z - ox), b (d_y / d_z - oy), 1 - o2)
// in the reference's operation order, f32, contraction off.  fx = K[0], fy = K[5] are read here.
constexpr int NDC_THREADS = 256;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(NDC_THREADS) void k_ndc_rays(const float* __restrict__ cam, const float* __restrict__ ray,
                                                          const float* __restrict__ K, float near, int R,
                                                          const float* __restrict__ d_src, float* __restrict__ o_ndc,
                                                          float* __restrict__ d_ndc, float* __restrict__ d_gt) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const float fx = K[0], fy = K[5];
    const float o0 = cam[3 * r], o1 = cam[3 * r + 1], o2 = cam[3 * r + 2];
    const float d0 = ray[3 * r], d1 = ray[3 * r + 1], d2 = ray[3 * r + 2];
    const float t = -(near + o2) / d2;
    const float p0 = o0 + t * d0, p1 = o1 + t * d1, p2 = o2 + t * d2;
    const float ox = p0 / p2, oy = p1 / p2;
    const float z = 1.0f + (2.0f * near) / p2;
    const float a = -1.0f / (1.0f / fx), b = -1.0f / (1.0f / fy);
    o_ndc[3 * r] = a * ox;
    o_ndc[3 * r + 1] = b * oy;
    o_ndc[3 * r + 2] = z;
    d_ndc[3 * r] = a * (d0 / d2 - ox);
    d_ndc[3 * r + 1] = b * (d1 / d2 - oy);
    d_ndc[3 * r + 2] = 1.0f - z;
    if (d_gt != nullptr) d_gt[r] = 1.0f - 1.0f / d_src[r];
}

// Its backward, in closed form rather than along the chain of the expressions: the shifted
// origin's z is -near whatever the ray, so o2 and 1 - o2 are constants (their upstream gradients
// reach nothing) and 1 / p_z = -1 / near; a = -fx, b = -fy.  With r0 = d_x / d_z, r1 = d_y / d_z:
//   g_ox = a (gO_x - gD_x), g_p0 = -g_ox / near (same in y);  g_t = g_p0 d_x + g_p1 d_y
//   g_cam = (g_p0, g_p1, -g_t / d_z)
//   g_ray = (g_p0 t + a gD_x / d_z, g_p1 t + b gD_y / d_z, -(g_t t + a gD_x r0 + b gD_y r1) / d_z)
//   g_fx = -sum gO_x ox + gD_x (r0 - ox), g_fy likewise;  g_dsrc = g_dgt / d_src^2
// evaluated in f64 from the f32 inputs and rounded once.  Without gK every block takes its own
// rays; with gK the launch is one workgroup that walks all rays, and the two focal sums are f64
// per-thread sums over a fixed ray stride, a wave butterfly, then the wave sums in order
// (deterministic, no atomics).
constexpr int NDC_BWD_THREADS = 1024;

__global__ __launch_bounds__(NDC_BWD_THREADS) void k_ndc_rays_bwd(
    const float* __restrict__ cam, const float* __restrict__ ray, const float* __restrict__ K, float near, int R,
    const float* __restrict__ d_src, const float* __restrict__ g_o, const float* __restrict__ g_d,
    const float* __restrict__ g_dgt, float* __restrict__ g_cam, float* __restrict__ g_ray, float* __restrict__ gK,
    float* __restrict__ g_dsrc) {
    __shared__ double red[NDC_BWD_THREADS / 64][2];
    const double a = -(double)K[0], b = -(double)K[5], ip2 = -1.0 / (double)near;
    double sfx = 0.0, sfy = 0.0;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
        const double o0 = cam[3 * r], o1 = cam[3 * r + 1], o2 = cam[3 * r + 2];
        const double d0 = ray[3 * r], d1 = ray[3 * r + 1], d2 = ray[3 * r + 2];
        const double t = -((double)near + o2) / d2;
        const double ox = (o0 + t * d0) * ip2, oy = (o1 + t * d1) * ip2;
        const double r0 = d0 / d2, r1 = d1 / d2;
        const double gO0 = g_o ? (double)g_o[3 * r] : 0.0, gO1 = g_o ? (double)g_o[3 * r + 1] : 0.0;
        const double gD0 = g_d ? (double)g_d[3 * r] : 0.0, gD1 = g_d ? (double)g_d[3 * r + 1] : 0.0;
        const double g_r0 = a * gD0, g_r1 = b * gD1;
        const double g_p0 = a * (gO0 - gD0) * ip2, g_p1 = b * (gO1 - gD1) * ip2;
        const double g_t = g_p0 * d0 + g_p1 * d1;
        g_cam[3 * r] = (float)g_p0;
        g_cam[3 * r + 1] = (float)g_p1;
        g_cam[3 * r + 2] = (float)(-g_t / d2);
        g_ray[3 * r] = (float)(g_p0 * t + g_r0 / d2);
        g_ray[3 * r + 1] = (float)(g_p1 * t + g_r1 / d2);
        g_ray[3 * r + 2] = (float)(-(g_t * t + g_r0 * r0 + g_r1 * r1) / d2);
        sfx -= gO0 * ox + gD0 * (r0 - ox);
        sfy -= gO1 * oy + gD1 * (r1 - oy);
        if (g_dsrc != nullptr) {
            // a ray whose d_gt took no gradient passes none on: 0, not 0 / 0, at d_src = 0 (the
            // rays without a depth prior, which the dense depth loss masks out)
            const double ds = d_src[r], g = g_dgt ? (double)g_dgt[r] : 0.0;
            g_dsrc[r] = g != 0.0 ? (float)(g / (ds * ds)) : 0.f;
        }
    }
    if (gK == nullptr) return;      // the same for every thread of the launch
    sfx = wave_sum_d(sfx);
    sfy = wave_sum_d(sfy);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { red[wv][0] = sfx; red[wv][1] = sfy; }
    __syncthreads();
    if (threadIdx.x < 16) {
        double s = 0.0;
        if (threadIdx.x == 0 || threadIdx.x == 5)
            for (int w = 0; w < NDC_BWD_THREADS / 64; ++w) s += red[w][threadIdx.x == 0 ? 0 : 1];
        gK[threadIdx.x] = (float)s;
    }
}

// ------------------------------------------------------------------------------------
// losses.py:28-33 (rgb l1/l2 over R rays), :60-66 (depth l1 over the masked rays), l2_mean
// = mse(rgb, gt), total = w_rgb l_rgb + w_depth l_depth.  out = {total, l_rgb, l_depth,
// l2_mean} (four scalars), cnt = number of depth rays used (for the backward).
__global__ __launch_bounds__(1024) void k_ray_loss(const float* __restrict__ rgb, const float* __restrict__ gt,
                                                   int R, const float* __restrict__ dp,
                                                   const float* __restrict__ dg, const uint8_t* __restrict__ mask,
                                                   int M, int l1, float w_rgb, float w_depth,
                                                   float* __restrict__ total, float* __restrict__ l_rgb,
                                                   float* __restrict__ l_depth, float* __restrict__ l2_mean,
                                                   float* __restrict__ cnt_out) {
    __shared__ float red[16][4];
    float s2 = 0.f, s1 = 0.f, sd = 0.f, cnt = 0.f;
    for (int i = threadIdx.x; i < 3 * R; i += blockDim.x) {
        const float e = rgb[i] - gt[i];
        s2 += e * e;
        s1 += fabsf(e);
    }
    if (dp != nullptr)
        for (int i = threadIdx.x; i < M; i += blockDim.x) {
            if (mask == nullptr || mask[i]) {
                sd += fabsf(dp[i] - dg[i]);
                cnt += 1.f;
            }
        }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    s2 = wave_sum(s2); s1 = wave_sum(s1); sd = wave_sum(sd); cnt = wave_sum(cnt);
    if (lane == 0) { red[wv][0] = s2; red[wv][1] = s1; red[wv][2] = sd; red[wv][3] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = 0.f, b = 0.f, c = 0.f, n = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { a += red[w][0]; b += red[w][1]; c += red[w][2]; n += red[w][3]; }
        const float lr = (l1 ? b : a) / (float)R;
        const float ld = dp != nullptr ? c / fmaxf(n, 1.f) : 0.f;   // 0 (not 0/0) with no valid ray
        *l_rgb = lr;
        *l_depth = ld;
        *l2_mean = a / (float)(3 * R);
        *total = w_rgb * lr + w_depth * ld;
        *cnt_out = n;
    }
}

// d(total, l_rgb, l_depth, l2_mean)/d(rgb, depth_pred, depth_gt) contracted with the
// upstream scalars go[0..3] (NULL = 0)
__global__ void k_ray_loss_bwd(const float* __restrict__ rgb, const float* __restrict__ gt, int R,
                               const float* __restrict__ dp, const float* __restrict__ dg,
                               const uint8_t* __restrict__ mask, int M, int l1, float w_rgb, float w_depth,
                               const float* __restrict__ go_total, const float* __restrict__ go_rgb,
                               const float* __restrict__ go_depth, const float* __restrict__ go_l2,
                               const float* __restrict__ cnt, float* __restrict__ g_rgb,
                               float* __restrict__ g_dp, float* __restrict__ g_dg) {
    const float gt_ = go_total ? *go_total : 0.f;
    const float a_rgb = gt_ * w_rgb + (go_rgb ? *go_rgb : 0.f);
    const float a_dep = gt_ * w_depth + (go_depth ? *go_depth : 0.f);
    const float a_l2 = go_l2 ? *go_l2 : 0.f;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (g_rgb != nullptr && i < 3 * R) {
        const float e = rgb[i] - gt[i];
        const float dl = l1 ? (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) : 2.f * e;
        g_rgb[i] = a_rgb * dl / (float)R + a_l2 * (2.f * e) / (float)(3 * R);
    }
    if (dp != nullptr && i < M) {
        float g = 0.f;
        if (mask == nullptr || mask[i]) {
            const float e = dp[i] - dg[i];
            g = a_dep * (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) / fmaxf(*cnt, 1.f);
        }
        if (g_dp) g_dp[i] = g;
        if (g_dg) g_dg[i] = -g;
    }
}

// ------------------------------------------------------------------------------------
// depth_loss_type 'invariant' (losses.py:35-58 through get_depth_loss :67-68) beside the rgb terms
// of k_ray_loss: over the masked entries, t = torch.median (the value of 0-based rank (cnt - 1) / 2),
// s = mean |d - t| for the prediction and the prior, l_depth = mean(((p - t_p) / s_p - (g - t_g) / s_g)^2).
// One workgroup; thread tid holds entries tid + q LI_THREADS in registers.  The median is a
// radix select on order-preserving keys, most significant bit first, one block-wide count per bit
// for both medians at once -- exact, whatever the values.  The depth arithmetic and its sums run in
// f64 in a fixed order (per-thread, wave butterfly, 16 wave sums in order): deterministic.
constexpr int LI_THREADS = 1024, LI_PER = NERF_SAMPLE_MAX_RAYS / LI_THREADS, LI_WAVES = LI_THREADS / 64;

__device__ __forceinline__ uint32_t float_key(float x) {     // a < b  <=>  key(a) < key(b), finite a, b
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// the sums of v[0..N) over the workgroup, the same bits in every thread; red: [LI_WAVES][N]
template <int N>
__device__ __forceinline__ void block_sum_d(double (&v)[N], double* red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum_d(v[i]);
    __syncthreads();   // the readers of an earlier use of red are done
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) red[wv * N + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = 0.0;
        for (int w = 0; w < LI_WAVES; ++w) s += red[w * N + i];
        v[i] = s;
    }
}

// stats = {cnt, t_p, s_p, t_g, s_g, entries equal to t_p, entries equal to t_g, 0} (s_p, s_g: for the caller)
__global__ __launch_bounds__(LI_THREADS) void k_ray_loss_inv(const float* __restrict__ rgb,
                                                             const float* __restrict__ gt, int R,
                                                             const float* __restrict__ dp,
                                                             const float* __restrict__ dg,
                                                             const uint8_t* __restrict__ mask, int M, int l1,
                                                             float w_rgb, float w_depth, float* __restrict__ total,
                                                             float* __restrict__ l_rgb, float* __restrict__ l_depth,
                                                             float* __restrict__ l2_mean,
                                                             float* __restrict__ stats) {
    __shared__ float red[LI_WAVES][2];
    __shared__ int cred[2][LI_WAVES];
    __shared__ double dred[LI_WAVES * 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the rgb sums, as k_ray_loss takes them
    float s2 = 0.f, s1 = 0.f;
    for (int i = tid; i < 3 * R; i += LI_THREADS) {
        const float e = rgb[i] - gt[i];
        s2 += e * e;
        s1 += fabsf(e);
    }
    s2 = wave_sum(s2); s1 = wave_sum(s1);
    if (lane == 0) { red[wv][0] = s2; red[wv][1] = s1; }
    float p[LI_PER], g[LI_PER];
    uint32_t kp[LI_PER], kg[LI_PER];
    bool m[LI_PER];
    int mine = 0;
#pragma unroll
    for (int q = 0; q < LI_PER; ++q) {
        const int i = tid + q * LI_THREADS;
        m[q] = i < M && (mask == nullptr || mask[i] != 0);
        p[q] = m[q] ? dp[i] : 0.f;
        g[q] = m[q] ? dg[i] : 0.f;
        kp[q] = float_key(p[q]);
        kg[q] = float_key(g[q]);
        mine += m[q] ? 1 : 0;
    }
    double c1[1] = {(double)mine};
    block_sum_d<1>(c1, dred);          // its barriers also publish red
    const int cnt = (int)c1[0];
    // rank (cnt - 1) / 2 of both key sets: bit by bit, the count of keys that share the prefix so
    // far and have a 0 next (the two counts packed in one int: each is at most 4096)
    uint32_t pre_p = 0u, pre_g = 0u;
    int rk_p = (cnt - 1) / 2, rk_g = rk_p;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t above = ~((2u << bit) - 1u);   // the bits above `bit` (0 at bit 31)
        int c0 = 0;
#pragma unroll
        for (int q = 0; q < LI_PER; ++q) {
            if (!m[q]) continue;
            c0 += ((kp[q] & above) == pre_p && !((kp[q] >> bit) & 1u)) ? 1 : 0;
            c0 += ((kg[q] & above) == pre_g && !((kg[q] >> bit) & 1u)) ? 65536 : 0;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c0 += __shfl_xor(c0, off, 64);
        int* cr = cred[bit & 1];       // two buffers: one barrier per bit
        if (lane == 0) cr[wv] = c0;
        __syncthreads();
        int n0 = 0;
        for (int w = 0; w < LI_WAVES; ++w) n0 += cr[w];
        const int n0p = n0 & 0xffff, n0g = n0 >> 16;
        if (rk_p >= n0p) { rk_p -= n0p; pre_p |= 1u << bit; }
        if (rk_g >= n0g) { rk_g -= n0g; pre_g |= 1u << bit; }
    }
    const float t_p = key_float(pre_p), t_g = key_float(pre_g);   // cnt = 0: all ones, a NaN
    double ep[LI_PER], eg[LI_PER], v4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < LI_PER; ++q) {
        ep[q] = (double)p[q] - (double)t_p;
        eg[q] = (double)g[q] - (double)t_g;
        if (!m[q]) continue;
        v4[0] += fabs(ep[q]);
        v4[1] += fabs(eg[q]);
        v4[2] += p[q] == t_p ? 1.0 : 0.0;
        v4[3] += g[q] == t_g ? 1.0 : 0.0;
    }
    block_sum_d<4>(v4, dred);
    const double s_p = v4[0] / (double)cnt, s_g = v4[1] / (double)cnt;   // 0 / 0 with no entry
    double sq[1] = {0.0};
#pragma unroll
    for (int q = 0; q < LI_PER; ++q) {
        if (!m[q]) continue;
        const double r = ep[q] / s_p - eg[q] / s_g;
        sq[0] += r * r;
    }
    block_sum_d<1>(sq, dred);
    if (tid == 0) {
        float a = 0.f, b = 0.f;
        for (int w = 0; w < LI_WAVES; ++w) { a += red[w][0]; b += red[w][1]; }
        const float lr = (l1 ? b : a) / (float)R;
        const float ld = (float)(sq[0] / (double)cnt);
        *l_rgb = lr;
        *l_depth = ld;
        *l2_mean = a / (float)(3 * R);
        *total = w_rgb * lr + w_depth * ld;
        stats[0] = (float)cnt; stats[1] = t_p; stats[2] = (float)s_p; stats[3] = t_g; stats[4] = (float)s_g;
        stats[5] = (float)v4[2]; stats[6] = (float)v4[3]; stats[7] = 0.f;
    }
}

// Its backward, what torch autograd gives for the expressions above: with u = (p - t_p) / s_p,
// v = (g - t_g) / s_g, a_i = a_dep 2 (u_i - v_i) / cnt, A = sum a, B_p = sum a u, B_g = sum a v,
// S = sum sign(d - t) and m_j = [d_j == t] / ties (the median's gradient, spread evenly over the
// entries equal to it; sign(0) = 0):
//   g_p[j] = (a_j - A m_j - B_p (sign_j - S_p m_j) / cnt) / s_p
//   g_g[j] = (-a_j + A m'_j + B_g (sign'_j - S_g m'_j) / cnt) / s_g
// Entries outside the mask get 0; without go_total and go_depth every depth gradient is 0.
// s = 0 (cnt <= 1, or all entries equal) gives NaN on every masked entry, as autograd does.
__global__ __launch_bounds__(LI_THREADS) void k_ray_loss_inv_bwd(
    const float* __restrict__ rgb, const float* __restrict__ gt, int R, const float* __restrict__ dp,
    const float* __restrict__ dg, const uint8_t* __restrict__ mask, int M, int l1, float w_rgb, float w_depth,
    const float* __restrict__ go_total, const float* __restrict__ go_rgb, const float* __restrict__ go_depth,
    const float* __restrict__ go_l2, const float* __restrict__ stats, float* __restrict__ g_rgb,
    float* __restrict__ g_dp, float* __restrict__ g_dg) {
    __shared__ double dred[LI_WAVES * 5];
    const int tid = threadIdx.x;
    const float gt_ = go_total ? *go_total : 0.f;
    const float a_rgb = gt_ * w_rgb + (go_rgb ? *go_rgb : 0.f);
    const float a_dep = gt_ * w_depth + (go_depth ? *go_depth : 0.f);
    const float a_l2 = go_l2 ? *go_l2 : 0.f;
    if (g_rgb != nullptr)
        for (int i = tid; i < 3 * R; i += LI_THREADS) {
            const float e = rgb[i] - gt[i];
            const float dl = l1 ? (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f)) : 2.f * e;
            g_rgb[i] = a_rgb * dl / (float)R + a_l2 * (2.f * e) / (float)(3 * R);
        }
    if (g_dp == nullptr && g_dg == nullptr) return;
    if (go_total == nullptr && go_depth == nullptr) {      // l_depth reaches no upstream scalar
        for (int i = tid; i < M; i += LI_THREADS) {
            if (g_dp) g_dp[i] = 0.f;
            if (g_dg) g_dg[i] = 0.f;
        }
        return;
    }
    // the count, the medians and their tie counts come from the forward; s is summed again from them, in
    // the forward's order, so that it is the forward's f64 value and not its f32 copy in stats
    const double cnt = stats[0], t_p = stats[1], t_g = stats[3], ties_p = stats[5], ties_g = stats[6];
    bool m[LI_PER];
    double ep[LI_PER], eg[LI_PER], a[LI_PER], v2[2] = {0.0, 0.0}, v5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    auto sgn = [](double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); };
#pragma unroll
    for (int q = 0; q < LI_PER; ++q) {
        const int i = tid + q * LI_THREADS;
        m[q] = i < M && (mask == nullptr || mask[i] != 0);
        ep[q] = m[q] ? (double)dp[i] - t_p : 0.0;
        eg[q] = m[q] ? (double)dg[i] - t_g : 0.0;
        v2[0] += fabs(ep[q]);
        v2[1] += fabs(eg[q]);
    }
    block_sum_d<2>(v2, dred);
    const double s_p = v2[0] / cnt, s_g = v2[1] / cnt;
#pragma unroll
    for (int q = 0; q < LI_PER; ++q) {
        a[q] = 0.0;
        if (!m[q]) continue;
        const double u = ep[q] / s_p, v = eg[q] / s_g;
        a[q] = (double)a_dep * 2.0 * (u - v) / cnt;
        v5[0] += a[q];
        v5[1] += a[q] * u;
        v5[2] += a[q] * v;
        v5[3] += sgn(ep[q]);
        v5[4] += sgn(eg[q]);
    }
    block_sum_d<5>(v5, dred);
#pragma unroll
    for (int q = 0; q < LI_PER; ++q) {
        const int i = tid + q * LI_THREADS;
        if (i >= M) continue;
        float gp = 0.f, gg = 0.f;
        if (m[q]) {
            const double mp = ep[q] == 0.0 ? 1.0 / ties_p : 0.0, mg = eg[q] == 0.0 ? 1.0 / ties_g : 0.0;
            gp = (float)((a[q] - v5[0] * mp - v5[1] * (sgn(ep[q]) - v5[3] * mp) / cnt) / s_p);
            gg = (float)((-a[q] + v5[0] * mg + v5[2] * (sgn(eg[q]) - v5[4] * mg) / cnt) / s_g);
        }
        if (g_dp) g_dp[i] = gp;
        if (g_dg) g_dg[i] = gg;
    }
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_sample_rays(int n_pix, int n_rays, uint64_t seed, int width, int height, const float* img,
                                int64_t* idx, float* pixels, float* rgb, int* status, uint64_t* seed_counter,
                                void* stream) {
    NERF_CHECK_PTR(idx);
    NERF_CHECK(n_rays > 0 && n_rays <= NERF_SAMPLE_MAX_RAYS, "%s: n_rays=%d outside 1..%d", __func__, n_rays,
               NERF_SAMPLE_MAX_RAYS);
    NERF_CHECK(n_pix >= 2 * n_rays, "%s: n_pix=%d < 2*n_rays=%d (draw a permutation instead)", __func__, n_pix,
               2 * n_rays);
    NERF_CHECK(pixels == nullptr || (width > 1 && height > 1 && width * height == n_pix),
               "%s: pixels need width, height > 1 with width*height == n_pix", __func__);
    NERF_CHECK(rgb == nullptr || (img != nullptr && width * height == n_pix), "%s: rgb needs img [3][n_pix]",
               __func__);
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    hipLaunchKernelGGL(k_sample_rays, dim3(1), dim3(SR_THREADS), 0, as_stream(stream), n_pix, n_rays, key,
                       width, height, img, idx, pixels, rgb, status,
                       reinterpret_cast<unsigned long long*>(seed_counter));
    return check_launch(__func__);
}

extern "C" int nerf_sample_rays_valid(int n_pix, int n_rays, uint64_t seed, int width, int height,
                                      const float* img, const uint8_t* valid, int64_t* idx, float* pixels,
                                      float* rgb, int* status, int* attempts, uint64_t* seed_counter,
                                      void* stream) {
    if (valid == nullptr && attempts == nullptr)      // no mask, nothing to report: today's launch
        return nerf_sample_rays(n_pix, n_rays, seed, width, height, img, idx, pixels, rgb, status, seed_counter,
                                stream);
    NERF_CHECK_PTR(idx);
    NERF_CHECK(n_rays > 0 && n_rays <= NERF_SAMPLE_MAX_RAYS, "%s: n_rays=%d outside 1..%d", __func__, n_rays,
               NERF_SAMPLE_MAX_RAYS);
    NERF_CHECK(n_pix >= 2 * n_rays, "%s: n_pix=%d < 2*n_rays=%d (draw a permutation instead)", __func__, n_pix,
               2 * n_rays);
    NERF_CHECK(pixels == nullptr || (width > 1 && height > 1 && width * height == n_pix),
               "%s: pixels need width, height > 1 with width*height == n_pix", __func__);
    NERF_CHECK(rgb == nullptr || (img != nullptr && width * height == n_pix), "%s: rgb needs img [3][n_pix]",
               __func__);
    hipLaunchKernelGGL(k_sample_rays_valid, dim3(1), dim3(SR_THREADS), 0, as_stream(stream), n_pix, n_rays,
                       (unsigned long long)seed, width, height, img, valid, idx, pixels, rgb, status, attempts,
                       reinterpret_cast<unsigned long long*>(seed_counter));
    return check_launch(__func__);
}

extern "C" int nerf_mat4_inv(const float* a, int n, float* out, void* stream) {
    NERF_CHECK_PTR(a); NERF_CHECK_PTR(out);
    NERF_CHECK(n > 0, "%s: n=%d", __func__, n);
    hipLaunchKernelGGL(k_mat4_inv, dim3((n + 63) / 64), dim3(64), 0, as_stream(stream), a, n, out);
    return check_launch(__func__);
}

extern "C" int nerf_pose_c2w(const float* r, const float* t, const float* init_c2w, float* c2w, void* stream) {
    NERF_CHECK_PTR(r); NERF_CHECK_PTR(t); NERF_CHECK_PTR(c2w);
    hipLaunchKernelGGL(k_pose_c2w, dim3(1), dim3(64), 0, as_stream(stream), r, t, init_c2w, c2w);
    return check_launch(__func__);
}

extern "C" int nerf_unproject_matrix(const float* K, const float* world, const float* scale, float* M,
                                     float* inverses, void* stream) {
    NERF_CHECK_PTR(K); NERF_CHECK_PTR(world); NERF_CHECK_PTR(scale); NERF_CHECK_PTR(M);
    hipLaunchKernelGGL(k_unproject, dim3(1), dim3(64), 0, as_stream(stream), K, world, scale, M, inverses);
    return check_launch(__func__);
}

extern "C" int nerf_pose_c2w_bwd(const float* r, const float* init_c2w, const float* g_c2w, float* g_r, float* g_t,
                                 void* stream) {
    NERF_CHECK_PTR(r); NERF_CHECK_PTR(g_c2w);
    hipLaunchKernelGGL(k_pose_c2w_bwd, dim3(1), dim3(64), 0, as_stream(stream), r, init_c2w, g_c2w, g_r, g_t);
    return check_launch(__func__);
}

extern "C" int nerf_mat4_inv_bwd(const float* inv_a, const float* g, int n, float* g_a, void* stream) {
    NERF_CHECK_PTR(inv_a); NERF_CHECK_PTR(g); NERF_CHECK_PTR(g_a);
    NERF_CHECK(n > 0, "%s: n=%d", __func__, n);
    hipLaunchKernelGGL(k_mat4_inv_bwd, dim3((n + 63) / 64), dim3(64), 0, as_stream(stream), inv_a, g, n, g_a);
    return check_launch(__func__);
}

extern "C" int nerf_mat4_mul(const float* a, const float* b, int n, float* c, void* stream) {
    NERF_CHECK_PTR(a); NERF_CHECK_PTR(b); NERF_CHECK_PTR(c);
    NERF_CHECK(n > 0, "%s: n=%d", __func__, n);
    hipLaunchKernelGGL(k_mat4_mul, dim3((n + 63) / 64), dim3(64), 0, as_stream(stream), a, b, n, c);
    return check_launch(__func__);
}

extern "C" int nerf_mat4_mul_bwd(const float* a, const float* b, const float* g, int n, float* g_a, float* g_b,
                                 void* stream) {
    NERF_CHECK_PTR(g);
    NERF_CHECK(n > 0, "%s: n=%d", __func__, n);
    NERF_CHECK(g_a == nullptr || b != nullptr, "%s: g_a needs b", __func__);
    NERF_CHECK(g_b == nullptr || a != nullptr, "%s: g_b needs a", __func__);
    hipLaunchKernelGGL(k_mat4_mul_bwd, dim3((n + 63) / 64), dim3(64), 0, as_stream(stream), a, b, g, n, g_a, g_b);
    return check_launch(__func__);
}

extern "C" int nerf_unproject_matrix_bwd(const float* inverses, const float* g_M, float* g_K, float* g_world,
                                         float* g_scale, void* stream) {
    NERF_CHECK_PTR(inverses); NERF_CHECK_PTR(g_M);
    hipLaunchKernelGGL(k_unproject_bwd, dim3(1), dim3(64), 0, as_stream(stream), inverses, g_M, g_K, g_world,
                       g_scale);
    return check_launch(__func__);
}

extern "C" int nerf_depth_affine(const float* d, int n, const float* scale, const float* shift, int shift_first,
                                 float lo, float* y, void* stream) {
    NERF_CHECK_PTR(d); NERF_CHECK_PTR(scale); NERF_CHECK_PTR(shift); NERF_CHECK_PTR(y);
    NERF_CHECK(n > 0, "%s: n=%d", __func__, n);
    const int blocks = (n + AF_THREADS - 1) / AF_THREADS;
    hipLaunchKernelGGL(k_depth_affine, dim3(blocks < 64 ? blocks : 64), dim3(AF_THREADS), 0, as_stream(stream), d,
                       n, scale, shift, shift_first, lo, y);
    return check_launch(__func__);
}

extern "C" int nerf_depth_affine_bwd(const float* d, int n, const float* scale, const float* shift, int shift_first,
                                     float lo, const float* g, float* g_scale, float* g_shift, void* stream) {
    NERF_CHECK_PTR(d); NERF_CHECK_PTR(scale); NERF_CHECK_PTR(shift); NERF_CHECK_PTR(g);
    NERF_CHECK(n > 0, "%s: n=%d", __func__, n);
    hipLaunchKernelGGL(k_depth_affine_bwd, dim3(1), dim3(AF_THREADS), 0, as_stream(stream), d, n, scale, shift,
                       shift_first, lo, g, g_scale, g_shift);
    return check_launch(__func__);
}

extern "C" int nerf_camera_rays(const float* M, const float* pixels, const float* depth, int n_rays, int flags,
                                float* cam, float* ray, float* view, float* ray_norm, float* d_src, uint8_t* mask,
                                void* stream) {
    NERF_CHECK_PTR(M); NERF_CHECK_PTR(pixels); NERF_CHECK_PTR(cam); NERF_CHECK_PTR(ray);
    NERF_CHECK_PTR(ray_norm); NERF_CHECK_PTR(d_src);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    hipLaunchKernelGGL(k_camera_rays, dim3((n_rays + CR_THREADS - 1) / CR_THREADS), dim3(CR_THREADS), 0,
                       as_stream(stream), M, pixels, depth, n_rays, flags, cam, ray, view, ray_norm, d_src, mask);
    return check_launch(__func__);
}

extern "C" int nerf_camera_rays_bwd(const float* M, const float* pixels, const float* depth, int n_rays, int flags,
                                    const float* g_cam, const float* g_ray, const float* g_view,
                                    const float* g_norm, const float* g_dsrc, float* gM, float* g_depth,
                                    void* stream) {
    NERF_CHECK_PTR(M); NERF_CHECK_PTR(pixels); NERF_CHECK_PTR(gM);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK(g_depth == nullptr || depth != nullptr, "%s: g_depth without depth", __func__);
    hipLaunchKernelGGL(k_camera_rays_bwd, dim3(1), dim3(1024), 0, as_stream(stream), M, pixels, depth, n_rays,
                       flags, g_cam, g_ray, g_view, g_norm, g_dsrc, gM, g_depth);
    return check_launch(__func__);
}

extern "C" int nerf_ndc_rays(const float* cam, const float* ray, const float* K, float near, int n_rays,
                             const float* d_src, float* o_ndc, float* d_ndc, float* d_gt, void* stream) {
    NERF_CHECK_PTR(cam); NERF_CHECK_PTR(ray); NERF_CHECK_PTR(K); NERF_CHECK_PTR(o_ndc); NERF_CHECK_PTR(d_ndc);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK(d_gt == nullptr || d_src != nullptr, "%s: d_gt without d_src", __func__);
    hipLaunchKernelGGL(k_ndc_rays, dim3((n_rays + NDC_THREADS - 1) / NDC_THREADS), dim3(NDC_THREADS), 0,
                       as_stream(stream), cam, ray, K, near, n_rays, d_src, o_ndc, d_ndc, d_gt);
    return check_launch(__func__);
}

extern "C" int nerf_ndc_rays_bwd(const float* cam, const float* ray, const float* K, float near, int n_rays,
                                 const float* d_src, const float* g_o, const float* g_d, const float* g_dgt,
                                 float* g_cam, float* g_ray, float* gK, float* g_dsrc, void* stream) {
    NERF_CHECK_PTR(cam); NERF_CHECK_PTR(ray); NERF_CHECK_PTR(K); NERF_CHECK_PTR(g_cam); NERF_CHECK_PTR(g_ray);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK(g_dsrc == nullptr || d_src != nullptr, "%s: g_dsrc without d_src", __func__);
    // the focal sums need every ray in one workgroup; without them the rays spread over the grid
    const int blocks = gK != nullptr ? 1 : (n_rays + NDC_BWD_THREADS - 1) / NDC_BWD_THREADS;
    hipLaunchKernelGGL(k_ndc_rays_bwd, dim3(blocks), dim3(NDC_BWD_THREADS), 0, as_stream(stream), cam, ray, K, near,
                       n_rays, d_src, g_o, g_d, g_dgt, g_cam, g_ray, gK, g_dsrc);
    return check_launch(__func__);
}

extern "C" int nerf_ray_loss(const float* rgb, const float* rgb_gt, int n_rays, const float* depth_pred,
                             const float* depth_gt, const uint8_t* mask, int n_depth, int rgb_l1, float w_rgb,
                             float w_depth, float* total, float* l_rgb, float* l_depth, float* l2_mean,
                             float* cnt, void* stream) {
    NERF_CHECK_PTR(rgb); NERF_CHECK_PTR(rgb_gt); NERF_CHECK_PTR(total); NERF_CHECK_PTR(l_rgb);
    NERF_CHECK_PTR(l_depth); NERF_CHECK_PTR(l2_mean); NERF_CHECK_PTR(cnt);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK(depth_pred == nullptr || (depth_gt != nullptr && n_depth >= 0), "%s: depth_pred without depth_gt",
               __func__);
    hipLaunchKernelGGL(k_ray_loss, dim3(1), dim3(1024), 0, as_stream(stream), rgb, rgb_gt, n_rays, depth_pred,
                       depth_gt, mask, n_depth, rgb_l1, w_rgb, w_depth, total, l_rgb, l_depth, l2_mean, cnt);
    return check_launch(__func__);
}

extern "C" int nerf_ray_loss_bwd(const float* rgb, const float* rgb_gt, int n_rays, const float* depth_pred,
                                 const float* depth_gt, const uint8_t* mask, int n_depth, int rgb_l1, float w_rgb,
                                 float w_depth, const float* go_total, const float* go_rgb, const float* go_depth,
                                 const float* go_l2, const float* cnt, float* g_rgb, float* g_depth_pred,
                                 float* g_depth_gt, void* stream) {
    NERF_CHECK_PTR(rgb); NERF_CHECK_PTR(rgb_gt); NERF_CHECK_PTR(cnt);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK((g_depth_pred == nullptr && g_depth_gt == nullptr) || depth_pred != nullptr,
               "%s: depth gradients without depth inputs", __func__);
    const int n = 3 * n_rays > n_depth ? 3 * n_rays : n_depth;
    hipLaunchKernelGGL(k_ray_loss_bwd, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), rgb, rgb_gt, n_rays,
                       depth_pred, depth_gt, mask, n_depth, rgb_l1, w_rgb, w_depth, go_total, go_rgb, go_depth,
                       go_l2, cnt, g_rgb, g_depth_pred, g_depth_gt);
    return check_launch(__func__);
}

extern "C" int nerf_ray_loss_invariant(const float* rgb, const float* rgb_gt, int n_rays, const float* depth_pred,
                                       const float* depth_gt, const uint8_t* mask, int n_depth, int rgb_l1,
                                       float w_rgb, float w_depth, float* total, float* l_rgb, float* l_depth,
                                       float* l2_mean, float* stats, void* stream) {
    NERF_CHECK_PTR(rgb); NERF_CHECK_PTR(rgb_gt); NERF_CHECK_PTR(depth_pred); NERF_CHECK_PTR(depth_gt);
    NERF_CHECK_PTR(total); NERF_CHECK_PTR(l_rgb); NERF_CHECK_PTR(l_depth); NERF_CHECK_PTR(l2_mean);
    NERF_CHECK_PTR(stats);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK(n_depth >= 0 && n_depth <= NERF_SAMPLE_MAX_RAYS, "%s: n_depth=%d outside 0..%d", __func__, n_depth,
               NERF_SAMPLE_MAX_RAYS);
    hipLaunchKernelGGL(k_ray_loss_inv, dim3(1), dim3(LI_THREADS), 0, as_stream(stream), rgb, rgb_gt, n_rays,
                       depth_pred, depth_gt, mask, n_depth, rgb_l1, w_rgb, w_depth, total, l_rgb, l_depth, l2_mean,
                       stats);
    return check_launch(__func__);
}

extern "C" int nerf_ray_loss_invariant_bwd(const float* rgb, const float* rgb_gt, int n_rays,
                                           const float* depth_pred, const float* depth_gt, const uint8_t* mask,
                                           int n_depth, int rgb_l1, float w_rgb, float w_depth,
                                           const float* go_total, const float* go_rgb, const float* go_depth,
                                           const float* go_l2, const float* stats, float* g_rgb,
                                           float* g_depth_pred, float* g_depth_gt, void* stream) {
    NERF_CHECK_PTR(rgb); NERF_CHECK_PTR(rgb_gt); NERF_CHECK_PTR(depth_pred); NERF_CHECK_PTR(depth_gt);
    NERF_CHECK_PTR(stats);
    NERF_CHECK(n_rays > 0, "%s: n_rays=%d", __func__, n_rays);
    NERF_CHECK(n_depth >= 0 && n_depth <= NERF_SAMPLE_MAX_RAYS, "%s: n_depth=%d outside 0..%d", __func__, n_depth,
               NERF_SAMPLE_MAX_RAYS);
    hipLaunchKernelGGL(k_ray_loss_inv_bwd, dim3(1), dim3(LI_THREADS), 0, as_stream(stream), rgb, rgb_gt, n_rays,
                       depth_pred, depth_gt, mask, n_depth, rgb_l1, w_rgb, w_depth, go_total, go_rgb, go_depth,
                       go_l2, stats, g_rgb, g_depth_pred, g_depth_gt);
    return check_launch(__func__);
}
