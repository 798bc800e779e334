// Windowed image metrics of the novel-view evaluation (model/eval_images.py:94-97 of the
// reference: F.mse_loss + third_party/pytorch_ssim/__init__.py:8-46): per image of a batch the
// mean squared error and the mean Gaussian SSIM of two images, optionally the SSIM map.
//
// The reference runs this as five depthwise convolutions, some twenty elementwise launches and
// three reductions per frame, on permuted views of the renderer's [H,W,3] frame.  Here:
//   k_image_metrics       : one workgroup per (32 x 32 output tile, channel, image).  It stages the
//                           tile + halo of both images in LDS straight from their strided layouts,
//                           filters x, y, x^2, y^2, xy, evaluates the map and writes one (sum of
//                           squared differences, sum of SSIM) pair to the workspace;
//   k_image_metrics_final : one wavefront per image sums the pairs in a fixed order.
// No atomics: the same inputs give the same bits.
//
// Arithmetic.  sigma^2 = E[x^2] - mu^2 loses ~1e-7 / C2 = 1e-4 of the map in f32 wherever the image
// is flat and bright (the reference's own f32 map is off by up to 7.7e-4 against fp64 on a 188 x 621
// frame), so the filters and the map run in fp64 (an fp64 FMA issues at the rate of an
// unpacked f32 one) and are rounded to f32 once, at the end.
// The window is the reference's: the f32-rounded outer product fl(g_i g_j) of the f32 taps, which is
// not rank one.  A separable row + column pass applies g_i g_j unrounded; the two differ by up to
// 2^-25 per weight, and because the difference does not average out over a frame it showed as up to 1e-5
// on the map and up to 1.2e-6 on the frame mean -- the whole f32 error of the reference's mean at
// window 3.  So the 2-D window is applied as it is: each thread owns four vertically adjacent
// outputs and walks the window rows once, so a staged pixel is read once per four outputs; 5 x 121
// fp64 FMAs per output.
//
// The depth half of the same evaluation (k_depth_metrics, k_depth_metrics_final) follows the image
// metrics below.
#include "common.hpp"

#include <cmath>

namespace nerf {

constexpr int MT = 32;                  // output tile edge
constexpr int MW = 11;                  // largest window
constexpr int MS = MT + MW - 1;         // staged edge: tile + halo
constexpr int MTHREADS = 256;
constexpr int MR = MT * MT / MTHREADS;  // outputs per thread: rows r0 .. r0 + 3 of one column

struct MetricArgs {
    const float* a; const float* b;     // the two images
    long long sa[4], sb[4];             // element strides: batch, channel, row, column
    int C, H, W;
    int pad;                            // zero padding on each side (window / 2 or 0)
    int Ho, Wo;                         // map size: H + 2 pad - window + 1, W likewise
    double w2[MW][MW];                  // the 2-D window: f32 outer product of the f32 taps, as doubles
    float* map;                         // [B][C][Ho][Wo] or NULL
    double* part;                       // [B][C][tiles_y][tiles_x][2]
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// WIN: the window's taps (odd, 1..11), a template argument so that the tap loops unroll without guards
template <int WIN>
__global__ __launch_bounds__(MTHREADS) void k_image_metrics(MetricArgs p) {
    __shared__ float sx[MS][MS], sy[MS][MS];
    __shared__ double red[2][MTHREADS / kWave];

    const int tid = threadIdx.x;
    const int bc = blockIdx.z, b = bc / p.C, ch = bc - b * p.C;
    const int y0 = blockIdx.y * MT, x0 = blockIdx.x * MT;
    constexpr int span = MT + WIN - 1;         // staged rows and columns in use

    // tile + halo: staged (r, c) is pixel (y0 - pad + r, x0 - pad + c), zero outside the image
    const float* pa = p.a + b * p.sa[0] + ch * p.sa[1];
    const float* pb = p.b + b * p.sb[0] + ch * p.sb[1];
    for (int i = tid; i < span * span; i += MTHREADS) {
        const int r = i / span, c = i - r * span;
        const int gy = y0 - p.pad + r, gx = x0 - p.pad + c;
        const bool in = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        sx[r][c] = in ? pa[gy * p.sa[2] + gx * p.sa[3]] : 0.f;
        sy[r][c] = in ? pb[gy * p.sb[2] + gx * p.sb[3]] : 0.f;
    }
    __syncthreads();

    // outputs (r0 + o, c), o < 4: window row i of output o is staged row r0 + o + i, so staged row
    // r0 + dr serves output o with window row dr - o.  Window column j outermost: its eleven
    // weights stay in scalar registers while the column of staged pixels goes by (w2 is symmetric,
    // so row j of it is read); every output sums j, then i, ascending.  A staged read has each
    // half-wave on 32 consecutive words of one row, and a 4-byte LDS read services the two halves
    // in separate cycles, so the four rows between them cost nothing
    const int c = tid % MT, r0 = (tid / MT) * MR;
    double m1[MR], m2[MR], e11[MR], e22[MR], e12[MR];
#pragma unroll
    for (int o = 0; o < MR; ++o) m1[o] = m2[o] = e11[o] = e22[o] = e12[o] = 0.;
#pragma unroll 1
    for (int j = 0; j < WIN; ++j) {                                // c + j <= span - 1
        double wj[WIN];
#pragma unroll
        for (int i = 0; i < WIN; ++i) wj[i] = p.w2[j][i];
#pragma unroll
        for (int dr = 0; dr < WIN + MR - 1; ++dr) {                // r0 + dr <= MT - MR + WIN + MR - 2 = span - 1
            const double xv = (double)sx[r0 + dr][c + j], yv = (double)sy[r0 + dr][c + j];
            const double xx = xv * xv, yy = yv * yv, xy = xv * yv;
#pragma unroll
            for (int o = 0; o < MR; ++o) {
                const int i = dr - o;                              // a constant once unrolled
                if (i >= 0 && i < WIN) {
                    const double w = wj[i];
                    m1[o] += w * xv;
                    m2[o] += w * yv;
                    e11[o] += w * xx;
                    e22[o] += w * yy;
                    e12[o] += w * xy;
                }
            }
        }
    }

    // the map (pytorch_ssim/__init__.py:30-41) and this tile's share of the MSE
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double sq = 0., ss = 0.;
#pragma unroll
    for (int o = 0; o < MR; ++o) {
        const int r = r0 + o, oy = y0 + r, ox = x0 + c;
        if (oy < p.H && ox < p.W) {            // the pixel itself sits at staged (r + pad, c + pad)
            const double d = (double)sx[r + p.pad][c + p.pad] - (double)sy[r + p.pad][c + p.pad];
            sq += d * d;
        }
        if (oy < p.Ho && ox < p.Wo) {
#pragma clang fp contract(off)
            const double m11 = m1[o] * m1[o], m22 = m2[o] * m2[o], m12 = m1[o] * m2[o];
            const double s11 = e11[o] - m11, s22 = e22[o] - m22, s12 = e12[o] - m12;
            const double v = ((2. * m12 + C1) * (2. * s12 + C2)) / ((m11 + m22 + C1) * (s11 + s22 + C2));
            ss += v;
            if (p.map) p.map[((size_t)bc * p.Ho + oy) * p.Wo + ox] = (float)v;
        }
    }

    // wavefront, then the four wavefronts in order
    sq = wave_sum_f64(sq);
    ss = wave_sum_f64(ss);
    if (lane_id() == 0) {
        red[0][tid / kWave] = sq;
        red[1][tid / kWave] = ss;
    }
    __syncthreads();
    if (tid == 0) {
        double* o = p.part + 2 * (((size_t)bc * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
        o[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        o[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// out[b] = (mse, ssim) of image b: its n partial pairs, lane l taking l, l + 64, ... in order
__global__ __launch_bounds__(kWave) void k_image_metrics_final(const double* __restrict__ part, int n, double n_pix,
                                                              double n_map, float* __restrict__ out) {
    const double* q = part + 2 * (size_t)blockIdx.x * n;
    double sq = 0., ss = 0.;
    for (int i = threadIdx.x; i < n; i += kWave) {
        sq += q[2 * i];
        ss += q[2 * i + 1];
    }
    sq = wave_sum_f64(sq);
    ss = wave_sum_f64(ss);
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = (float)(sq / n_pix);
        out[2 * blockIdx.x + 1] = (float)(ss / n_map);
    }
}

static inline int metric_tiles(int n) { return (n + MT - 1) / MT; }

// ---- depth metrics (model/eval_images.py:105-107, 152-160, 200-201 and model/common.py:676-694 of the
// reference): the rendered depth is resampled to the ground truth's grid by pixel-centre nearest
// neighbour and scaled inside the kernel, both range masks, the four confusion counts and the seven
// error sums over the pixels in range in both come from one pass.
//   k_depth_metrics       : one workgroup per (DPIX consecutive pixels of the gt grid, image); thread t
//                           takes pixels t, t + 256, ... of the block's span, so a wavefront reads 64
//                           consecutive gt pixels.  Eleven doubles per block go to the workspace;
//   k_depth_metrics_final : one wavefront per image sums them in a fixed order and finishes the means.
// The selection is made on the f32 values exactly as numpy makes it; everything after is fp64 (the
// counts too: integers below 2^31 sum exactly).  No atomics.
constexpr int DTHREADS = 256;
constexpr int DPPT = 4;                 // pixels per thread
constexpr int DPIX = DTHREADS * DPPT;   // pixels per workgroup
constexpr int DN = 11;                  // four error sums, three indicator counts, tp, fn, fp, tn

struct DepthArgs {
    const float* pred; const float* gt;
    long long sp[3], sg[3];             // element strides: batch, row, column
    int h, w, H, W;
    float sc, lo, hi;
    double* part;                       // [B][blocks][DN]
    float* depth;                       // [B][H][W] or NULL
    unsigned char* mask;                // [B][H][W] or NULL
};

__global__ __launch_bounds__(DTHREADS) void k_depth_metrics(DepthArgs p) {
    __shared__ double red[DN][DTHREADS / kWave];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long n_pix = (long long)p.H * p.W;        // < 2^31 (checked by the entry)
    const float* pp = p.pred + b * p.sp[0];
    const float* pg = p.gt + b * p.sg[0];

    double v[DN];
#pragma unroll
    for (int k = 0; k < DN; ++k) v[k] = 0.;
#pragma unroll
    for (int k = 0; k < DPPT; ++k) {
        const long long i = (long long)blockIdx.x * DPIX + k * DTHREADS + tid;
        if (i >= n_pix) continue;
        const int Y = (int)(i / p.W), X = (int)(i - (long long)Y * p.W);
        // pixel-centre nearest neighbour (cv2.INTER_NEAREST_EXACT): (2 Y + 1) h < 2^63
        const long long iy = min(((2LL * Y + 1) * p.h) / (2LL * p.H), (long long)p.h - 1);
        const long long ix = min(((2LL * X + 1) * p.w) / (2LL * p.W), (long long)p.w - 1);
        const float d = pp[iy * p.sp[1] + ix * p.sp[2]] * p.sc;           // one f32 multiply (depth_out *= sc)
        const float g = pg[Y * p.sg[1] + X * p.sg[2]];
        const bool mr = d >= p.lo && d <= p.hi, mg = g >= p.lo && g <= p.hi;   // NaN, inf, 0, negatives: false
        if (p.depth) p.depth[(size_t)b * n_pix + i] = d;
        if (p.mask) p.mask[(size_t)b * n_pix + i] = (unsigned char)((mr ? 1 : 0) | (mg ? 2 : 0));
        if (mr && mg) {
            const double gd = (double)g, dd = (double)d, diff = gd - dd, sq = diff * diff;
            const double lg = log(gd) - log(dd);
            const double r = fmax(gd / dd, dd / gd);
            v[0] += fabs(diff) / gd;
            v[1] += sq / gd;
            v[2] += sq;
            v[3] += lg * lg;
            v[4] += r < 1.25 ? 1. : 0.;
            v[5] += r < 1.5625 ? 1. : 0.;
            v[6] += r < 1.953125 ? 1. : 0.;
            v[7] += 1.;
        } else if (mg) {
            v[8] += 1.;                 // fn: gt in range, rendered not
        } else if (mr) {
            v[9] += 1.;                 // fp
        } else {
            v[10] += 1.;                // tn
        }
    }

    // wavefront, then the four wavefronts in order
#pragma unroll
    for (int k = 0; k < DN; ++k) {
        v[k] = wave_sum_f64(v[k]);
        if (lane_id() == 0) red[k][tid / kWave] = v[k];
    }
    __syncthreads();
    if (tid < DN)
        p.part[((size_t)b * gridDim.x + blockIdx.x) * DN + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// out[b] = {abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, tp, fn, fp, tn} of image b: its n partials, lane l
// taking l, l + 64, ... in order; tp == 0 leaves the seven errors 0 / 0 = NaN, as numpy's mean of nothing is
__global__ __launch_bounds__(kWave) void k_depth_metrics_final(const double* __restrict__ part, int n,
                                                              double* __restrict__ out) {
    const double* q = part + (size_t)blockIdx.x * n * DN;
    double v[DN];
#pragma unroll
    for (int k = 0; k < DN; ++k) v[k] = 0.;
    for (int i = threadIdx.x; i < n; i += kWave) {
#pragma unroll
        for (int k = 0; k < DN; ++k) v[k] += q[(size_t)i * DN + k];
    }
#pragma unroll
    for (int k = 0; k < DN; ++k) v[k] = wave_sum_f64(v[k]);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)blockIdx.x * DN;
        const double tp = v[7];
        o[0] = v[0] / tp;
        o[1] = v[1] / tp;
        o[2] = sqrt(v[2] / tp);
        o[3] = sqrt(v[3] / tp);
        o[4] = v[4] / tp;
        o[5] = v[5] / tp;
        o[6] = v[6] / tp;
        o[7] = tp;
        o[8] = v[8];
        o[9] = v[9];
        o[10] = v[10];
    }
}

static inline long long depth_blocks(int H, int W) { return ((long long)H * W + DPIX - 1) / DPIX; }

}  // namespace nerf

using namespace nerf;

extern "C" size_t nerf_image_metrics_workspace_bytes(int batch, int channels, int height, int width) {
    if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)batch * channels * metric_tiles(height) * metric_tiles(width) * 2 * sizeof(double);
}

extern "C" int nerf_image_metrics(const float* img1, int64_t s1_batch, int64_t s1_channel, int64_t s1_row,
                                  int64_t s1_col, const float* img2, int64_t s2_batch, int64_t s2_channel,
                                  int64_t s2_row, int64_t s2_col, int batch, int channels, int height, int width,
                                  int window, int use_padding, float* out, float* ssim_map, void* workspace,
                                  void* stream) {
    NERF_CHECK_PTR(img1); NERF_CHECK_PTR(img2); NERF_CHECK_PTR(out);
    NERF_CHECK(window >= 1 && window <= MW && (window & 1), "%s: window=%d must be odd, 1..%d", __func__, window, MW);
    NERF_CHECK(batch > 0, "%s: batch=%d", __func__, batch);
    NERF_CHECK(channels > 0, "%s: channels=%d", __func__, channels);
    NERF_CHECK(height > 0, "%s: height=%d", __func__, height);
    NERF_CHECK(width > 0, "%s: width=%d", __func__, width);
    NERF_CHECK((long long)batch * channels <= 65535, "%s: batch * channels = %lld exceeds the grid's 65535", __func__,
               (long long)batch * channels);
    NERF_CHECK(height <= 65535 * MT, "%s: height=%d exceeds the grid's 65535 tiles", __func__, height);
    NERF_CHECK(use_padding || (height >= window && width >= window),
               "%s: use_padding=0 needs height=%d and width=%d >= window=%d", __func__, height, width, window);
    NERF_CHECK(workspace != nullptr, "%s: null pointer 'workspace' (nerf_image_metrics_workspace_bytes)", __func__);
    NERF_CHECK((((uintptr_t)workspace) & 7u) == 0, "%s: pointer 'workspace' not 8-byte aligned", __func__);

    MetricArgs p;
    p.a = img1; p.b = img2;
    p.sa[0] = s1_batch; p.sa[1] = s1_channel; p.sa[2] = s1_row; p.sa[3] = s1_col;
    p.sb[0] = s2_batch; p.sb[1] = s2_channel; p.sb[2] = s2_row; p.sb[3] = s2_col;
    p.C = channels; p.H = height; p.W = width;
    p.pad = use_padding ? window / 2 : 0;
    p.Ho = height + 2 * p.pad - window + 1;
    p.Wo = width + 2 * p.pad - window + 1;
    // create_window(window, .) of pytorch_ssim/__init__.py:8-17: f32 taps over their sum (the sum
    // rounded to f32 once, as torch's reduction of these few values gives it), then their f32
    // outer product
    float e[MW], g[MW];
    double sum = 0.;
    for (int k = 0; k < window; ++k) {
        const double d = (double)(k - window / 2);
        e[k] = (float)std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += (double)e[k];
    }
    for (int k = 0; k < MW; ++k) g[k] = k < window ? e[k] / (float)sum : 0.f;
    for (int i = 0; i < MW; ++i)
        for (int j = 0; j < MW; ++j) p.w2[i][j] = (double)(float)(g[i] * g[j]);
    p.map = ssim_map;
    p.part = static_cast<double*>(workspace);

    const int ty = metric_tiles(height), tx = metric_tiles(width);
    hipStream_t s = as_stream(stream);
    const dim3 grid(tx, ty, batch * channels);
    switch (window) {
        case 1: hipLaunchKernelGGL(k_image_metrics<1>, grid, dim3(MTHREADS), 0, s, p); break;
        case 3: hipLaunchKernelGGL(k_image_metrics<3>, grid, dim3(MTHREADS), 0, s, p); break;
        case 5: hipLaunchKernelGGL(k_image_metrics<5>, grid, dim3(MTHREADS), 0, s, p); break;
        case 7: hipLaunchKernelGGL(k_image_metrics<7>, grid, dim3(MTHREADS), 0, s, p); break;
        case 9: hipLaunchKernelGGL(k_image_metrics<9>, grid, dim3(MTHREADS), 0, s, p); break;
        default: hipLaunchKernelGGL(k_image_metrics<11>, grid, dim3(MTHREADS), 0, s, p); break;
    }
    hipLaunchKernelGGL(k_image_metrics_final, dim3(batch), dim3(kWave), 0, s, (const double*)p.part, channels * ty * tx,
                       (double)channels * height * width, (double)channels * p.Ho * p.Wo, out);
    return check_launch(__func__);
}

extern "C" size_t nerf_depth_metrics_workspace_bytes(int batch, int gt_height, int gt_width) {
    if (batch <= 0 || gt_height <= 0 || gt_width <= 0) return 0;
    return (size_t)batch * (size_t)depth_blocks(gt_height, gt_width) * DN * sizeof(double);
}

extern "C" int nerf_depth_metrics(const float* pred, int64_t sp_batch, int64_t sp_row, int64_t sp_col, int h, int w,
                                  const float* gt, int64_t sg_batch, int64_t sg_row, int64_t sg_col, int H, int W,
                                  int batch, float sc, float min_depth, float max_depth, double* out, float* depth_out,
                                  uint8_t* mask_out, void* workspace, void* stream) {
    NERF_CHECK_PTR(pred); NERF_CHECK_PTR(gt); NERF_CHECK_PTR(out);
    NERF_CHECK(workspace != nullptr, "%s: null pointer 'workspace' (nerf_depth_metrics_workspace_bytes)", __func__);
    NERF_CHECK((((uintptr_t)workspace) & 7u) == 0, "%s: pointer 'workspace' not 8-byte aligned", __func__);
    NERF_CHECK((((uintptr_t)out) & 7u) == 0, "%s: pointer 'out' not 8-byte aligned", __func__);
    NERF_CHECK(h > 0, "%s: h=%d", __func__, h);
    NERF_CHECK(w > 0, "%s: w=%d", __func__, w);
    NERF_CHECK(H > 0, "%s: H=%d", __func__, H);
    NERF_CHECK(W > 0, "%s: W=%d", __func__, W);
    NERF_CHECK(batch > 0, "%s: batch=%d", __func__, batch);
    NERF_CHECK(batch <= 65535, "%s: batch=%d exceeds the grid's 65535", __func__, batch);
    NERF_CHECK((long long)H * W < (1LL << 31), "%s: H * W = %lld must be below 2^31", __func__, (long long)H * W);
    NERF_CHECK(std::isfinite(sc), "%s: sc=%g must be finite", __func__, (double)sc);
    // log and the ratios are undefined at 0: the reference never checks, this entry says so
    NERF_CHECK(min_depth > 0.f, "%s: min_depth=%g must be positive", __func__, (double)min_depth);
    NERF_CHECK(max_depth >= min_depth, "%s: max_depth=%g must be at least min_depth=%g", __func__, (double)max_depth,
               (double)min_depth);

    DepthArgs p;
    p.pred = pred; p.gt = gt;
    p.sp[0] = sp_batch; p.sp[1] = sp_row; p.sp[2] = sp_col;
    p.sg[0] = sg_batch; p.sg[1] = sg_row; p.sg[2] = sg_col;
    p.h = h; p.w = w; p.H = H; p.W = W;
    p.sc = sc; p.lo = min_depth; p.hi = max_depth;
    p.part = static_cast<double*>(workspace);
    p.depth = depth_out;
    p.mask = mask_out;

    const int blocks = (int)depth_blocks(H, W);          // < 2^21
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_depth_metrics, dim3(blocks, batch), dim3(DTHREADS), 0, s, p);
    hipLaunchKernelGGL(k_depth_metrics_final, dim3(batch), dim3(kWave), 0, s, (const double*)p.part, blocks, out);
    return check_launch(__func__);
}
