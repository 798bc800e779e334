// Weight packing shared by k_pack (misc.hip) and the step head's pack blocks (step_head.hip):
// the descriptor batch, its host-side checks and the per-block device functions.
#pragma once
#include "common.hpp"

#include <cmath>

namespace nerf {

struct PackBatch {
    nerf_pack_desc d[NERF_MAX_PACK];
    int n;
    int f16;   // GEMM precision mode 2: images in the fp16 pair form (pack_h), not bf16x3
};

// x -> three bf16 words (RNE each) with x = hi + mid + lo (same split as gemm_x6.hip)
__device__ __forceinline__ void split3(float x, uint16_t& h, uint16_t& m, uint16_t& l) {
    const __bf16 bh = (__bf16)x;
    const float r = x - (float)bh;
    const __bf16 bm = (__bf16)r;
    const __bf16 bl = (__bf16)(r - (float)bm);
    h = __builtin_bit_cast(uint16_t, bh);
    m = __builtin_bit_cast(uint16_t, bm);
    l = __builtin_bit_cast(uint16_t, bl);
}

// element (r, c) of a [N][K] operand into its bf16x3 image [3][K/8][N][8]
__device__ __forceinline__ void put_split(uint16_t* img, int N, int K, int r, int c, float x) {
    uint16_t h, m, l;
    split3(x, h, m, l);
    const size_t plane = (size_t)K * N;
    const size_t o = ((size_t)(c >> 3) * N + r) * 8 + (c & 7);
    img[o] = h;
    img[o + plane] = m;
    img[o + 2 * plane] = l;
}

// descriptor d; block bx of nb grid-strides over the padded destination
__device__ __forceinline__ void pack_f32(const PackBatch& pb, const nerf_pack_desc& d, int bx, int nb) {
#pragma clang fp contract(off)
    const int rows_s = d.rows_s > d.rows ? d.rows_s : d.rows;
    const int total = (d.dst_s != nullptr ? rows_s : d.rows) * d.ld_dst;
    const int gs = nb * blockDim.x;
    for (int e = bx * blockDim.x + threadIdx.x; e < total; e += gs) {
        const int r = e / d.ld_dst, c = e % d.ld_dst;
        const float x = (c < d.cols && r < d.rows) ? d.src[(size_t)r * d.cols + c] : 0.f;
        if (r < d.rows) d.dst[e] = x;
        if (d.dst_s != nullptr && !pb.f16) put_split(d.dst_s, rows_s, d.ld_dst, r, c, x);
    }
    if (d.dst_t != nullptr) {
        const int tt = d.rows_t * d.rows;  // dst_t[c][r], c < rows_t, r < rows
        for (int e = bx * blockDim.x + threadIdx.x; e < tt; e += gs) {
            const int c = e / d.rows, r = e % d.rows;
            d.dst_t[(size_t)c * d.ld_t + r] = c < d.cols ? d.src[(size_t)r * d.cols + c] : 0.f;
        }
    }
    if (d.dst_ts != nullptr && !pb.f16) {
        const int tt = d.rows_t * d.ld_t;  // whole image of dst_t, zero past the source
        for (int e = bx * blockDim.x + threadIdx.x; e < tt; e += gs) {
            const int c = e / d.ld_t, r = e % d.ld_t;   // dst_t row c, column r
            const float x = (c < d.cols && r < d.rows) ? d.src[(size_t)r * d.cols + c] : 0.f;
            put_split(d.dst_ts, d.rows_t, d.ld_t, c, r, x);
        }
    }
}

// Row r of the fp16 pair image of a [N][K] operand (x(c) = element (r, c)): one wave per
// row; the row max sets the scale 2^e, planes 0 / 1 get hi / lo of x 2^e (RNE fp16 each),
// e goes into the first word of the row's plane-2 chunk 0 (gemm_x6.hip, mode 2).  The row
// stays in registers between the max and the split (all its loads in flight at once: one
// memory latency per row, not one per 64 elements and pass).
constexpr int PACK_H_MAXK = 16 * kWave;
// chain images (cexp = true) also get the row exponents as one compact int array in plane 2's
// chunk 1 (unused otherwise): the chain kernels fetch a layer's 256 exponents with one 1 KB
// LDS-DMA instead of one 16-byte chunk per row
template <typename F>
__device__ __forceinline__ void put_row_h(uint16_t* img, int N, int K, int r, F&& x, bool cexp = false) {
    const int lane = lane_id();
    float v[PACK_H_MAXK / kWave];
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < PACK_H_MAXK / kWave; ++i) {
        const int c = lane + kWave * i;
        v[i] = c < K ? x(c) : 0.f;
        m = fmaxf(m, fabsf(v[i]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    const int e = row_exp(m);
    const size_t plane = (size_t)K * N;
#pragma unroll
    for (int i = 0; i < PACK_H_MAXK / kWave; ++i) {
        const int c = lane + kWave * i;
        if (c >= K) break;
        const float y = __builtin_amdgcn_ldexpf(v[i], e);
        const _Float16 h = (_Float16)y;
        const _Float16 l = (_Float16)(y - (float)h);
        const size_t o = ((size_t)(c >> 3) * N + r) * 8 + (c & 7);
        img[o] = __builtin_bit_cast(uint16_t, h);
        img[o + plane] = __builtin_bit_cast(uint16_t, l);
    }
    if (lane == 0) *reinterpret_cast<int*>(img + 2 * plane + (size_t)r * 8) = e;
    if (cexp && lane == 0) reinterpret_cast<int*>(img + 2 * plane + (size_t)N * 8)[r] = e;
}

// fp16 pair images of the packed weights (GEMM precision mode 2): one wave per image row,
// rows of dst_s, dst_ts, then of the chain images dst_cs (the first perm_k columns in
// chain_perm order) and dst_cts (every column in chain order) (block bx of nb)
__device__ __forceinline__ void pack_h(const nerf_pack_desc& d, int bx, int nb) {
    const int rows_s = d.rows_s > d.rows ? d.rows_s : d.rows;
    const int ns = d.dst_s ? rows_s : 0, nt = d.dst_ts ? d.rows_t : 0;
    const int ncs = d.dst_cs ? rows_s : 0, nct = d.dst_cts ? d.rows_t : 0;
    const int wave = (bx * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (nb * blockDim.x) >> 6;
    auto w_at = [&](int r, int c) { return (c < d.cols && r < d.rows) ? d.src[(size_t)r * d.cols + c] : 0.f; };
    for (int w = wave; w < ns + nt + ncs + nct; w += nwaves) {
        if (w < ns) {
            const int r = w;
            put_row_h(d.dst_s, rows_s, d.ld_dst, r, [&](int c) { return w_at(r, c); });
        } else if (w < ns + nt) {
            const int c = w - ns;   // dst_t row = source column c, its columns = source rows
            put_row_h(d.dst_ts, d.rows_t, d.ld_t, c, [&](int r) { return w_at(r, c); });
        } else if (w < ns + nt + ncs) {
            const int r = w - ns - nt;
            put_row_h(d.dst_cs, rows_s, d.ld_dst, r, [&](int c) { return w_at(r, c < d.perm_k ? chain_perm(c) : c); },
                      true);
        } else {
            const int c = w - ns - nt - ncs;
            put_row_h(d.dst_cts, d.rows_t, d.ld_t, c, [&](int r) { return w_at(chain_perm(r), c); }, true);
        }
    }
}

// the checks of nerf_pack_weights on descs[0..n) and the kernel argument they fill; images: some
// descriptor has an image destination (the fp16 pair blocks are launched only then)
inline int pack_batch_fill(const char* fn, const nerf_pack_desc* descs, int n, PackBatch& pb, bool& images) {
    pb = PackBatch{};
    pb.n = n;
    pb.f16 = gemm_precision() == 2;
    for (int i = 0; i < n; ++i) {
        const nerf_pack_desc& d = descs[i];
        NERF_CHECK(d.src && d.dst && d.rows > 0 && d.cols > 0 && d.ld_dst >= d.cols,
                   "%s: bad descriptor %d", fn, i);
        NERF_CHECK(d.dst_t == nullptr || (d.rows_t >= d.cols && d.ld_t >= d.rows),
                   "%s: descriptor %d: rows_t < cols or ld_t < rows", fn, i);
        NERF_CHECK(d.dst_s == nullptr || d.ld_dst % 8 == 0, "%s: descriptor %d: split image needs ld_dst %% 8 == 0",
                   fn, i);
        NERF_CHECK(!pb.f16 || ((d.dst_s == nullptr || d.ld_dst <= PACK_H_MAXK) &&
                               (d.dst_ts == nullptr || d.ld_t <= PACK_H_MAXK)),
                   "%s: descriptor %d: fp16 pair image rows longer than %d", fn, i, PACK_H_MAXK);
        NERF_CHECK(d.dst_ts == nullptr || (d.rows_t >= d.cols && d.ld_t >= d.rows && d.ld_t % 8 == 0),
                   "%s: descriptor %d: transposed split image needs rows_t >= cols, ld_t >= rows, ld_t %% 8 == 0",
                   fn, i);
        // the compact exponent array sits at plane 2's chunk 1: an image of one chunk (K = 8) has none
        NERF_CHECK(d.dst_cs == nullptr || d.ld_dst >= 16, "%s: descriptor %d: the chain image needs ld_dst >= 16",
                   fn, i);
        NERF_CHECK(d.dst_cts == nullptr || d.ld_t >= 16, "%s: descriptor %d: the transposed chain image needs ld_t >= 16",
                   fn, i);
        NERF_CHECK((d.dst_cs == nullptr && d.dst_cts == nullptr) ||
                       (pb.f16 && d.perm_k >= 0 && d.perm_k % 32 == 0 && d.perm_k <= d.ld_dst && d.ld_dst % 8 == 0 &&
                        d.ld_dst <= PACK_H_MAXK),
                   "%s: descriptor %d: chain images need precision mode 2, perm_k %% 32 == 0 (<= ld_dst)", fn, i);
        NERF_CHECK(d.dst_cts == nullptr || (d.rows_t >= d.cols && d.ld_t >= d.rows && d.ld_t % 32 == 0 &&
                                            d.ld_t <= PACK_H_MAXK),
                   "%s: descriptor %d: the transposed chain image needs rows_t >= cols, ld_t >= rows, ld_t %% 32 == 0",
                   fn, i);
        pb.d[i] = d;
    }
    images = false;
    for (int i = 0; i < n; ++i)
        images = images || descs[i].dst_s != nullptr || descs[i].dst_ts != nullptr || descs[i].dst_cs != nullptr ||
                 descs[i].dst_cts != nullptr;
    return NERF_OK;
}

}  // namespace nerf
