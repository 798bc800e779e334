// The head of a training step in one launch (nerf_step_head): the ray set-up of rays.hip's
// seven launches in block 0, the weight pack of k_pack in the other blocks.  The two read
// nothing the other writes, so the blocks never wait for one another; the launch lasts as long
// as its slower part.  Every stage is the device function the separate kernel calls
// (rays_dev.hpp, pack_dev.hpp, mat4.hpp) and hands its values on through registers or LDS
// behind a __syncthreads(), so the results are those of the separate entries bit for bit.
#include "common.hpp"
#include "mat4.hpp"
#include "pack_dev.hpp"
#include "rays_dev.hpp"

#include <cmath>

namespace nerf {

// 512 threads: the pack code needs ~180 VGPRs (two waves per SIMD, as in k_pack), which a
// 1024-thread block cannot have; the draw does not depend on the slot-to-thread mapping.
// (256 threads, k_pack's own block, was measured: the ray block alone 19.6 us against 15.9 us
// and the whole launch 24.9 us against 20.1 us back to back, profiles/r07/step_head_parts.txt.)
// Pack blocks per descriptor: k_pack's 128 + 128 blocks of 256 threads as blocks of SH_THREADS
constexpr int SH_THREADS = 512, SH_PER_THREAD = NERF_SAMPLE_MAX_RAYS / SH_THREADS;
constexpr int SH_F32 = 128 * 256 / SH_THREADS, SH_H = 128 * 256 / SH_THREADS;

struct StepHeadArgs {
    nerf_step_head_rays rays;
    int has_rays;
    int log_table;     // the hash set: 2^log_table slots of table and of owner (dynamic LDS)
    int pack_blocks;   // blocks per descriptor: SH_F32 (+ SH_H with fp16 pair images)
};

// VALID: the draw repeats until a drawn pixel has a valid depth (rays_dev.hpp sample_draw_valid);
// the instantiation without it is the kernel as it was.
template <bool VALID>
__device__ __forceinline__ void ray_block(const nerf_step_head_rays& a, uint32_t* table, uint32_t* owner,
                                          int log_table, const uint8_t* __restrict__ valid,
                                          int* __restrict__ attempts) {
    __shared__ float Ms[16];
    const int tid = threadIdx.x;
    const int R = a.n_rays;
    if (tid == 0) {   // the 4x4 chain: one thread, as in the separate kernels
        float c2w[16], world[16], k[16], sc[16], m[16], ki[16], wi[16], si[16];
        load4(a.K, k);        // every input first: their misses overlap (the stores below would
        load4(a.scale, sc);   // otherwise keep these loads behind the pose arithmetic)
        if (a.r != nullptr) pose_c2w_eval(a.r, a.t, a.init_c2w, c2w);
        else load4(a.c2w_in, c2w);
        store4(a.c2w, c2w);
        inverse4(c2w, world);
        store4(a.world, world);
        unproject_eval(k, world, sc, m, ki, wi, si);
        store4(a.M, m);
        store4(a.inverses, ki);
        store4(a.inverses + 16, wi);
        store4(a.inverses + 32, si);
#pragma unroll
        for (int i = 0; i < 16; ++i) Ms[i] = m[i];
    }
    // device step counter: read by all threads, advanced once at the end (k_sample_rays' rule)
    unsigned long long* ctr = reinterpret_cast<unsigned long long*>(a.seed_counter);
    const unsigned long long c = ctr ? *ctr : 0ull;
    uint32_t val[SH_PER_THREAD];
    bool pend[SH_PER_THREAD];
    int st;
    if constexpr (VALID) {
        int att;
        st = sample_draw_valid<SH_THREADS>(a.n_pix, R, a.seed, ctr != nullptr, c, valid, table, owner, log_table,
                                           val, pend, att);
        if (tid == 0 && attempts != nullptr) *attempts = att;
    } else {
        uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        if (ctr) key = sample_key_mix(key, c);
        st = sample_draw<SH_THREADS>(a.n_pix, R, key, table, owner, log_table, val, pend);   // syncs: Ms is visible
    }
    if (tid == 0 && a.status != nullptr) *a.status = st;
    float M[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) M[i] = Ms[i];
    const bool has_depth = a.depth_map != nullptr;
    const bool affine = has_depth && a.aff_scale != nullptr;
    const float sc = affine ? a.aff_scale[0] : 1.f, sh = affine ? a.aff_shift[0] : 0.f;
#pragma unroll
    for (int q = 0; q < SH_PER_THREAD; ++q) {
        const int j = tid + q * SH_THREADS;
        if (j >= R) continue;
        const uint32_t v = pend[q] ? 0u : val[q];
        float px, py;
        sample_gather(j, v, a.width, a.height, a.img, a.idx, a.pixels, a.rgb, px, py);
        float d = 0.f;
        if (has_depth) {    // network.py:24-26: the prior at the ray
            d = a.depth_map[v];
            a.depth_g[j] = d;
            if (affine) {
                d = depth_affine_eval(d, sc, sh, a.shift_first, a.lo);
                a.depth_d[j] = d;
            }
        }
        camera_ray_eval(M, px, py, has_depth, d, j, a.flags, a.cam, a.ray, a.view, a.ray_norm, a.d_src, a.mask);
    }
    if (ctr != nullptr) {
        __syncthreads();
        if (tid == 0) *ctr = c + 1;
    }
}

template <bool VALID>
__device__ __forceinline__ void step_head_body(const StepHeadArgs& a, const PackBatch& pb, const uint8_t* valid,
                                               int* attempts) {
    extern __shared__ uint32_t sh_table[];
    int b = blockIdx.x;
    if (a.has_rays) {
        if (b == 0) {
            ray_block<VALID>(a.rays, sh_table, sh_table + (1 << a.log_table), a.log_table, valid, attempts);
            return;
        }
        --b;
    }
    const nerf_pack_desc& d = pb.d[b / a.pack_blocks];
    const int bx = b % a.pack_blocks;
    if (bx < SH_F32) pack_f32(pb, d, bx, SH_F32);
    else pack_h(d, bx - SH_F32, SH_H);
}

__global__ __launch_bounds__(SH_THREADS) void k_step_head(StepHeadArgs a, PackBatch pb) {
    step_head_body<false>(a, pb, nullptr, nullptr);
}

__global__ __launch_bounds__(SH_THREADS) void k_step_head_valid(StepHeadArgs a, PackBatch pb,
                                                                const uint8_t* __restrict__ valid,
                                                                int* __restrict__ attempts) {
    step_head_body<true>(a, pb, valid, attempts);
}

}  // namespace nerf

using namespace nerf;

static int step_head_launch(const char* fn, const nerf_step_head_rays* rays, const uint8_t* valid,
                            int* attempts, bool with_valid, const nerf_pack_desc* descs, int n_desc, void* stream) {
    NERF_CHECK(rays != nullptr || n_desc > 0, "%s: neither a ray block nor pack descriptors", fn);
    NERF_CHECK(n_desc >= 0 && n_desc <= NERF_MAX_PACK, "%s: n_desc=%d outside 0..%d", fn, n_desc,
               NERF_MAX_PACK);
    NERF_CHECK(n_desc == 0 || descs != nullptr, "%s: null pointer 'descs'", fn);
    StepHeadArgs a{};
    size_t lds = 0;
    if (rays != nullptr) {
        const nerf_step_head_rays& r = *rays;
        NERF_CHECK(r.n_rays > 0 && r.n_rays <= NERF_SAMPLE_MAX_RAYS, "%s: n_rays=%d outside 1..%d", fn,
                   r.n_rays, NERF_SAMPLE_MAX_RAYS);
        NERF_CHECK(r.n_pix >= 2 * r.n_rays, "%s: n_pix=%d < 2*n_rays=%d (draw a permutation instead)", fn,
                   r.n_pix, 2 * r.n_rays);
        NERF_CHECK(r.width > 1 && r.height > 1 && r.width * r.height == r.n_pix,
                   "%s: width, height > 1 with width*height == n_pix", fn);
        NERF_CHECK((r.r != nullptr && r.t != nullptr) || (r.r == nullptr && r.c2w_in != nullptr),
                   "%s: the pose is (r, t) or c2w_in", fn);
        NERF_CHECK(r.K != nullptr && r.scale != nullptr && r.img != nullptr, "%s: null pointer among K, scale, img",
                   fn);
        NERF_CHECK(r.aff_scale == nullptr || (r.aff_shift != nullptr && r.depth_map != nullptr),
                   "%s: aff_scale needs aff_shift and depth_map", fn);
#define SH_OUT(p) NERF_CHECK(r.p != nullptr, "%s: null output '%s'", fn, #p)
        SH_OUT(c2w); SH_OUT(world); SH_OUT(M); SH_OUT(inverses); SH_OUT(idx); SH_OUT(pixels); SH_OUT(rgb);
        SH_OUT(cam); SH_OUT(ray); SH_OUT(ray_norm); SH_OUT(d_src);
        if (r.depth_map != nullptr) SH_OUT(depth_g);
        if (r.aff_scale != nullptr) SH_OUT(depth_d);
#undef SH_OUT
        a.rays = r;
        a.has_rays = 1;
        int lt = 2;
        while ((1 << lt) < 4 * r.n_rays) ++lt;
        a.log_table = lt;
        lds = 2 * sizeof(uint32_t) << lt;
    }
    PackBatch pb{};
    bool images = false;
    if (n_desc > 0)
        if (const int rc = pack_batch_fill(fn, descs, n_desc, pb, images)) return rc;
    a.pack_blocks = SH_F32 + ((pb.f16 && images) ? SH_H : 0);
    const unsigned grid = (unsigned)(a.has_rays + n_desc * a.pack_blocks);
    if (with_valid) {
        if (lds > 64 * 1024) {   // the largest tables (n_rays > 2048) need the per-kernel opt-in
            static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(k_step_head_valid),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                                               128 * 1024);
            (void)once;
        }
        hipLaunchKernelGGL(k_step_head_valid, dim3(grid), dim3(SH_THREADS), lds, as_stream(stream), a, pb, valid,
                           attempts);
        return check_launch(fn);
    }
    if (lds > 64 * 1024) {
        static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(k_step_head),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        (void)once;
    }
    hipLaunchKernelGGL(k_step_head, dim3(grid), dim3(SH_THREADS), lds, as_stream(stream), a, pb);
    return check_launch(fn);
}

extern "C" int nerf_step_head(const nerf_step_head_rays* rays, const nerf_pack_desc* descs, int n_desc,
                              void* stream) {
    return step_head_launch(__func__, rays, nullptr, nullptr, false, descs, n_desc, stream);
}

// The step head with the draw repeated until a drawn pixel has a valid depth.  valid == NULL and
// attempts == NULL: nerf_step_head's own kernel.
extern "C" int nerf_step_head_valid(const nerf_step_head_rays* rays, const uint8_t* valid, int* attempts,
                                    const nerf_pack_desc* descs, int n_desc, void* stream) {
    NERF_CHECK((valid == nullptr && attempts == nullptr) || rays != nullptr, "%s: valid / attempts without rays",
               __func__);
    return step_head_launch(__func__, rays, valid, attempts, valid != nullptr || attempts != nullptr, descs, n_desc,
                            stream);
}
