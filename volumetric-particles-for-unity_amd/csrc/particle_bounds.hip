// particle_bounds.hip -- where the resident particles are and what the bin kept of them (include/vpfx.h "where the resident particles
// are"): the two queries a host needs once its particles never leave the GPU (emitter_device.hip).  Nothing here runs on the frame path.
//
//   k_bounds_init    the result words of one vp_particle_bounds call: min keys = key(+inf), max keys = key(-inf), the rest 0
//   k_bounds         ONE launch over d_ws[P] (world position + size as k_extract wrote them): per lane 13 running floats + 2 counters in a
//                    grid-stride loop of float4 loads, __shfl_xor across the wave, LDS across the four waves, one atomic per value per workgroup
//   k_cover_count    one thread per (particle, metavoxel) pair of the CSR lists the bin built: cover[ids[i]] += 1
//   k_cover_reduce   over cover[P]: particles in >= 1 list, finite particles in none, non-finite ones, the sum and the maximum
//
// Float min / max across workgroups are unsigned atomicMin / atomicMax on monotone keys: key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000)
// orders every float as an unsigned integer (-inf < ... < -0 < +0 < ... < +inf), so the reduction is exact and order-free and the result is
// defined to the bit (up to the sign of a zero).  The arithmetic is the frame transform of k_bin's light-space line (bin.hip), f32 without
// contraction; the skip rule is k_bin's as well.  The coverage repeats none of the bin's acceptance arithmetic: it counts list entries.
#include "vpfx_internal.h"

#include <cmath>
#include <cstring>

namespace {

// layout of the result words (d_query / h_query)
constexpr int QW_MIN = 0;          // [6] keys: center_min.xyz, sphere_min.xyz
constexpr int QW_MAX = 6;          // [6] keys: center_max.xyz, sphere_max.xyz
constexpr int QW_RADIUS = 12;      // bits of max_radius (>= 0: float bits order like unsigned integers)
constexpr int QW_COUNTED = 13, QW_SKIPPED = 14;
constexpr int QW_COVER = 16;       // coverage: covered, uncovered, skipped, max, pairs (64 bits, words 20..21)
constexpr int QUERY_WORDS = 24;

constexpr uint32_t KEY_POS_INF = 0x7F800000u ^ 0x80000000u;
constexpr uint32_t KEY_NEG_INF = 0xFF800000u ^ 0xFFFFFFFFu;

__host__ __device__ inline uint32_t key_of_bits(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
inline float float_of_key(uint32_t k)
{
    const uint32_t b = (k >> 31) ? (k ^ 0x80000000u) : ~k;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

struct FrameRows { float m[12]; };             // world_to_frame rows 0..2: m[r*4 + c]

__global__ void k_bounds_init(uint32_t* __restrict__ w)
{
    const int i = threadIdx.x;
    if (i < 16) w[i] = i < QW_MAX ? KEY_POS_INF : i < QW_RADIUS ? KEY_NEG_INF : 0u;
}

__device__ __forceinline__ bool particle_finite(const float4 w)
{
    // the rule k_bin skips by (bin.hip)
    return fabsf(w.x) < INFINITY && fabsf(w.y) < INFINITY && fabsf(w.z) < INFINITY && fabsf(w.w) < INFINITY;
}

__global__ void __launch_bounds__(256)
k_bounds(const float4* __restrict__ ws4, int P, FrameRows fr, uint32_t* __restrict__ out)
{
    __shared__ uint32_t sh[4][16];
    float lo[6], hi[6], rad = 0.f;             // 0..2 the centres, 3..5 the spheres
    int counted = 0, skipped = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    const unsigned stride = gridDim.x * 256u;     // at most 2^18 (grid_for): p + stride stays below 2^32
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < (unsigned)P; p += stride) {
        const float4 w = ws4[p];
        if (!particle_finite(w)) { ++skipped; continue; }
        ++counted;
        const float h = fabsf(w.w) * 0.5f;
        rad = fmaxf(rad, h);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float f = ((fr.m[r * 4] * w.x + fr.m[r * 4 + 1] * w.y) + fr.m[r * 4 + 2] * w.z) + fr.m[r * 4 + 3];
            lo[r] = fminf(lo[r], f); hi[r] = fmaxf(hi[r], f);
            lo[3 + r] = fminf(lo[3 + r], f - h); hi[3 + r] = fmaxf(hi[3 + r], f + h);
        }
    }
    // across the 64 lanes of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], d)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d)); }
        rad = fmaxf(rad, __shfl_xor(rad, d));
        counted += __shfl_xor(counted, d);
        skipped += __shfl_xor(skipped, d);
    }
    // across the four waves through LDS, then lanes 0..14 of wave 0 publish one value each
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { sh[wv][QW_MIN + k] = key_of_bits(__float_as_uint(lo[k])); sh[wv][QW_MAX + k] = key_of_bits(__float_as_uint(hi[k])); }
        sh[wv][QW_RADIUS] = __float_as_uint(rad);
        sh[wv][QW_COUNTED] = (uint32_t)counted;
        sh[wv][QW_SKIPPED] = (uint32_t)skipped;
    }
    __syncthreads();
    if (threadIdx.x < 15) {
        const int j = threadIdx.x;
        const uint32_t a = sh[0][j], b = sh[1][j], c = sh[2][j], d = sh[3][j];
        if (j < QW_MAX) atomicMin(&out[j], min(min(a, b), min(c, d)));
        else if (j <= QW_RADIUS) atomicMax(&out[j], max(max(a, b), max(c, d)));
        else atomicAdd(&out[j], a + b + c + d);
    }
}

__global__ void __launch_bounds__(256)
k_cover_count(const int* __restrict__ ids, int pairs, int P, int* __restrict__ cover)
{
    const unsigned stride = gridDim.x * 256u;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)pairs; i += stride) {
        const int p = ids[i];
        if ((unsigned)p < (unsigned)P) atomicAdd(&cover[p], 1);
    }
}

__global__ void __launch_bounds__(256)
k_cover_reduce(const int* __restrict__ cover, const float4* __restrict__ ws4, int P, uint32_t* __restrict__ out)
{
    __shared__ unsigned long long sh[4][5];
    int covered = 0, uncovered = 0, skipped = 0, mx = 0;
    unsigned long long sum = 0;
    const unsigned stride = gridDim.x * 256u;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < (unsigned)P; p += stride) {
        const int n = cover[p];
        if (n > 0) { ++covered; sum += (unsigned)n; mx = max(mx, n); }
        else if (particle_finite(ws4[p])) ++uncovered;
        else ++skipped;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        covered += __shfl_xor(covered, d);
        uncovered += __shfl_xor(uncovered, d);
        skipped += __shfl_xor(skipped, d);
        mx = max(mx, __shfl_xor(mx, d));
        sum += __shfl_xor(sum, d);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { sh[wv][0] = (unsigned)covered; sh[wv][1] = (unsigned)uncovered; sh[wv][2] = (unsigned)skipped; sh[wv][3] = (unsigned)mx; sh[wv][4] = sum; }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int j = threadIdx.x;
        const unsigned long long a = sh[0][j], b = sh[1][j], c = sh[2][j], d = sh[3][j];
        if (j < 3) atomicAdd(&out[QW_COVER + j], (uint32_t)(a + b + c + d));
        else if (j == 3) atomicMax(&out[QW_COVER + 3], (uint32_t)max(max(a, b), max(c, d)));
        else atomicAdd(reinterpret_cast<unsigned long long*>(out + QW_COVER + 4), a + b + c + d);
    }
}

// a few workgroups per CU at the most; every workgroup strides over the rest
inline unsigned grid_for(const vp_ctx* c, size_t n)
{
    const size_t want = (n + 255) / 256, cap = (size_t)(c->num_cus > 0 ? c->num_cus : 256) * 4;
    return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

int ensure_query_words(vp_ctx* c)
{
    if (c->d_query) return VP_OK;
    uint32_t* d = nullptr;
    uint32_t* h = nullptr;
    VP_HIP(hipMalloc((void**)&d, QUERY_WORDS * sizeof(uint32_t)));
    const hipError_t e = hipHostMalloc((void**)&h, QUERY_WORDS * sizeof(uint32_t), hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipFree(d); return vp_fail(c, e == hipErrorOutOfMemory ? VP_ERR_OOM : VP_ERR_HIP, "hipHostMalloc failed: %s", hipGetErrorString(e)); }
    c->d_query = d; c->h_query = h;
    return VP_OK;
}

}  // namespace

void particle_queries_free(vp_ctx* c)
{
    if (c->d_query) (void)hipFree(c->d_query);
    if (c->h_query) (void)hipHostFree(c->h_query);
    if (c->d_cover) (void)hipFree(c->d_cover);
    c->d_query = c->h_query = nullptr;
    c->d_cover = nullptr; c->cover_cap = 0;
}

VP_EXPORT int vp_particle_bounds(vp_ctx* c, const float world_to_frame[16], struct vp_particle_bounds* out)
{
    if (!c) return VP_ERR_BAD_ARG;
    if (c->multi) return vp_fail(c, VP_ERR_UNSUPPORTED, "vp_particle_bounds: not available on a fan-out (multi-GPU) context");
    if (!out) return vp_fail(c, VP_ERR_BAD_ARG, "vp_particle_bounds: null output");
    if (world_to_frame && !hl_is_rigid(world_to_frame))
        return vp_fail(c, VP_ERR_BAD_ARG, "vp_particle_bounds: world_to_frame is not a finite rigid transform (rows orthonormal within 1e-3, last row 0 0 0 1)");
    if (!c->have_particles) return vp_fail(c, VP_ERR_STATE, "vp_particle_bounds before vp_upload_particles");
    struct vp_particle_bounds r;
    std::memset(&r, 0, sizeof r);
    for (int k = 0; k < 3; ++k) { r.center_min[k] = r.sphere_min[k] = INFINITY; r.center_max[k] = r.sphere_max[k] = -INFINITY; }
    if (c->P > 0) {
        VP_HIP(hipSetDevice(c->device));
        int rc = ensure_query_words(c); if (rc) return rc;
        FrameRows fr;
        for (int row = 0; row < 3; ++row)
            for (int col = 0; col < 4; ++col) fr.m[row * 4 + col] = world_to_frame ? world_to_frame[col * 4 + row] : (row == col ? 1.f : 0.f);
        hipLaunchKernelGGL(k_bounds_init, dim3(1), dim3(64), 0, c->stream, c->d_query);
        hipLaunchKernelGGL(k_bounds, dim3(grid_for(c, (size_t)c->P)), dim3(256), 0, c->stream, (const float4*)c->d_ws, c->P, fr, c->d_query);
        VP_HIP(hipGetLastError());
        VP_HIP(hipMemcpyAsync(c->h_query, c->d_query, 16 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        rc = api_stream_sync(c); if (rc) return rc;
        const uint32_t* w = c->h_query;
        for (int k = 0; k < 3; ++k) {
            r.center_min[k] = float_of_key(w[QW_MIN + k]);     r.sphere_min[k] = float_of_key(w[QW_MIN + 3 + k]);
            r.center_max[k] = float_of_key(w[QW_MAX + k]);     r.sphere_max[k] = float_of_key(w[QW_MAX + 3 + k]);
        }
        std::memcpy(&r.max_radius, &w[QW_RADIUS], 4);
        r.counted = (int32_t)w[QW_COUNTED];
        r.skipped = (int32_t)w[QW_SKIPPED];
    }
    *out = r;
    return VP_OK;
}

VP_EXPORT int vp_particle_coverage(vp_ctx* c, struct vp_particle_coverage* out, int32_t* mv_per_particle_out)
{
    if (!c) return VP_ERR_BAD_ARG;
    if (c->multi) return vp_fail(c, VP_ERR_UNSUPPORTED, "vp_particle_coverage: not available on a fan-out (multi-GPU) context");
    if (!out) return vp_fail(c, VP_ERR_BAD_ARG, "vp_particle_coverage: null output");
    if (!c->binned) return vp_fail(c, VP_ERR_STATE, "vp_particle_coverage before vp_bin");
    struct vp_particle_coverage r;
    std::memset(&r, 0, sizeof r);
    r.particles = c->P;
    if (c->P > 0) {
        VP_HIP(hipSetDevice(c->device));
        int rc = ensure_query_words(c); if (rc) return rc;
        if ((size_t)c->P > c->cover_cap) {
            if (c->d_cover) VP_HIP(hipFree(c->d_cover));
            c->d_cover = nullptr; c->cover_cap = 0;
            const size_t cap = (size_t)c->P + (size_t)c->P / 4 + 64;
            VP_HIP(hipMalloc((void**)&c->d_cover, cap * sizeof(int)));
            c->cover_cap = cap;
        }
        const int pairs = c->h_meta.pairs;
        VP_HIP(hipMemsetAsync(c->d_cover, 0, (size_t)c->P * sizeof(int), c->stream));
        VP_HIP(hipMemsetAsync(c->d_query + QW_COVER, 0, 8 * sizeof(uint32_t), c->stream));
        if (pairs > 0)
            hipLaunchKernelGGL(k_cover_count, dim3(grid_for(c, (size_t)pairs)), dim3(256), 0, c->stream, (const int*)c->d_ids, pairs, c->P, c->d_cover);
        hipLaunchKernelGGL(k_cover_reduce, dim3(grid_for(c, (size_t)c->P)), dim3(256), 0, c->stream, (const int*)c->d_cover, (const float4*)c->d_ws, c->P,
                           c->d_query);
        VP_HIP(hipGetLastError());
        VP_HIP(hipMemcpyAsync(c->h_query + QW_COVER, c->d_query + QW_COVER, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (mv_per_particle_out)
            VP_HIP(hipMemcpyAsync(mv_per_particle_out, c->d_cover, (size_t)c->P * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        rc = api_stream_sync(c); if (rc) return rc;
        const uint32_t* w = c->h_query + QW_COVER;
        r.covered = (int32_t)w[0]; r.uncovered = (int32_t)w[1]; r.skipped = (int32_t)w[2];
        r.max_mv_per_particle = (int32_t)w[3];
        unsigned long long sum;
        std::memcpy(&sum, w + 4, 8);
        r.pairs = (int64_t)sum;
    }
    *out = r;
    return VP_OK;
}
