// volume_shadow.hip -- the shadow the particle volume casts on the opaque scene (include/vpfx.h "volume shadows"): the light-propagation
// map of the last fill projected onto world points or onto the pixels of the scene's eye depth.  The reference keeps that map for exactly
// this ("we can project the light propagation texture on to the scene ... and thus have shadows cast by the volume", FillVolume.shader:224-250;
// bound at RayMarchVoxel.shader:4,43 and VPR.cs:719) and never does it.  No brick is sampled; nothing here runs on the bin / fill / ray-march path.
//
//   k_shadow_points   one thread per world point [n][3] -> factor [n]
//   k_shadow_image    one thread per pixel: the pixel ray of k_scene_depth (occluders.hip) to the eye depth, then the same core; a wave is 64
//                     consecutive pixels of one row (coalesced depth read and factor write)
//   k_shadow_apply    scene.rgb *= factor on [H][W][4], alpha untouched
//
// Arithmetic: f32 in the order written, no contraction (the build's -ffp-contract=off), plain divisions, no transcendental on the device --
// tests/shadow_twin.py repeats it op by op in numpy float32 and the points form equals it to the bit.
#include "vpfx_internal.h"

#include <cmath>

namespace {

struct CamRows { float r[12]; };       // rows of cameraToWorld's upper 3 x 4

// Light arriving at the first lit surface of the light-map column that holds world point p (or leaving the grid there); 1 outside the
// grid's footprint, in front of its near face, and for a non-finite point (every comparison is written so that a NaN fails it).
__device__ __forceinline__ float shadow_factor(float px, float py, float pz, const GridConsts& g, const float* __restrict__ Lm, int filter)
{
    const float* L = g.Linv;
    const float lx = ((L[0] * px + L[1] * py) + L[2] * pz) + L[3];
    const float ly = ((L[4] * px + L[5] * py) + L[6] * pz) + L[7];
    const float lz = ((L[8] * px + L[9] * py) + L[10] * pz) + L[11];
    // metavoxel xx is centred at lsO.x - (Nx/2 - xx) s with the INTEGER N/2 of hl_build_grid; its unbordered cube spans +/- s/2
    const float gx = ((lx - g.lsO[0]) / g.s + (float)(g.Nx / 2)) + 0.5f;
    const float gy = ((ly - g.lsO[1]) / g.s + (float)(g.Ny / 2)) + 0.5f;
    const float gz = ((lz - g.lsO[2]) / g.s + (float)(g.Nz / 2)) + 0.5f;
    const bool inside = gx >= 0.f && gx < (float)g.Nx && gy >= 0.f && gy < (float)g.Ny && gz >= 0.f;
    if (!inside) return 1.0f;
    const int nv = g.nv, b = g.b;
    const int xx = (int)floorf(gx), yy = (int)floorf(gy);
    const float u = gx - (float)xx, v = gy - (float)yy;
    // the ray-march's texel rule (RmConsts.texScale / texBias) on the light map's tile of column (xx, yy)
    const float tx = (u * (float)(nv - 2 * b) + (float)b) - 0.5f;
    const float ty = (v * (float)(nv - 2 * b) + (float)b) - 0.5f;
    const size_t LW = (size_t)g.Nx * nv;
    const float* tile = Lm + (size_t)yy * nv * LW + (size_t)xx * nv;
    if (filter == VP_SHADOW_NEAREST) {
        const int ix = min(max((int)floorf(tx + 0.5f), 0), nv - 1);
        const int iy = min(max((int)floorf(ty + 0.5f), 0), nv - 1);
        return tile[(size_t)iy * LW + ix];
    }
    const int x0 = (int)floorf(tx), y0 = (int)floorf(ty);
    const float wx = tx - (float)x0, wy = ty - (float)y0;
    // clamped INSIDE the tile: its border texels are the neighbours' data, as the bricks are filtered (the clamp only acts when b = 0)
    const int xa = min(max(x0, 0), nv - 1), xb = min(max(x0 + 1, 0), nv - 1);
    const int ya = min(max(y0, 0), nv - 1), yb = min(max(y0 + 1, 0), nv - 1);
    const float L00 = tile[(size_t)ya * LW + xa], L10 = tile[(size_t)ya * LW + xb];
    const float L01 = tile[(size_t)yb * LW + xa], L11 = tile[(size_t)yb * LW + xb];
    const float a = L00 + wx * (L10 - L00);
    const float c = L01 + wx * (L11 - L01);
    return a + wy * (c - a);
}

// factor = 1 - strength (1 - f); strength 1 hands the map's value through unrounded (1 - (1 - f) loses the low bits of an f below 0.5)
__device__ __forceinline__ float shadow_strength(float f, float strength) { return strength == 1.0f ? f : 1.0f - strength * (1.0f - f); }

__global__ void __launch_bounds__(256)
k_shadow_points(GridConsts g, const float* __restrict__ Lm, const float* __restrict__ pts, size_t n, int filter, float strength,
                float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float f = shadow_factor(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], g, Lm, filter);
    out[i] = shadow_strength(f, strength);
}

__global__ void __launch_bounds__(256)
k_shadow_image(GridConsts g, const float* __restrict__ Lm, int W, int H, float aspect, float neg_inv_tan, const CamRows cam,
               const float* __restrict__ depth /* nullable: no geometry anywhere */, int filter, float strength, float* __restrict__ out)
{
    const float* c2w = cam.r;
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), row = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (col >= W || row >= H) return;
    const size_t i = (size_t)row * W + col;
    const float d = depth ? depth[i] : 3.0e38f;
    float res = 1.0f;
    if (!(d >= 3.0e38f) && d > 0.f) {
        // the pixel ray of k_scene_depth (occluders.hip); row 0 = bottom of the view
        const float dx = (2.0f * ((float)col + 0.5f) / (float)W - 1.0f) * aspect;
        const float dy = 2.0f * ((float)row + 0.5f) / (float)H - 1.0f;
        const float dz = neg_inv_tan;
        const float wx = (c2w[0] * dx + c2w[1] * dy) + c2w[2] * dz, wy = (c2w[4] * dx + c2w[5] * dy) + c2w[6] * dz,
                    wz = (c2w[8] * dx + c2w[9] * dy) + c2w[10] * dz;
        const float t = d / (-dz);                            // eye depth = t * (-dz) along this direction
        const float f = shadow_factor(c2w[3] + t * wx, c2w[7] + t * wy, c2w[11] + t * wz, g, Lm, filter);
        res = shadow_strength(f, strength);
    }
    out[i] = res;
}

__global__ void __launch_bounds__(256)
k_shadow_apply(const float* __restrict__ shadow, float4* __restrict__ scene, size_t npix)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    const float s = shadow[i];
    float4 p = scene[i];
    p.x *= s; p.y *= s; p.z *= s;
    scene[i] = p;
}

// the checks every entry point shares, in the order the header documents; nothing is allocated, queued or written before they pass
int shadow_check(vp_ctx* c, const vp_shadow_params* sp, const char* who)
{
    if (c->multi) return vp_fail(c, VP_ERR_UNSUPPORTED, "%s: not available on a fan-out (multi-GPU) context", who);
    if (!sp) return vp_fail(c, VP_ERR_BAD_ARG, "%s: null params", who);
    if (sp->filter != VP_SHADOW_NEAREST && sp->filter != VP_SHADOW_BILINEAR)
        return vp_fail(c, VP_ERR_BAD_ARG, "%s: filter %d (VP_SHADOW_NEAREST or VP_SHADOW_BILINEAR)", who, sp->filter);
    if (!(sp->strength >= 0.f && sp->strength <= 1.f)) return vp_fail(c, VP_ERR_BAD_ARG, "%s: strength %g outside [0, 1]", who, (double)sp->strength);
    if (sp->reserved[0] || sp->reserved[1]) return vp_fail(c, VP_ERR_BAD_ARG, "%s: reserved[] must be 0", who);
    return VP_OK;
}

int shadow_check_state(vp_ctx* c, const char* who)
{
    const vp_config& cfg = c->cfg;
    if (cfg.slab_z0 != 0 || (cfg.slab_z1 != 0 && cfg.slab_z1 != cfg.num_mv[2]))
        return vp_fail(c, VP_ERR_UNSUPPORTED, "%s: the context owns the slab [%d,%d) of the light axis: its map is not the whole column's", who,
                       cfg.slab_z0, cfg.slab_z1);
    if (!c->filled) return vp_fail(c, VP_ERR_STATE, "%s before vp_fill", who);
    return VP_OK;
}

int launch_shadow_points(vp_ctx* c, const float* d_pts, size_t n, const vp_shadow_params* sp, float* d_out)
{
    if (n == 0) return VP_OK;
    hipLaunchKernelGGL(k_shadow_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->g, (const float*)c->d_lightmap, d_pts, n,
                       sp->filter, sp->strength, d_out);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int launch_shadow_image(vp_ctx* c, const vp_camera* cam, const float* d_depth, const vp_shadow_params* sp, float* d_out)
{
    const int W = c->cfg.width, H = c->cfg.height;
    CamRows rows;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) rows.r[r * 4 + k] = cam->camera_to_world[k * 4 + r];
    const float aspect = (float)W / (float)H;
    const float nit = -(1.0f / (float)tan((double)cam->fov_y * 0.5));     // as launch_scene_depth
    hipLaunchKernelGGL(k_shadow_image, dim3((W + 63) / 64, (H + 3) / 4), dim3(256), 0, c->stream, c->g, (const float*)c->d_lightmap, W, H, aspect, nit,
                       rows, d_depth, sp->filter, sp->strength, d_out);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

// the eye depth a NULL scene_depth stands for: the map vp_raymarch renders from the solids and mesh instances, or none at all
int shadow_default_depth(vp_ctx* c, const vp_camera* cam, const float** d_depth)
{
    *d_depth = nullptr;
    if (!has_occluders(c)) return VP_OK;
    int rc = api_ensure_eye_depth(c, cam); if (rc) return rc;
    *d_depth = c->d_scene_depth;
    return VP_OK;
}

}  // namespace

void volume_shadow_free(vp_ctx* c)
{
    float** bufs[] = {&c->d_shadow_depth, &c->d_shadow_image, &c->d_shadow_points, &c->d_shadow_factors};
    for (float** p : bufs) { if (*p) (void)hipFree(*p); *p = nullptr; }
    c->shadow_points_cap = 0;
}

VP_EXPORT int vp_volume_shadow_points_device(vp_ctx* c, const void* d_world_xyz, int64_t n, const vp_shadow_params* sp, void* d_out)
{
    if (!c) return VP_ERR_BAD_ARG;
    int rc = shadow_check(c, sp, "vp_volume_shadow_points_device"); if (rc) return rc;
    if (n < 0 || (n > 0 && (!d_world_xyz || !d_out))) return vp_fail(c, VP_ERR_BAD_ARG, "vp_volume_shadow_points_device: null pointer or negative count");
    if (n > (int64_t)INT32_MAX) return vp_fail(c, VP_ERR_UNSUPPORTED, "vp_volume_shadow_points_device: more than 2^31 - 1 points");
    rc = shadow_check_state(c, "vp_volume_shadow_points_device"); if (rc) return rc;
    VP_HIP(hipSetDevice(c->device));
    return launch_shadow_points(c, (const float*)d_world_xyz, (size_t)n, sp, (float*)d_out);
}

VP_EXPORT int vp_volume_shadow_points(vp_ctx* c, const float* world_xyz, int64_t n, const vp_shadow_params* sp, float* out)
{
    if (!c) return VP_ERR_BAD_ARG;
    int rc = shadow_check(c, sp, "vp_volume_shadow_points"); if (rc) return rc;
    if (n < 0 || (n > 0 && (!world_xyz || !out))) return vp_fail(c, VP_ERR_BAD_ARG, "vp_volume_shadow_points: null pointer or negative count");
    if (n > (int64_t)INT32_MAX) return vp_fail(c, VP_ERR_UNSUPPORTED, "vp_volume_shadow_points: more than 2^31 - 1 points");
    rc = shadow_check_state(c, "vp_volume_shadow_points"); if (rc) return rc;
    if (n == 0) return VP_OK;
    VP_HIP(hipSetDevice(c->device));
    if ((size_t)n > c->shadow_points_cap) {
        if (c->d_shadow_points) (void)hipFree(c->d_shadow_points);
        if (c->d_shadow_factors) (void)hipFree(c->d_shadow_factors);
        c->d_shadow_points = c->d_shadow_factors = nullptr; c->shadow_points_cap = 0;
        const size_t cap = (size_t)n + (size_t)n / 4 + 64;
        VP_HIP(hipMalloc((void**)&c->d_shadow_points, cap * 3 * sizeof(float)));
        VP_HIP(hipMalloc((void**)&c->d_shadow_factors, cap * sizeof(float)));
        c->shadow_points_cap = cap;
    }
    VP_HIP(hipMemcpyAsync(c->d_shadow_points, world_xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    rc = launch_shadow_points(c, c->d_shadow_points, (size_t)n, sp, c->d_shadow_factors); if (rc) return rc;
    VP_HIP(hipMemcpyAsync(out, c->d_shadow_factors, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return api_stream_sync(c);
}

VP_EXPORT int vp_volume_shadow_image_device(vp_ctx* c, const vp_camera* cam, const void* d_scene_depth, const vp_shadow_params* sp, void* d_out)
{
    if (!c) return VP_ERR_BAD_ARG;
    int rc = shadow_check(c, sp, "vp_volume_shadow_image_device"); if (rc) return rc;
    if (!cam || !d_out) return vp_fail(c, VP_ERR_BAD_ARG, "vp_volume_shadow_image_device: null camera / output");
    rc = shadow_check_state(c, "vp_volume_shadow_image_device"); if (rc) return rc;
    VP_HIP(hipSetDevice(c->device));
    const float* d_depth = (const float*)d_scene_depth;
    if (!d_depth) { rc = shadow_default_depth(c, cam, &d_depth); if (rc) return rc; }
    return launch_shadow_image(c, cam, d_depth, sp, (float*)d_out);
}

VP_EXPORT int vp_volume_shadow_image(vp_ctx* c, const vp_camera* cam, const float* scene_depth, const vp_shadow_params* sp, float* out)
{
    if (!c) return VP_ERR_BAD_ARG;
    int rc = shadow_check(c, sp, "vp_volume_shadow_image"); if (rc) return rc;
    if (!cam || !out) return vp_fail(c, VP_ERR_BAD_ARG, "vp_volume_shadow_image: null camera / output");
    rc = shadow_check_state(c, "vp_volume_shadow_image"); if (rc) return rc;
    VP_HIP(hipSetDevice(c->device));
    const size_t npix = (size_t)c->cfg.width * c->cfg.height;
    if (!c->d_shadow_image) VP_HIP(hipMalloc((void**)&c->d_shadow_image, (npix ? npix : 1) * sizeof(float)));
    const float* d_depth = nullptr;
    if (scene_depth) {
        // staged in a buffer of the feature's own: d_scene_depth keeps the rendered map (and its cache tags) for the next vp_raymarch
        if (!c->d_shadow_depth) VP_HIP(hipMalloc((void**)&c->d_shadow_depth, (npix ? npix : 1) * sizeof(float)));
        VP_HIP(hipMemcpyAsync(c->d_shadow_depth, scene_depth, npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
        d_depth = c->d_shadow_depth;
    } else {
        rc = shadow_default_depth(c, cam, &d_depth); if (rc) return rc;
    }
    rc = launch_shadow_image(c, cam, d_depth, sp, c->d_shadow_image); if (rc) return rc;
    VP_HIP(hipMemcpyAsync(out, c->d_shadow_image, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return api_stream_sync(c);
}

VP_EXPORT int vp_apply_shadow_device(vp_ctx* c, const void* d_shadow, void* d_scene_rgba)
{
    if (!c) return VP_ERR_BAD_ARG;
    if (c->multi) return vp_fail(c, VP_ERR_UNSUPPORTED, "vp_apply_shadow_device: not available on a fan-out (multi-GPU) context");
    if (!d_shadow || !d_scene_rgba) return vp_fail(c, VP_ERR_BAD_ARG, "vp_apply_shadow_device: null argument");
    VP_HIP(hipSetDevice(c->device));
    const size_t npix = (size_t)c->cfg.width * c->cfg.height;
    if (npix == 0) return VP_OK;
    hipLaunchKernelGGL(k_shadow_apply, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, c->stream, (const float*)d_shadow, (float4*)d_scene_rgba, npix);
    VP_HIP(hipGetLastError());
    return VP_OK;
}
