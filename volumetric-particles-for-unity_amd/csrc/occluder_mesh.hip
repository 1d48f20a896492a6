// occluder_mesh.hip -- triangle-mesh occluders for the two scene-occlusion inputs (SURVEY section 2 row 11's producer, for meshes).
// In the reference every mesh on the Default layer is rasterised into both maps (VPR.cs:184 + LDM.shader:6 Cull Front; RM.shader:14 ZTest
// against the main camera's depth, Cull Back).  Here the placed instances are RAY-CAST with exactly the rays of occluders.hip (pixel centres,
// same origin / direction / depth), so mesh and analytic results compare tightly, and min()-ed over the map k_light_depth / k_scene_depth left.
//   k_mesh_setup    one thread per (instance, triangle): world-space vertices, conservative facing cull, pixel box padded by one pixel
//                   (eye view: the part in front of the near plane), per-tile counts
//   k_mesh_scan     exclusive scan of the counts (one workgroup) -> CSR starts + the list length (read back by the host: the one wait)
//   k_mesh_scatter  per-tile triangle lists (order inside a list is free: the result is a minimum)
//   k_mesh_tiles    one 256-lane workgroup per 16 x 16 tile, records staged in LDS; a lane = a pixel; watertight ray / triangle test
//                   (Woop, Benthin, Wald 2013, JCGT 2(1), with the double-precision re-test of an edge value of exactly 0); culling by the
//                   sign of the test's determinant, i.e. per ray, consistently with the hit test itself.
// -ffp-contract=off (Makefile): an edge function of a shared edge is the exact negation of its neighbour's.  No fmaf in this file.
#include <cmath>

#include "vpfx_internal.h"

namespace {

constexpr int MESH_TILE = 16;
constexpr unsigned long long MESH_LIST_MAX = 1ull << 28;

struct MeshView {
    int W, H, ntx, nty;
    int eye;                      // 0: light (ortho), 1: main camera (perspective)
    float o[3];                   // light: camera position; eye: camera origin
    float inv[9];                 // rows: world offset from o -> light (lx, ly, t) / eye camera-space (vx, vy, vz)
    float r, t;                   // light: half extents of the ortho frustum
    float negdz, aspect, zclip;   // eye: 1 / tan(fov / 2), W / H, near plane used for the pixel box
    float fwd[3];                 // light direction (cull)
};

__device__ __forceinline__ uint32_t pack2(int a, int b) { return (uint32_t)a | ((uint32_t)b << 16); }

__device__ __forceinline__ void xform(const float* m, const float* p, float* w)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = ((m[r * 4] * p[0] + m[r * 4 + 1] * p[1]) + m[r * 4 + 2] * p[2]) + m[r * 4 + 3];
}

__global__ void __launch_bounds__(256)
k_mesh_setup(MeshView v, const MeshInstDev* __restrict__ inst, const uint32_t* __restrict__ first, int n_inst, uint32_t n_tris,
             const float* __restrict__ pos, const int32_t* __restrict__ idx, MeshTri* __restrict__ rec, uint32_t* __restrict__ cnt)
{
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= n_tris) return;
    int lo = 0, hi = n_inst - 1;                             // the instance whose range holds gid: largest i with first[i] <= gid
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= gid) lo = mid; else hi = mid - 1; }
    const MeshInstDev& I = inst[lo];
    const size_t tri = (size_t)I.first_triangle + (gid - first[lo]);
    float a[3], b[3], c[3];
    xform(I.m, pos + (size_t)idx[tri * 3] * 3, a);
    xform(I.m, pos + (size_t)idx[tri * 3 + 1] * 3, b);
    xform(I.m, pos + (size_t)idx[tri * 3 + 2] * 3, c);
    if (I.mirrored) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { const float s = b[k]; b[k] = c[k]; c[k] = s; }
    }
    // outward normal and a conservative facing cull (the exact decision is per ray, in k_mesh_tiles)
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const float N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float scale = sqrtf((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]) * sqrtf((e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]);
    bool keep;
    float fx0 = 3.0e38f, fx1 = -3.0e38f, fy0 = 3.0e38f, fy1 = -3.0e38f;
    if (!v.eye) {
        const float d = (N[0] * v.fwd[0] + N[1] * v.fwd[1]) + N[2] * v.fwd[2];
        keep = d >= -1e-4f * scale;                          // Cull Front: only faces turned away from the light
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* P = k == 0 ? a : (k == 1 ? b : c);
            const float q0 = P[0] - v.o[0], q1 = P[1] - v.o[1], q2 = P[2] - v.o[2];
            const float lx = (v.inv[0] * q0 + v.inv[1] * q1) + v.inv[2] * q2, ly = (v.inv[3] * q0 + v.inv[4] * q1) + v.inv[5] * q2;
            const float X = (lx + v.r) / (2.0f * v.r) * (float)v.W - 0.5f, Y = (ly + v.t) / (2.0f * v.t) * (float)v.H - 0.5f;
            fx0 = fminf(fx0, X); fx1 = fmaxf(fx1, X); fy0 = fminf(fy0, Y); fy1 = fmaxf(fy1, Y);
        }
    } else {
        const float q[3] = {a[0] - v.o[0], a[1] - v.o[1], a[2] - v.o[2]};
        const float d = (N[0] * q[0] + N[1] * q[1]) + N[2] * q[2];
        const float ql = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
        keep = d <= 1e-4f * scale * ql;                      // Cull Back: only faces turned towards the camera
        // camera-space vertices; depth = -vz; the polygon clipped to depth >= zclip bounds every pixel centre whose ray hits at depth >= near
        float vx[3], vy[3], dep[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* P = k == 0 ? a : (k == 1 ? b : c);
            const float q0 = P[0] - v.o[0], q1 = P[1] - v.o[1], q2 = P[2] - v.o[2];
            vx[k] = (v.inv[0] * q0 + v.inv[1] * q1) + v.inv[2] * q2;
            vy[k] = (v.inv[3] * q0 + v.inv[4] * q1) + v.inv[5] * q2;
            dep[k] = -((v.inv[6] * q0 + v.inv[7] * q1) + v.inv[8] * q2);
        }
        int nin = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int j = k == 2 ? 0 : k + 1;
            const bool ik = dep[k] >= v.zclip, ij = dep[j] >= v.zclip;
            float px = 0.f, py = 0.f, pz = 0.f;
            bool emit = false;
            if (ik) { px = vx[k]; py = vy[k]; pz = dep[k]; emit = true; ++nin; }
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                if (pass == 1) {
                    if (ik == ij) break;
                    const float s = (v.zclip - dep[k]) / (dep[j] - dep[k]);
                    px = vx[k] + s * (vx[j] - vx[k]); py = vy[k] + s * (vy[j] - vy[k]); pz = v.zclip; emit = true;
                }
                if (emit) {
                    const float X = ((px * v.negdz / pz) / v.aspect + 1.0f) * (float)v.W * 0.5f - 0.5f;
                    const float Y = (py * v.negdz / pz + 1.0f) * (float)v.H * 0.5f - 0.5f;
                    fx0 = fminf(fx0, X); fx1 = fmaxf(fx1, X); fy0 = fminf(fy0, Y); fy1 = fmaxf(fy1, Y);
                    emit = false;
                }
            }
        }
        keep = keep && nin > 0;
    }
    // pixel box padded by one pixel, clamped before the conversion to int
    fx0 = fmaxf(fx0, -4.0f); fy0 = fmaxf(fy0, -4.0f); fx1 = fminf(fx1, (float)v.W + 4.0f); fy1 = fminf(fy1, (float)v.H + 4.0f);
    const int X0 = max(0, (int)floorf(fx0) - 1), X1 = min(v.W - 1, (int)ceilf(fx1) + 1);
    const int Y0 = max(0, (int)floorf(fy0) - 1), Y1 = min(v.H - 1, (int)ceilf(fy1) + 1);
    int tx0 = X0 / MESH_TILE, tx1 = X1 / MESH_TILE, ty0 = Y0 / MESH_TILE, ty1 = Y1 / MESH_TILE;
    if (!keep || X0 > X1 || Y0 > Y1) { tx0 = 1; tx1 = 0; ty0 = 1; ty1 = 0; }
    MeshTri o;
    o.p0 = make_float4(a[0], a[1], a[2], b[0]);
    o.p1 = make_float4(b[1], b[2], c[0], c[1]);
    o.p2 = make_float4(c[2], __uint_as_float(pack2(tx0, ty0)), __uint_as_float(pack2(tx1, ty1)), 0.f);
    rec[gid] = o;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&cnt[ty * v.ntx + tx], 1u);
}

// exclusive scan of the per-tile counts (one workgroup); start[n] = total; the counts are zeroed for k_mesh_scatter's cursors
__global__ void __launch_bounds__(1024)
k_mesh_scan(uint32_t* __restrict__ cnt, unsigned long long* __restrict__ start, int n)
{
    __shared__ unsigned long long s[1024];
    const int tid = threadIdx.x, per = (n + 1023) / 1024, b = tid * per, e = min(n, b + per);
    unsigned long long sum = 0;
    for (int i = b; i < e; ++i) sum += cnt[i];
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned long long add = tid >= off ? s[tid - off] : 0ull;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    unsigned long long run = s[tid] - sum;
    for (int i = b; i < e; ++i) { start[i] = run; run += cnt[i]; cnt[i] = 0u; }
    if (tid == 1023) start[n] = s[1023];
}

__global__ void __launch_bounds__(256)
k_mesh_scatter(const MeshTri* __restrict__ rec, uint32_t n_tris, int ntx, const unsigned long long* __restrict__ start, uint32_t* __restrict__ cur,
               uint32_t* __restrict__ list)
{
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= n_tris) return;
    const float4 p2 = rec[gid].p2;
    const uint32_t lo = __float_as_uint(p2.y), hi = __float_as_uint(p2.z);
    const int tx0 = lo & 0xffff, ty0 = lo >> 16, tx1 = hi & 0xffff, ty1 = hi >> 16;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int t = ty * ntx + tx;
            list[start[t] + atomicAdd(&cur[t], 1u)] = gid;
        }
}

__device__ __forceinline__ float pick(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// Woop / Benthin / Wald watertight test.  Returns the ray parameter of an accepted hit (the determinant's sign = `want`), else 3e38.
// det = U + V + W = -(Cross(b - a, c - a) . dir) * (positive factor): want_neg selects faces whose outward normal points along the ray.
__device__ __forceinline__ float ray_tri(const float4 p0, const float4 p1, const float4 p2, float ox, float oy, float oz, int kx, int ky, int kz,
                                         float Sx, float Sy, float Sz, bool want_neg)
{
    const float A0 = p0.x - ox, A1 = p0.y - oy, A2 = p0.z - oz;
    const float B0 = p0.w - ox, B1 = p1.x - oy, B2 = p1.y - oz;
    const float C0 = p1.z - ox, C1 = p1.w - oy, C2 = p2.x - oz;
    const float Akz = pick(A0, A1, A2, kz), Bkz = pick(B0, B1, B2, kz), Ckz = pick(C0, C1, C2, kz);
    const float Ax = pick(A0, A1, A2, kx) - Sx * Akz, Ay = pick(A0, A1, A2, ky) - Sy * Akz;
    const float Bx = pick(B0, B1, B2, kx) - Sx * Bkz, By = pick(B0, B1, B2, ky) - Sy * Bkz;
    const float Cx = pick(C0, C1, C2, kx) - Sx * Ckz, Cy = pick(C0, C1, C2, ky) - Sy * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (U == 0.f || V == 0.f || W == 0.f) {
        U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
        V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
        W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
    }
    if ((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f)) return 3.0e38f;
    const float det = (U + V) + W;
    if (want_neg ? !(det < 0.f) : !(det > 0.f)) return 3.0e38f;
    const float T = (U * (Sz * Akz) + V * (Sz * Bkz)) + W * (Sz * Ckz);
    return T / det;
}

__device__ __forceinline__ void ray_frame(float dx, float dy, float dz, int& kx, int& ky, int& kz, float& Sx, float& Sy, float& Sz)
{
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    kz = (ax > ay) ? (ax > az ? 0 : 2) : (ay > az ? 1 : 2);
    kx = kz == 2 ? 0 : kz + 1;
    ky = kx == 2 ? 0 : kx + 1;
    const float dkz = pick(dx, dy, dz, kz);
    if (dkz < 0.f) { const int s = kx; kx = ky; ky = s; }   // keeps the winding
    Sx = pick(dx, dy, dz, kx) / dkz; Sy = pick(dx, dy, dz, ky) / dkz; Sz = 1.0f / dkz;
}

// One workgroup per tile; view 0 = light depth (the rays of k_light_depth), 1 = eye depth (the rays of k_scene_depth).
__global__ void __launch_bounds__(256)
k_mesh_tiles(int view, GridConsts g, float nearz, float farz, float cam_dist,                         // light
             int W, int H, float aspect, float neg_inv_tan, float nearc, float farc, float3 c0, float3 c1, float3 c2, float3 corg,   // eye
             int ntx, const MeshTri* __restrict__ rec, const unsigned long long* __restrict__ start, const uint32_t* __restrict__ list,
             float* __restrict__ out)
{
    __shared__ float4 s_rec[3][256];
    const int tile = blockIdx.x, tid = threadIdx.x;
    const int X = (tile % ntx) * MESH_TILE + (tid & 15), Y = (tile / ntx) * MESH_TILE + (tid >> 4);
    float ox, oy, oz, dx, dy, dz;
    bool inside;
    if (view == 0) {
        const int LW = g.Nx * g.nv, LH = g.Ny * g.nv;
        inside = X < LW && Y < LH;
        const float r = (float)g.Nx * g.s * 0.5f, t = (float)g.Ny * g.s * 0.5f;           // exactly k_light_depth's ray
        const float lx = -r + ((float)X + 0.5f) / (float)LW * (2.0f * r);
        const float ly = -t + ((float)Y + 0.5f) / (float)LH * (2.0f * t);
        const float cx = g.gc[0] - g.fwd[0] * cam_dist, cy = g.gc[1] - g.fwd[1] * cam_dist, cz = g.gc[2] - g.fwd[2] * cam_dist;
        ox = cx + g.Rl[0] * lx + g.Rl[1] * ly; oy = cy + g.Rl[3] * lx + g.Rl[4] * ly; oz = cz + g.Rl[6] * lx + g.Rl[7] * ly;
        dx = g.fwd[0]; dy = g.fwd[1]; dz = g.fwd[2];
    } else {
        inside = X < W && Y < H;
        const float ex = (2.0f * ((float)X + 0.5f) / (float)W - 1.0f) * aspect;              // exactly k_scene_depth's ray
        const float ey = 2.0f * ((float)Y + 0.5f) / (float)H - 1.0f;
        const float ez = neg_inv_tan;
        dx = (c0.x * ex + c0.y * ey) + c0.z * ez; dy = (c1.x * ex + c1.y * ey) + c1.z * ez; dz = (c2.x * ex + c2.y * ey) + c2.z * ez;
        ox = corg.x; oy = corg.y; oz = corg.z;
    }
    int kx, ky, kz;
    float Sx, Sy, Sz;
    ray_frame(dx, dy, dz, kx, ky, kz, Sx, Sy, Sz);
    const bool want_neg = view == 0;                         // light: back faces (Cull Front); eye: front faces (Cull Back)
    const float tlo = view == 0 ? nearz : 0.f;
    float best = 3.0e38f;
    const unsigned long long b = start[tile], e = start[tile + 1];
    for (unsigned long long base = b; base < e; base += 256) {
        const int n = (int)min(256ull, e - base);
        __syncthreads();
        if (tid < n) {
            const MeshTri r = rec[list[base + tid]];
            s_rec[0][tid] = r.p0; s_rec[1][tid] = r.p1; s_rec[2][tid] = r.p2;
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const float th = ray_tri(s_rec[0][k], s_rec[1][k], s_rec[2][k], ox, oy, oz, kx, ky, kz, Sx, Sy, Sz, want_neg);
            if (view == 0) {
                if (th >= tlo && th <= farz) best = fminf(best, th);
            } else {
                const float depth = th * (-neg_inv_tan);
                if (th > 0.f && th < 3.0e38f && depth >= nearc && depth <= farc) best = fminf(best, depth);
            }
        }
    }
    if (!inside || !(best < 3.0e38f)) return;
    const size_t o = view == 0 ? (size_t)Y * (g.Nx * g.nv) + X : (size_t)Y * W + X;
    const float val = view == 0 ? (best - nearz) / (farz - nearz) : best;
    out[o] = fminf(out[o], val);
}

template <typename T>
int grow(vp_ctx* c, T** p, size_t* cap, size_t need)
{
    if (need <= *cap && *p) return VP_OK;
    const size_t n = need + need / 2 + 64;
    T* q = nullptr;
    if (hipMalloc((void**)&q, n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return vp_fail(c, VP_ERR_OOM, "mesh occluders: device allocation failed"); }
    if (*p) (void)hipFree(*p);
    *p = q; *cap = n;
    return VP_OK;
}

void inv3(const double m[9], float out[9])          // rows of m^-1 (m row-major); a singular m gives zeros (no box, nothing drawn)
{
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    const double id = det != 0.0 ? 1.0 / det : 0.0;
    const double r[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                         m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                         m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
    for (int i = 0; i < 9; ++i) out[i] = (float)(r[i] * id);
}

// setup + binning of one view; returns with d_mesh_tile_start / d_mesh_list ready for k_mesh_tiles
int mesh_bin(vp_ctx* c, const MeshView& v)
{
    const size_t ntiles = (size_t)v.ntx * v.nty;
    int rc;
    if ((rc = grow(c, &c->d_mesh_rec, &c->mesh_rec_cap, c->n_mesh_tris))) return rc;
    if (ntiles + 1 > c->mesh_tiles_cap || !c->d_mesh_tile_count) {
        uint32_t* cnt = nullptr; unsigned long long* st = nullptr;
        const size_t n = ntiles + 1;
        if (hipMalloc((void**)&cnt, n * sizeof(uint32_t)) != hipSuccess || hipMalloc((void**)&st, n * sizeof(unsigned long long)) != hipSuccess) {
            (void)hipGetLastError(); if (cnt) (void)hipFree(cnt);
            return vp_fail(c, VP_ERR_OOM, "mesh occluders: device allocation failed");
        }
        if (c->d_mesh_tile_count) (void)hipFree(c->d_mesh_tile_count);
        if (c->d_mesh_tile_start) (void)hipFree(c->d_mesh_tile_start);
        c->d_mesh_tile_count = cnt; c->d_mesh_tile_start = st; c->mesh_tiles_cap = n;
    }
    if (!c->h_mesh_total) VP_HIP(hipHostMalloc((void**)&c->h_mesh_total, sizeof(unsigned long long), hipHostMallocDefault));
    VP_HIP(hipMemsetAsync(c->d_mesh_tile_count, 0, ntiles * sizeof(uint32_t), c->stream));
    const unsigned blocks = (c->n_mesh_tris + 255u) / 256u;
    hipLaunchKernelGGL(k_mesh_setup, dim3(blocks), dim3(256), 0, c->stream, v, c->d_mesh_inst, c->d_mesh_inst_first, c->n_mesh_inst, c->n_mesh_tris,
                       c->d_mesh_pos, c->d_mesh_idx, c->d_mesh_rec, c->d_mesh_tile_count);
    VP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(1024), 0, c->stream, c->d_mesh_tile_count, c->d_mesh_tile_start, (int)ntiles);
    VP_HIP(hipGetLastError());
    VP_HIP(hipMemcpyAsync(c->h_mesh_total, c->d_mesh_tile_start + ntiles, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    VP_HIP(hipStreamSynchronize(c->stream));                  // the one host wait of the mesh path: the list length
    const unsigned long long total = *c->h_mesh_total;
    if (total > MESH_LIST_MAX)
        return vp_fail(c, VP_ERR_UNSUPPORTED, "mesh occluders: %llu triangle / tile pairs in one view (limit 2^28)", total);
    if ((rc = grow(c, &c->d_mesh_list, &c->mesh_list_cap, (size_t)total))) return rc;
    hipLaunchKernelGGL(k_mesh_scatter, dim3(blocks), dim3(256), 0, c->stream, c->d_mesh_rec, c->n_mesh_tris, v.ntx, c->d_mesh_tile_start,
                       c->d_mesh_tile_count, c->d_mesh_list);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

}  // namespace

int launch_mesh_light_depth(vp_ctx* c, float nearz, float farz, float cam_dist, float* d_out)
{
    if (c->n_mesh_tris == 0) return VP_OK;
    const GridConsts& g = c->g;
    MeshView v{};
    v.W = g.Nx * g.nv; v.H = g.Ny * g.nv;
    v.ntx = (v.W + MESH_TILE - 1) / MESH_TILE; v.nty = (v.H + MESH_TILE - 1) / MESH_TILE;
    v.eye = 0;
    for (int k = 0; k < 3; ++k) { v.o[k] = g.gc[k] - g.fwd[k] * cam_dist; v.fwd[k] = g.fwd[k]; }
    // columns: the ortho camera's x / y axes as k_light_depth steps along them, and the ray direction
    const double m[9] = {g.Rl[0], g.Rl[1], g.fwd[0], g.Rl[3], g.Rl[4], g.fwd[1], g.Rl[6], g.Rl[7], g.fwd[2]};
    inv3(m, v.inv);
    v.r = (float)g.Nx * g.s * 0.5f; v.t = (float)g.Ny * g.s * 0.5f;
    int rc = mesh_bin(c, v); if (rc) return rc;
    const float3 z3 = make_float3(0.f, 0.f, 0.f);
    hipLaunchKernelGGL(k_mesh_tiles, dim3(v.ntx * v.nty), dim3(256), 0, c->stream, 0, g, nearz, farz, cam_dist, 0, 0, 0.f, 0.f, 0.f, 0.f, z3, z3, z3, z3,
                       v.ntx, c->d_mesh_rec, c->d_mesh_tile_start, c->d_mesh_list, d_out);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

int launch_mesh_scene_depth(vp_ctx* c, const vp_camera* cam, float* d_out)
{
    if (c->n_mesh_tris == 0) return VP_OK;
    const int W = c->cfg.width, H = c->cfg.height;
    const float* m = cam->camera_to_world;                    // column-major: element (r, k) = m[k * 4 + r]
    MeshView v{};
    v.W = W; v.H = H; v.ntx = (W + MESH_TILE - 1) / MESH_TILE; v.nty = (H + MESH_TILE - 1) / MESH_TILE;
    v.eye = 1;
    for (int r = 0; r < 3; ++r) v.o[r] = m[12 + r];
    const double c3[9] = {m[0], m[4], m[8], m[1], m[5], m[9], m[2], m[6], m[10]};
    inv3(c3, v.inv);
    v.aspect = (float)W / (float)H;
    const float nit = -(1.0f / (float)tan((double)cam->fov_y * 0.5));   // as launch_scene_depth
    v.negdz = -nit;
    v.zclip = fmaxf(cam->near_clip, 1e-20f);
    int rc = mesh_bin(c, v); if (rc) return rc;
    const float3 c0 = make_float3(m[0], m[4], m[8]), c1 = make_float3(m[1], m[5], m[9]), c2 = make_float3(m[2], m[6], m[10]);
    const float3 org = make_float3(m[12], m[13], m[14]);
    hipLaunchKernelGGL(k_mesh_tiles, dim3(v.ntx * v.nty), dim3(256), 0, c->stream, 1, c->g, 0.f, 0.f, 0.f, W, H, v.aspect, nit, cam->near_clip,
                       cam->far_clip > 0.f ? cam->far_clip : 3.0e38f, c0, c1, c2, org, v.ntx, c->d_mesh_rec, c->d_mesh_tile_start, c->d_mesh_list, d_out);
    VP_HIP(hipGetLastError());
    return VP_OK;
}

void mesh_free_all(vp_ctx* c)
{
    void* dev[] = {c->d_mesh_pos, c->d_mesh_idx, c->d_mesh_inst, c->d_mesh_inst_first, c->d_mesh_rec, c->d_mesh_tile_count, c->d_mesh_tile_start, c->d_mesh_list};
    for (void* p : dev) if (p) (void)hipFree(p);
    if (c->h_mesh_total) (void)hipHostFree(c->h_mesh_total);
}
