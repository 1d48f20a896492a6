// mv_box.h -- the per-metavoxel voxel box: an axis-aligned box, in the brick's voxel index space (px, py, slice), of the voxels that some
// listed particle's sphere can cover.  Written at bin time (bin.hip), read by the ray-march (raymarch_kernels.h: march_mv starts a visit at
// the box instead of at the far face of the unit cube).  Plain C++ / HIP: a CPU program can include it (tests/test_mv_box_cpu.py).
//
// Containment: the fill marks a voxel covered when d^2 <= 0.25 in particle space (Fill.shader:172,196), and shades a (tile, particle)
// pair only when its pre-cull calls the pair "near".  The pre-cull is a sphere (cx, cy, cz, rv) in voxel-index coordinates; this file uses
// its expressions literally (fill_kernels.h, the `cx, cy, cz, rv` block, margin `* 1.002 + 0.05` included), so whatever the pre-cull can call
// near lies inside the box, and no voxel outside the box ever receives density.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VPFX_BOX_HD __host__ __device__
#else
#define VPFX_BOX_HD
#endif

struct MvBox { int lo[3], hi[3]; };     // inclusive voxel indices per axis (x = px, y = py, z = slice); empty when lo[0] > hi[0]

VPFX_BOX_HD inline MvBox mv_box_empty() { return MvBox{{255, 255, 255}, {-1, -1, -1}}; }
VPFX_BOX_HD inline bool mv_box_is_empty(const MvBox& b) { return b.lo[0] > b.hi[0]; }

// The voxel-index box of ONE particle (world position and size w = (x, y, z, size)) in the brick of the metavoxel at world position mv:
// centre and radius exactly as the fill's pre-cull forms them (Rl = the light rotation, row-major; inv_sb = 1 / bordered metavoxel size).
// Column centres sit at px + 0.5, slices at s (quirk Q4: no half-voxel offset in z): lo = ceil(c - r - off), hi = floor(c + r - off),
// clamped to [0, nv - 1].  Returns false when the sphere misses the brick's index range on some axis (nothing of it can be covered).
// Compile with -ffp-contract=off like the library: the expressions must round as the pre-cull's do.
VPFX_BOX_HD inline bool mv_box_of_particle(float wx, float wy, float wz, float wsize, float mvx, float mvy, float mvz, const float* Rl /* [9] */,
                                           float inv_sb, int nv, MvBox& out)
{
    const float fnv = (float)nv;
    const float dx = wx - mvx, dy = wy - mvy, dz = wz - mvz;
    const float sc_v = fnv * inv_sb;                                        // voxels per world unit
    const float cx = ((Rl[0] * dx + Rl[3] * dy) + Rl[6] * dz) * sc_v + 0.5f * fnv;
    const float cy = ((Rl[1] * dx + Rl[4] * dy) + Rl[7] * dz) * sc_v + 0.5f * fnv;
    const float cz = ((Rl[2] * dx + Rl[5] * dy) + Rl[8] * dz) * sc_v + 0.5f * fnv;
    const float rv = 0.5f * wsize * sc_v * 1.002f + 0.05f;
    const float c[3] = {cx, cy, cz}, off[3] = {0.5f, 0.5f, 0.0f};
    bool any = true;
    for (int a = 0; a < 3; ++a) {
        const float lo = fmaxf(ceilf((c[a] - rv) - off[a]), 0.0f), hi = fminf(floorf((c[a] + rv) - off[a]), fnv - 1.0f);
        if (!(lo <= hi)) any = false;                                       // (also a NaN centre: never listed by the bin, refused all the same)
        out.lo[a] = (int)fminf(lo, 255.0f); out.hi[a] = (int)fmaxf(hi, -1.0f);
    }
    return any;
}

VPFX_BOX_HD inline void mv_box_union(MvBox& acc, const MvBox& b)
{
    for (int a = 0; a < 3; ++a) { acc.lo[a] = b.lo[a] < acc.lo[a] ? b.lo[a] : acc.lo[a]; acc.hi[a] = b.hi[a] > acc.hi[a] ? b.hi[a] : acc.hi[a]; }
}

// Storage: two words per cell, one byte per field (nv <= 64: seven bits each) so that the ray-march converts a field to float with one
// byte-convert instruction.  x = lo.x | lo.y << 8 | lo.z << 16 | empty << 31, y = hi.x | hi.y << 8 | hi.z << 16.
#define VPFX_MVBOX_EMPTY_X 0x80ffffffu
#define VPFX_MVBOX_EMPTY_Y 0x00000000u
// "no statement": every voxel index a brick can have -- the clip then never moves a visit's start
#define VPFX_MVBOX_FULL_X 0x00000000u
#define VPFX_MVBOX_FULL_Y 0x00ffffffu

VPFX_BOX_HD inline void mv_box_pack(const MvBox& b, uint32_t& x, uint32_t& y)
{
    if (mv_box_is_empty(b)) { x = VPFX_MVBOX_EMPTY_X; y = VPFX_MVBOX_EMPTY_Y; return; }
    x = (uint32_t)b.lo[0] | (uint32_t)b.lo[1] << 8 | (uint32_t)b.lo[2] << 16;
    y = (uint32_t)b.hi[0] | (uint32_t)b.hi[1] << 8 | (uint32_t)b.hi[2] << 16;
}

VPFX_BOX_HD inline MvBox mv_box_unpack(uint32_t x, uint32_t y)
{
    if (x >> 31) return mv_box_empty();
    return MvBox{{(int)(x & 255u), (int)((x >> 8) & 255u), (int)((x >> 16) & 255u)}, {(int)(y & 255u), (int)((y >> 8) & 255u), (int)((y >> 16) & 255u)}};
}
