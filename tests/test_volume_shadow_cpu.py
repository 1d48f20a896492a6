"""CPU: the volume-shadow projection (include/vpfx.h "volume shadows") proven on its numpy twin, tests/shadow_twin.py -- the float32 form is
what tests/test_gpu_volume_shadow.py holds the kernels to bit for bit, so what is shown here about the twin is shown about them.

  closed forms     a map of ones; points in front of the grid, beside it, not finite; points behind the far face
  affine map       bilinear sampling reproduces an affine function of the texel centres' light-space position across metavoxel seams, with
                   odd and even N: pins the tile mapping, the border overlap and the integer N/2
  oracle           nearest sampling at the voxel-column centres built from vp_get_mv_positions and SURVEY A.3's v0 returns the CPU oracle's
                   light map texel for texel: the mapping agrees with the fill's, independently of the twin's own formulas
  ABI              the new prototypes and the parameter struct"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import shadow_twin as T
from oracle import oracle as O
from vpfx_amd import abi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(3, 2, 2), (2, 3, 4)]
NV = 8
CASES = [(N, b) for N in GRIDS for b in (0, 1, 2)]
IDS = [f"N{N[0]}{N[1]}{N[2]}_b{b}" for N, b in CASES]


def consts(sc, dtype):
    return T.grid_consts(sc.N, sc.nv, sc.border, sc.mv_scale, sc.light_to_world, sc.grid_center, dtype)


def light_to_world64(sc):
    return T.rows_of(sc.light_to_world).astype(np.float64)


def grid_box(sc, g64):
    """Light-space box of the grid's footprint and depth: lsO + [-(N/2) - 0.5, N - N/2 - 0.5] s with integer N/2."""
    n, s = np.array(sc.N), float(g64["s"])
    lo = g64["lsO"] - (n // 2 + 0.5) * s
    return lo, lo + n * s


def world_of(ls, sc):
    """World points (float32) of light-space points (float64)."""
    L = light_to_world64(sc)
    return (ls @ L[:3, :3].T + L[:3, 3]).astype(F)


def random_map(sc, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.05, 0.95, (sc.N[1] * sc.nv, sc.N[0] * sc.nv)).astype(F)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,b", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", [F, np.float64], ids=["f32", "f64"])
def test_a_map_of_ones_gives_one_everywhere(N, b, dtype):
    sc, _ = T.make_case(N, NV, b)
    g = consts(sc, dtype)
    lo, hi = grid_box(sc, consts(sc, np.float64))
    rng = np.random.default_rng(1)
    p = world_of(rng.uniform(lo - 4.0, hi + 4.0, (4096, 3)), sc)
    ones = np.ones((N[1] * NV, N[0] * NV), dtype=F)
    for filt in (T.NEAREST, T.BILINEAR):
        for strength in (1.0, 0.37):
            assert np.all(T.factor(p, g, ones, filt, strength) == 1.0)


@pytest.mark.parametrize("N,b", CASES, ids=IDS)
def test_points_outside_the_lit_column_get_one_and_points_behind_it_the_map(N, b):
    sc, _ = T.make_case(N, NV, b)
    g, g64 = consts(sc, F), consts(sc, np.float64)
    lo, hi = grid_box(sc, g64)
    Lm = random_map(sc)
    rng = np.random.default_rng(2)
    n = 2000
    xy = rng.uniform(lo[:2] + 0.01, hi[:2] - 0.01, (n, 2))
    inside = np.column_stack([xy, rng.uniform(lo[2] + 0.01, hi[2] - 0.01, n)])
    front = np.column_stack([xy, rng.uniform(lo[2] - 50.0, lo[2] - 0.01, n)])                 # between the light and the near face
    behind = np.column_stack([xy, rng.uniform(hi[2] + 0.01, hi[2] + 500.0, n)])               # behind the far face
    side = inside.copy()
    k = rng.integers(0, 2, n)
    side[np.arange(n), k] = np.where(rng.random(n) < 0.5, lo[k] - rng.uniform(0.01, 9.0, n), hi[k] + rng.uniform(0.01, 9.0, n))
    bad = world_of(inside[:6], sc)
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, 1], bad[5] = np.nan, np.inf, -np.inf, -np.inf, np.nan, np.nan
    for filt in (T.NEAREST, T.BILINEAR):
        for g_ in (g, g64):
            assert np.all(T.factor(world_of(front, sc), g_, Lm, filt) == 1.0)
            assert np.all(T.factor(world_of(side, sc), g_, Lm, filt) == 1.0)
            assert np.all(T.factor(bad, g_, Lm, filt, 0.5) == 1.0)
            f_in, f_behind = T.factor(world_of(inside, sc), g_, Lm, filt), T.factor(world_of(behind, sc), g_, Lm, filt)
            assert np.all(f_in < 1.0) and np.all(f_behind < 1.0)
    # behind the far face: the value of the map in that column -- the same texel a point inside the grid on the same light ray reads
    # (nearest mode; points within 1e-3 texel of a texel edge left out: the two world points round differently)
    _, _, tx, ty, _ = T.factor(world_of(inside, sc), g64, Lm, T.NEAREST, details=True)
    clear = (np.abs(tx + 0.5 - np.rint(tx + 0.5)) > 1e-3) & (np.abs(ty + 0.5 - np.rint(ty + 0.5)) > 1e-3)
    assert clear.sum() > 0.99 * n
    a, c = T.factor(world_of(inside, sc), g, Lm, T.NEAREST), T.factor(world_of(behind, sc), g, Lm, T.NEAREST)
    assert np.array_equal(a[clear], c[clear]) and len(np.unique(a)) > 50
    # strength scales the darkening: 1 - k (1 - f)
    half = T.factor(world_of(inside, sc), g, Lm, T.NEAREST, 0.5)
    assert np.array_equal(half, F(1.0) - F(0.5) * (F(1.0) - a))


# ---- affine map ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,b", CASES, ids=IDS)
def test_bilinear_sampling_reproduces_an_affine_map_across_seams(N, b):
    sc, _ = T.make_case(N, NV, b)
    g64 = consts(sc, np.float64)
    nv, s = NV, float(g64["s"])
    one = s / (nv - 2 * b)                                                                # sb / nv
    lsO = g64["lsO"]
    c0, cx, cy = 0.55, 0.031, -0.047
    # centre of texel (xx, px): lsO.x + (xx - Nx/2) s + (px + 0.5 - nv/2) one, integer Nx/2; border texels lie in the neighbour's cube
    X, Y = np.arange(N[0] * nv), np.arange(N[1] * nv)
    cxs = lsO[0] + (X // nv - N[0] // 2) * s + (X % nv + 0.5 - nv / 2.0) * one
    cys = lsO[1] + (Y // nv - N[1] // 2) * s + (Y % nv + 0.5 - nv / 2.0) * one
    exact_map = c0 + cx * cxs[None, :] + cy * cys[:, None]
    Lm = exact_map.astype(F)
    lo, hi = grid_box(sc, g64)
    rng = np.random.default_rng(4)
    n = 20000
    ls = rng.uniform(lo + 1e-6, hi - 1e-6, (n, 3))
    # every seam gets points within a tenth of a voxel on both sides
    for k in (0, 1):
        seams = lo[k] + s * np.arange(1, N[k])
        m = n // 4
        ls[k * m:(k + 1) * m, k] = rng.choice(seams, m) + rng.uniform(-0.1, 0.1, m) * one
    p = world_of(ls, sc)
    got, inside, tx, ty, _ = T.factor(p, g64, Lm, T.BILINEAR, details=True)
    assert inside.all()
    lsp = T.light_space(p, g64)                                                           # of the ROUNDED world points, in double
    want = c0 + cx * lsp[0] + cy * lsp[1]
    if b == 0:
        # no border: the tile's edge texels are clamped (the bricks are filtered the same way), so within half a voxel of a tile edge the
        # sample is one-sided by design and the affine function is not reproduced there
        free = (tx >= 0) & (tx <= nv - 1) & (ty >= 0) & (ty <= nv - 1)
        assert 5000 < free.sum() < n                                                      # (the seam points all fall in that band)
    else:
        free = np.ones(n, dtype=bool)
    # Bound: (1) every texel of the map is the float32 rounding of the exact affine value: off by <= 2^-24 max|Lm|, and the bilinear sample is a
    # convex combination of four texels, so it inherits that bound; (2) double rounding in the twin and in `want`: light space is a sum of four
    # terms of magnitude <= M = 4 max(|Linv|) max(|p|, 1), about 16 roundings of 2^-53 M on the way to the texel coordinate (in light-space
    # units), which moves the affine value by (|cx| + |cy|) times that; (3) the interpolation itself, 6 roundings of 2^-53 max|Lm|.
    amax = float(np.abs(exact_map).max())
    M = 4.0 * float(np.abs(g64["Linv"]).max()) * max(float(np.abs(p).max()), 1.0)
    bound = 2.0 ** -24 * amax + (abs(cx) + abs(cy)) * 16 * 2.0 ** -53 * M + 6 * 2.0 ** -53 * amax
    err = np.abs(got - want)[free]
    print(f"N={N} b={b}: max error {err.max():.3e}, bound {bound:.3e}, points {free.sum()}, near seams {n // 2}")
    assert err.max() <= bound
    assert bound < 1e-7                                                                   # ... and that is far below one texel's step
    assert min(abs(cx), abs(cy)) * one > 1e4 * bound


# ---- independent of the twin's mapping: the oracle's fill --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,b", CASES, ids=IDS)
def test_nearest_sampling_at_the_voxel_column_centres_returns_the_oracles_light_map(N, b):
    sc, ground = T.make_case(N, NV, b)
    ora = O.Oracle(sc.config())
    ora.set_frame(sc.light_to_world, sc.grid_center)
    ora.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    ora.set_occluders([ground])
    sc.light_depth_map = ora.render_light_depth()
    ora.fill(sc.fill_params())
    Lm = ora.read_lightmap()
    world, Y, X = T.column_centres(ora.mv_positions(), sc.light_to_world, NV, b, sc.mv_scale, zz=N[2] - 1, z_local=-0.25)
    ora.close()
    assert (sc.light_depth_map < 1.0).any() and Lm.min() < 0.9 and len(np.unique(Lm)) > 20          # the map is not trivial
    assert world.shape[:4] == (N[1], N[0], NV - 2 * b, NV - 2 * b)
    got = T.factor(world.reshape(-1, 3), consts(sc, F), Lm, T.NEAREST)
    assert np.array_equal(got.reshape(Y.shape), Lm[Y, X])
    got64 = T.factor(world.reshape(-1, 3), consts(sc, np.float64), Lm, T.NEAREST)
    assert np.array_equal(got64.reshape(Y.shape), Lm[Y, X].astype(np.float64))


# ---- the image form: the float32 twin alone against the float64 twin (the check the GPU image has to pass, and its camera) ----------------------
@pytest.mark.parametrize("N", GRIDS, ids=["N322", "N234"])
@pytest.mark.parametrize("nv,b", [(8, 0), (8, 1), (16, 0), (16, 1)], ids=["nv8_b0", "nv8_b1", "nv16_b0", "nv16_b1"])
def test_the_float32_image_form_stays_within_the_float64_twins_tolerance(N, nv, b):
    sc, ground = T.make_case(N, nv, b)
    ora = O.Oracle(sc.config())
    ora.set_frame(sc.light_to_world, sc.grid_center)
    ora.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    ora.set_occluders([ground])
    sc.light_depth_map = ora.render_light_depth()
    ora.fill(sc.fill_params())
    Lm, cam = ora.read_lightmap(), sc.camera()
    depth = ora.render_scene_depth(cam)
    ora.close()
    W, H = sc.width, sc.height
    assert (W, H) == (70, 45)
    g32 = consts(sc, F)
    for filt in (T.NEAREST, T.BILINEAR):
        for strength in (1.0, 0.37):
            img = T.image(cam, W, H, depth, g32, Lm, filt, strength)
            st = T.check_image_against_float64(img, cam, W, H, depth, sc, Lm, filt, strength)
            print(f"N={N} nv={nv} b={b} filter={filt} strength={strength}: {st}")
            assert st["below_one"] > 20 and st["inside"] > 100 and 0.5 * W * H < st["hit"] < W * H      # shadow, ground and sky are in view
            assert st["tol"] < 1e-2 * st["step"]                                          # the tolerance is far below one texel's step


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_headers_new_prototypes_are_exported_and_the_struct_is_16_bytes():
    hdr = open(os.path.join(ROOT, "include", "vpfx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(vp_volume_shadow_\w+|vp_apply_shadow\w*)\s*\(", code))
    assert names == {"vp_volume_shadow_points", "vp_volume_shadow_points_device", "vp_volume_shadow_image", "vp_volume_shadow_image_device",
                     "vp_apply_shadow_device"}
    assert names <= set(abi.EXPORTED_SYMBOLS)
    assert C.sizeof(abi.vp_shadow_params) == 16
    assert [f for f, _ in abi.vp_shadow_params._fields_] == ["filter", "strength", "reserved"]
    assert (abi.VP_SHADOW_NEAREST, abi.VP_SHADOW_BILINEAR) == (0, 1)
    assert re.search(r"#define\s+VP_SHADOW_NEAREST\s+0\b", code) and re.search(r"#define\s+VP_SHADOW_BILINEAR\s+1\b", code)
    assert "ABI 6 (additive): volume shadows" in hdr
