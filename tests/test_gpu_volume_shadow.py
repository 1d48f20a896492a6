"""GPU: volume shadows (include/vpfx.h "volume shadows", csrc/volume_shadow.hip) -- the light-propagation map of the last fill projected onto
world points and onto the pixels of the scene's eye depth.

The input map is always the GPU's own read_lightmap(): the fill is not re-tested here.  The points form is held to the float32 twin of
tests/shadow_twin.py bit for bit; the image form to the float64 twin within (largest step between adjacent texels of the map) x (coordinate
error bound in texels), both derived in shadow_twin.check_image_against_float64; tests/test_volume_shadow_cpu.py proves the twin itself.

test_the_image_form_against_the_float64_twin also prints, without asserting it, how many pixels differ from the float32 twin at all
(measured on an MI355X: 0 of 3150 in each of the 32 grid x nv x border x filter x strength combinations)."""
import ctypes as C

import numpy as np
import pytest
import torch

import shadow_twin as T
from vpfx_amd import abi, engine as E
from vpfx_amd.manager import MetavoxelManager

pytestmark = pytest.mark.gpu
F = np.float32
GRIDS = [(3, 2, 2), (2, 3, 4)]
CASES = [(N, nv, b) for N in GRIDS for nv in (8, 16) for b in (0, 1)]
IDS = [f"N{N[0]}{N[1]}{N[2]}_nv{nv}_b{b}" for N, nv, b in CASES]
FILTERS = (abi.VP_SHADOW_NEAREST, abi.VP_SHADOW_BILINEAR)
SENTINEL = F(-7.25)


class Case:
    """One filled engine (ground box set, light depth map rendered inside vp_fill), its own light map, and the twin's constants."""

    def __init__(self, N, nv, b):
        self.sc, self.ground = T.make_case(N, nv, b)
        sc = self.sc
        self.eng = E.Engine(sc.config(device=0))
        self.eng.set_occluders2([self.ground])
        self.eng.set_frame(sc.light_to_world, sc.grid_center)
        self.eng.bin(sc.particles, sc.layout, sc.psys_local_to_world)
        self.eng.fill(sc.fill_params())
        self.Lm = self.eng.read_lightmap()
        self.g32 = T.grid_consts(sc.N, sc.nv, sc.border, sc.mv_scale, sc.light_to_world, sc.grid_center, F)
        self.cam = sc.camera()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(N, nv, b):
        if (N, nv, b) not in made:
            made[(N, nv, b)] = Case(N, nv, b)
        return made[(N, nv, b)]
    yield get
    for c in made.values():
        c.eng.close()


# ---- 1. voxel-column centres ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nv,b", CASES, ids=IDS)
def test_nearest_at_every_voxel_column_centre_is_the_light_map_texel(cases, N, nv, b):
    c = cases(N, nv, b)
    assert c.Lm.min() < 0.9 and len(np.unique(c.Lm)) > 20                                 # the cloud and the ground left their mark
    for zz, z_local in ((0, 0.3), (N[2] - 1, -0.25)):
        world, Y, X = T.column_centres(c.eng.mv_positions(), c.sc.light_to_world, nv, b, c.sc.mv_scale, zz=zz, z_local=z_local)
        got = c.eng.volume_shadow_points(world.reshape(-1, 3), abi.VP_SHADOW_NEAREST, 1.0)
        assert got.tobytes() == np.ascontiguousarray(c.Lm[Y, X]).tobytes()
    assert Y.shape == (N[1], N[0], nv - 2 * b, nv - 2 * b)                                 # every interior column of every metavoxel


# ---- 2. random points against the float32 twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nv,b", CASES, ids=IDS)
def test_random_points_equal_the_float32_twin_bit_for_bit(cases, N, nv, b):
    c = cases(N, nv, b)
    sc = c.sc
    g64 = T.grid_consts(sc.N, sc.nv, sc.border, sc.mv_scale, sc.light_to_world, sc.grid_center, np.float64)
    n, s = np.array(N), sc.mv_scale
    lo = g64["lsO"] - (n // 2 + 0.5) * s
    mid, half = lo + n * s / 2.0, n * s / 2.0
    rng = np.random.default_rng(11)
    ls = mid + rng.uniform(-1.5, 1.5, (4096, 3)) * half                                   # a box 1.5 x the grid, about its middle
    L = T.rows_of(sc.light_to_world).astype(np.float64)
    p = (ls @ L[:3, :3].T + L[:3, 3]).astype(F)
    bad = p[:8].copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4, 1], bad[5, 2], bad[6], bad[7] = np.nan, np.inf, -np.inf, -np.inf, np.nan, np.inf, np.nan, np.inf
    p = np.concatenate([p, bad])
    inside = 0
    for filt in FILTERS:
        for strength in (1.0, 0.37):
            got = c.eng.volume_shadow_points(p, filt, strength)
            want = T.factor(p, c.g32, c.Lm, filt, strength)
            assert want.dtype == F and got.tobytes() == want.tobytes(), (filt, strength, int((got != want).sum()))
            assert np.all(got[-8:] == 1.0)
            inside = int((got < 1.0).sum())
    assert 50 < inside < 4000                                                              # points in the shadow and points outside the grid


# ---- 3. the image form ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nv,b", CASES, ids=IDS)
def test_the_image_form_against_the_float64_twin(cases, N, nv, b):
    c = cases(N, nv, b)
    sc, W, H = c.sc, c.sc.width, c.sc.height
    assert (W, H) == (70, 45)
    depth = c.eng.render_scene_depth(c.cam)
    for filt in FILTERS:
        for strength in (1.0, 0.37):
            img = c.eng.volume_shadow_image(c.cam, depth, filt, strength)
            img_null = c.eng.volume_shadow_image(c.cam, None, filt, strength)              # the depth the library renders itself
            assert img.tobytes() == img_null.tobytes()
            st = T.check_image_against_float64(img, c.cam, W, H, depth, sc, c.Lm, filt, strength)
            differ = int((img != T.image(c.cam, W, H, depth, c.g32, c.Lm, filt, strength)).sum())
            print(f"N={N} nv={nv} b={b} filter={filt} strength={strength}: {st}; pixels that differ from the float32 twin: {differ} of {W * H}")
            assert st["below_one"] >= 1 and st["hit"] < W * H                              # a pixel under the cloud is darkened; there is sky
            under = (depth < 3e38) & (img < 1.0)
            assert under.any() and np.all(img[depth >= 3e38] == 1.0)
    # no occluders at all: 1.0 everywhere
    c.eng.set_occluders2([])
    assert np.all(c.eng.volume_shadow_image(c.cam, None, abi.VP_SHADOW_BILINEAR, 1.0) == 1.0)
    c.eng.set_occluders2([c.ground])


# ---- 4. device forms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nv,b", [CASES[1], CASES[6]], ids=[IDS[1], IDS[6]])
def test_device_forms_equal_the_host_forms_and_apply_equals_numpy(cases, N, nv, b):
    c = cases(N, nv, b)
    W, H = c.sc.width, c.sc.height
    world, _, _ = T.column_centres(c.eng.mv_positions(), c.sc.light_to_world, nv, b, c.sc.mv_scale, zz=0, z_local=0.1)
    rng = np.random.default_rng(3)
    p = np.ascontiguousarray((world.reshape(-1, 3) + rng.uniform(-2.0, 2.0, (world.size // 3, 3))).astype(F))
    depth = c.eng.render_scene_depth(c.cam)
    d_p, d_depth = torch.from_numpy(p).cuda(), torch.from_numpy(depth).cuda()
    for filt in FILTERS:
        d_out = torch.full((len(p),), float(SENTINEL), dtype=torch.float32, device="cuda")
        d_img = torch.full((H, W), float(SENTINEL), dtype=torch.float32, device="cuda")
        d_img_null = torch.full((H, W), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        c.eng.volume_shadow_points_device(d_p.data_ptr(), len(p), d_out.data_ptr(), filt, 0.8)
        c.eng.volume_shadow_image_device(c.cam, d_depth.data_ptr(), d_img.data_ptr(), filt, 0.8)
        c.eng.volume_shadow_image_device(c.cam, None, d_img_null.data_ptr(), filt, 0.8)
        c.eng.sync()
        assert d_out.cpu().numpy().tobytes() == c.eng.volume_shadow_points(p, filt, 0.8).tobytes()
        host = c.eng.volume_shadow_image(c.cam, depth, filt, 0.8)
        assert d_img.cpu().numpy().tobytes() == host.tobytes() == d_img_null.cpu().numpy().tobytes()
    # apply: scene.rgb *= shadow, alpha untouched
    scene = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F)
    d_scene = torch.from_numpy(scene).cuda()
    torch.cuda.synchronize()
    c.eng.apply_shadow_device(d_img.data_ptr(), d_scene.data_ptr())
    c.eng.sync()
    want = scene.copy()
    want[..., :3] = scene[..., :3] * host[..., None]
    assert d_scene.cpu().numpy().tobytes() == want.tobytes()
    assert (host < 1.0).any()


# ---- 5. the map follows the fill -------------------------------------------------------------------------------------------------------------------
def test_the_shadow_follows_a_refill_and_the_per_metavoxel_fill_gives_the_same_image():
    N, nv, b = (2, 3, 4), 8, 1
    c = Case(N, nv, b)
    sc, eng = c.sc, c.eng
    img0 = eng.volume_shadow_image(c.cam, None, abi.VP_SHADOW_BILINEAR, 1.0)
    near0 = eng.volume_shadow_image(c.cam, None, abi.VP_SHADOW_NEAREST, 1.0)
    moved = sc.particles.copy()
    R = T.rows_of(sc.light_to_world).astype(np.float64)[:3, :3]
    moved["position"] = (moved["position"] + 1.5 * R[:, 0]).astype(F)                      # half a metavoxel along the light's x axis
    eng.bin(moved, sc.layout, sc.psys_local_to_world)
    eng.fill(sc.fill_params())
    Lm1 = eng.read_lightmap()
    img1 = eng.volume_shadow_image(c.cam, None, abi.VP_SHADOW_BILINEAR, 1.0)
    assert not np.array_equal(Lm1, c.Lm) and not np.array_equal(img1, img0)
    depth = eng.render_scene_depth(c.cam)
    T.check_image_against_float64(img1, c.cam, sc.width, sc.height, depth, sc, Lm1, T.BILINEAR, 1.0)       # it is the NEW map that is projected
    # nearest mode: each image is its own map's, and pixels changed only where geometry lies inside the grid
    near1 = eng.volume_shadow_image(c.cam, None, abi.VP_SHADOW_NEAREST, 1.0)
    T.check_image_against_float64(near0, c.cam, sc.width, sc.height, depth, sc, c.Lm, T.NEAREST, 1.0)
    T.check_image_against_float64(near1, c.cam, sc.width, sc.height, depth, sc, Lm1, T.NEAREST, 1.0)
    g64 = T.grid_consts(sc.N, sc.nv, sc.border, sc.mv_scale, sc.light_to_world, sc.grid_center, np.float64)
    _, hit, inside, _, _, _ = T.image(c.cam, sc.width, sc.height, depth, g64, Lm1, T.NEAREST, 1.0, details=True)
    changed = near0 != near1
    assert changed.any() and not changed[~hit].any() and changed[inside].sum() >= changed.sum() - 2
    # the per-metavoxel fill on the same bins: the same map (f32 cube map: bit for bit), hence the same image
    p = sc.fill_params()
    eng.fill_begin(p)
    with pytest.raises(E.VpfxError) as ei:                                                # begun, no metavoxel filled yet: nothing completed
        eng.volume_shadow_image(c.cam, None)
    assert ei.value.code == abi.VP_ERR_STATE
    counts = eng.bin_counts()
    for zz, yy, xx in np.argwhere(counts > 0):                                            # argwhere is zz-major
        eng.fill_metavoxel(xx, yy, zz)
    assert np.array_equal(eng.read_lightmap(), Lm1)
    assert eng.volume_shadow_image(c.cam, None, abi.VP_SHADOW_BILINEAR, 1.0).tobytes() == img1.tobytes()
    eng.close()


# ---- 6. the kept maps ---------------------------------------------------------------------------------------------------------------------------------
def test_a_callers_depth_does_not_touch_the_maps_the_raymarch_uses():
    c = Case((3, 2, 2), 16, 1)
    sc, eng = c.sc, c.eng
    rp = sc.raymarch_params()                                                             # scene_depth NULL: the eye depth rendered from the ground
    before = eng.raymarch(c.cam, rp)
    shadow_null = eng.volume_shadow_image(c.cam, None)
    wall = np.full((sc.height, sc.width), 2.0, dtype=F)                                   # a wall two units in front of the eye: hides the whole volume
    shadow_wall = eng.volume_shadow_image(c.cam, wall)
    assert not np.array_equal(shadow_wall, shadow_null)
    after = eng.raymarch(c.cam, rp)
    assert after.tobytes() == before.tobytes() and (before[..., 3] > 0).any()
    # ... and the wall WOULD have changed the ray-march, had it been picked up
    rp_wall = sc.raymarch_params()
    rp_wall.scene_depth = wall.ctypes.data_as(abi.c_float_p)
    walled = eng.raymarch(c.cam, rp_wall)
    assert not np.array_equal(walled, before)
    # the ray-march's own staging now holds the wall; a NULL-depth shadow call still means the rendered map
    assert eng.volume_shadow_image(c.cam, None).tobytes() == shadow_null.tobytes()
    assert eng.raymarch(c.cam, rp).tobytes() == before.tobytes()
    eng.close()


# ---- 7. the error table ----------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_error_table_and_a_refused_call_writes_nothing():
    L = E.lib()
    c = Case((3, 2, 2), 8, 1)
    sc, eng, cam = c.sc, c.eng, c.cam
    W, H = sc.width, sc.height
    pts = np.zeros((5, 3), dtype=F)
    out = np.full(5, SENTINEL, dtype=F)
    img = np.full((H, W), SENTINEL, dtype=F)
    depth = np.full((H, W), 10.0, dtype=F)
    d_pts, d_out = torch.from_numpy(pts).cuda(), torch.full((5,), float(SENTINEL), device="cuda")
    d_img, d_depth = torch.full((H, W), float(SENTINEL), device="cuda"), torch.from_numpy(depth).cuda()
    d_scene = torch.full((H, W, 4), float(SENTINEL), device="cuda")
    torch.cuda.synchronize()
    good = E.shadow_params()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                                            # noqa: E731

    def calls(h, sp, n=5, p_in=True, p_out=True, camera=True, forms="points image"):
        """The query entry points (points forms, image forms) with the given handle / params / count and optionally nulled pointers."""
        spp = C.byref(sp) if sp is not None else None
        camp = C.byref(cam) if camera else None
        rcs = []
        if "points" in forms:
            rcs += [L.vp_volume_shadow_points(h, vp(pts) if p_in else None, n, spp, vp(out) if p_out else None),
                    L.vp_volume_shadow_points_device(h, d_pts.data_ptr() if p_in else None, n, spp, d_out.data_ptr() if p_out else None)]
        if "image" in forms:
            rcs += [L.vp_volume_shadow_image(h, camp, vp(depth), spp, vp(img) if p_out else None),
                    L.vp_volume_shadow_image_device(h, camp, d_depth.data_ptr(), spp, d_img.data_ptr() if p_out else None)]
        return rcs

    def untouched():
        eng.sync()
        return (np.all(out == SENTINEL) and np.all(img == SENTINEL) and bool((d_out == float(SENTINEL)).all()) and bool((d_img == float(SENTINEL)).all())
                and bool((d_scene == float(SENTINEL)).all()))
    reference = eng.volume_shadow_image(cam, None)
    # VP_ERR_BAD_ARG
    assert calls(eng.h, None) == [abi.VP_ERR_BAD_ARG] * 4                                  # null params
    assert calls(None, good) == [abi.VP_ERR_BAD_ARG] * 4                                   # null context
    for filt in (2, -1, 7):
        assert calls(eng.h, E.shadow_params(filt, 1.0)) == [abi.VP_ERR_BAD_ARG] * 4
    for strength in (-0.01, 1.01, np.nan, np.inf, -np.inf):
        assert calls(eng.h, E.shadow_params(0, strength)) == [abi.VP_ERR_BAD_ARG] * 4
    for k in (0, 1):
        sp = E.shadow_params()
        sp.reserved[k] = 1
        assert calls(eng.h, sp) == [abi.VP_ERR_BAD_ARG] * 4
    assert calls(eng.h, good, n=-1, forms="points") == [abi.VP_ERR_BAD_ARG] * 2            # n < 0
    assert calls(eng.h, good, p_in=False, forms="points") == [abi.VP_ERR_BAD_ARG] * 2      # null points with n > 0
    assert calls(eng.h, good, p_out=False) == [abi.VP_ERR_BAD_ARG] * 4                     # null output
    assert calls(eng.h, good, camera=False, forms="image") == [abi.VP_ERR_BAD_ARG] * 2     # null camera
    assert L.vp_apply_shadow_device(eng.h, None, d_scene.data_ptr()) == abi.VP_ERR_BAD_ARG
    assert L.vp_apply_shadow_device(eng.h, d_img.data_ptr(), None) == abi.VP_ERR_BAD_ARG
    assert L.vp_apply_shadow_device(None, d_img.data_ptr(), d_scene.data_ptr()) == abi.VP_ERR_BAD_ARG
    # VP_ERR_UNSUPPORTED: n > 2^31 - 1 (refused before a byte is read)
    assert calls(eng.h, good, n=2 ** 31, forms="points") == [abi.VP_ERR_UNSUPPORTED] * 2
    assert untouched()
    # n = 0 is valid, with or without pointers, and writes nothing
    assert calls(eng.h, good, n=0, forms="points") == [abi.VP_OK] * 2
    assert calls(eng.h, good, n=0, p_in=False, p_out=False, forms="points") == [abi.VP_OK] * 2
    assert untouched()
    assert eng.volume_shadow_image(cam, None).tobytes() == reference.tobytes()             # and nothing changed
    # VP_ERR_STATE: no fill has completed (a new bin invalidates the last one)
    eng.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    assert calls(eng.h, good) == [abi.VP_ERR_STATE] * 4
    eng.fill_begin(sc.fill_params())
    assert calls(eng.h, good) == [abi.VP_ERR_STATE] * 4
    fresh = E.Engine(sc.config(device=0))
    assert calls(fresh.h, good) == [abi.VP_ERR_STATE] * 4
    fresh.close()
    # VP_ERR_UNSUPPORTED: a context that owns part of the light axis, and a fan-out context
    slab = E.Engine(sc.config(device=0, slab=(0, 1)))
    assert calls(slab.h, good) == [abi.VP_ERR_UNSUPPORTED] * 4
    slab.close()
    fan = E.Engine(sc.config(devices=[0, 0], multi_flags=abi.VP_MULTI_PEER_COPY))
    assert calls(fan.h, good) == [abi.VP_ERR_UNSUPPORTED] * 4
    assert L.vp_apply_shadow_device(fan.h, d_img.data_ptr(), d_scene.data_ptr()) == abi.VP_ERR_UNSUPPORTED
    fan.close()
    assert untouched()
    eng.close()


# ---- 8. the host mirror ----------------------------------------------------------------------------------------------------------------------------------
def test_the_manager_darkens_the_scene_under_the_cloud_only_with_the_switch_on():
    sc, ground = T.make_case((3, 2, 2), 16, 1)

    def frame(cast, strength=1.0):
        m = MetavoxelManager(numMetavoxelsX=3, numMetavoxelsY=2, numMetavoxelsZ=2, numVoxelsInMetavoxel=16, numBorderVoxels=1, mvScale=sc.mv_scale,
                             screenWidth=sc.width, screenHeight=sc.height, device=0)
        m.opacityFactor = sc.opacity_factor
        m.castVolumeShadows, m.shadowStrength = cast, strength
        m.Start()
        m.SetLight(sc.light_to_world)
        m.SetGridCenter(sc.grid_center)
        m.SetDisplacementTexture(sc.cubemap)
        m.SetOccluders([ground])
        rt = np.zeros((sc.height, sc.width, 4), dtype=F)
        m.OnPreRender(rt)
        rt[..., :3] = 0.5                                                                  # the opaque scene, drawn by the host
        particles = m.OnPostRender(0, sc.particles, sc.layout, sc.camera(), rt)
        shadow = m._engine.volume_shadow_image(sc.camera(), None, m.shadowFilter, strength)
        m.OnDestroy()
        return rt, particles, shadow
    off, p_off, shadow = frame(False)
    on, p_on, _ = frame(True)
    assert m_is_default_off()
    assert p_on.tobytes() == p_off.tobytes()                                               # the particles themselves do not change
    want = np.full_like(off, 0.0)
    want[..., :3] = p_on[..., :3] + (F(0.5) * shadow)[..., None] * (F(1.0) - p_on[..., 3:4])
    want[..., 3] = p_on[..., 3] + F(1.0)
    assert np.array_equal(on, want) and (shadow < 1.0).any()
    assert np.all(on[..., :3] <= off[..., :3]) and (on[..., :3] < off[..., :3]).any()
    half, _, shadow_half = frame(True, 0.5)
    assert np.all(half[..., :3] >= on[..., :3]) and np.all(shadow_half >= shadow)


def m_is_default_off():
    m = MetavoxelManager()
    return m.castVolumeShadows is False and m.shadowStrength == 1.0 and m.shadowFilter == abi.VP_SHADOW_BILINEAR
