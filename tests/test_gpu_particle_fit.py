"""GPU: where the resident particles are and what the bin kept of them -- `vp_particle_bounds` against the float32 twin of
tests/bounds_twin.py (all 13 floats with ==: minimum and maximum are exact and order-free), `vp_particle_coverage` against counts rebuilt
from the bin's own lists, and the whole loop bounds -> `vp_fit_grid` -> `vp_set_frame` on a cloud the host never sees."""
import ctypes as C

import numpy as np
import pytest
import torch

import bounds_twin as B
from vpfx_amd import abi, engine as E, scene as S
from vpfx_amd.manager import MetavoxelManager

pytestmark = pytest.mark.gpu
F = np.float32
IDENT = S.to_colmajor16(np.eye(4))
MOVED = S.to_colmajor16(S.trs((1.25, -0.75, 2.5), S.quat_to_matrix((0.0, 0.38268343, 0.0, 0.92387953))))     # 45 degrees about y + a shift
SIZES = [1, 63, 64, 65, 257, 100003]          # one lane, the wave edge, the workgroup edge, many workgroups with a tail


def to_device(records: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(records.tobytes(), dtype=np.uint8).copy()).cuda()


def cloud(P, seed, shift=(0.0, 0.0, 0.0)):
    """P records of the 84-byte layout: positions in a 20-unit cube about `shift`, sizes 0.5 .. 1 with every fifth one negative."""
    rng = np.random.default_rng(seed)
    p = np.zeros(P, dtype=S.PARTICLE_DTYPE)
    p["position"] = (rng.uniform(-10.0, 10.0, (P, 3)) + np.asarray(shift)).astype(F)
    p["size"] = rng.uniform(0.5, 1.0, P).astype(F)
    p["size"][::5] *= F(-1.0)
    p["rotation"] = rng.uniform(0.0, 360.0, P).astype(F)
    p["lifetime"], p["startLifetime"] = 3.0, 6.0
    return p


def repacked(p):
    """The same particles as 37-byte records with unaligned field offsets and the rotation in radians."""
    lay = abi.vp_particle_layout()
    lay.stride, lay.off_position, lay.off_size, lay.off_rotation, lay.off_lifetime, lay.off_start_lifetime = 37, 1, 13, 18, 23, 31
    lay.rotation_in_radians = 1
    rec = np.full((len(p), 37), 0xCD, dtype=np.uint8)

    def put(off, v):
        b = np.ascontiguousarray(v, dtype="<f4").reshape(len(p), -1).view(np.uint8)
        rec[:, off:off + b.shape[1]] = b
    put(1, p["position"]); put(13, p["size"]); put(18, np.radians(p["rotation"].astype(np.float64)).astype(F))
    put(23, p["lifetime"]); put(31, p["startLifetime"])
    return rec.reshape(-1).view("V37"), lay


def frames(sc):
    return {"world": None, "camera": np.array(list(sc.camera().world_to_camera), dtype=F), "light": E.rigid_inverse(sc.light_to_world)}


@pytest.fixture(scope="module")
def sc():
    return S.make_scene("T0")


@pytest.fixture(scope="module")
def eng(sc):
    e = E.Engine(sc.config(device=0))
    e.set_frame(sc.light_to_world, sc.grid_center)
    yield e
    e.close()


def check_all_frames(eng, sc, ws):
    for name, m in frames(sc).items():
        got = eng.particle_bounds(m)
        B.assert_bounds_equal(got, B.bounds(ws, m))
        assert got["counted"] + got["skipped"] == len(ws), name


# ---- 1. bounds against the twin -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
def test_bounds_equal_the_twin(eng, sc, P):
    p = cloud(P, seed=P)
    lay84 = S.particle_layout()
    # host upload, 84-byte layout, identity system
    eng.upload_particles(p, lay84, IDENT)
    check_all_frames(eng, sc, B.world_particles(p["position"], p["size"], IDENT))
    # host upload, packed 37-byte radians layout, moved system
    rec37, lay37 = repacked(p)
    eng.upload_particles(rec37, lay37, MOVED)
    ws_moved = B.world_particles(p["position"], p["size"], MOVED)
    check_all_frames(eng, sc, ws_moved)
    # device upload of both layouts
    d84, d37 = to_device(p), to_device(rec37)
    torch.cuda.synchronize()
    eng.upload_particles_device(d84.data_ptr(), P, lay84, MOVED)
    check_all_frames(eng, sc, ws_moved)
    eng.upload_particles_device(d37.data_ptr(), P, lay37, IDENT)
    check_all_frames(eng, sc, B.world_particles(p["position"], p["size"], IDENT))
    got = eng.particle_bounds()
    assert got["counted"] == P and got["skipped"] == 0 and got["max_radius"] > 0
    assert np.all(got["sphere_min"] < got["center_min"]) and np.all(got["sphere_max"] > got["center_max"])


@pytest.mark.parametrize("moved", [False, True], ids=["identity_system", "moved_system"])
def test_bounds_of_the_device_emitter_equal_the_twin(eng, sc, moved):
    l2w = MOVED if moved else IDENT
    em = S.DeviceEmitter(eng, seed=11, rate=4000.0, lifetime=2.0, max_particles=5000)
    for _ in range(45):
        n = em.step(1 / 30)
    assert n > 4000
    eng.upload_particles_from_emitter(em, l2w)
    rec = em.particles()                                  # the parity probe, for the twin only
    check_all_frames(eng, sc, B.world_particles(rec["position"], rec["size"], l2w))
    em.close()


# ---- 2. reduction edges ---------------------------------------------------------------------------------------------------------------------
def canonical_layout():
    lay = abi.vp_particle_layout()
    lay.stride, lay.off_position, lay.off_size, lay.off_rotation, lay.off_lifetime, lay.off_start_lifetime = 32, 0, 12, 16, 20, 24
    return lay


@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), (-100.0, -50.0, -30.0)], ids=["mixed_signs", "all_negative"])
def test_every_extreme_from_every_place_in_the_grid_stride(eng, sc, centre):
    """The particle that sets each of the 13 values sits at index 0, 63, 64, 255, 256 and P - 1 in turn; everybody else is strictly inside."""
    P = 100003
    base = cloud(P, seed=5, shift=centre)
    rec = np.zeros((P, 8), dtype=F)
    rec[:, :3], rec[:, 3], rec[:, 5], rec[:, 6] = base["position"], base["size"], 3.0, 6.0
    d = torch.from_numpy(rec).cuda()
    lay = canonical_layout()
    c = np.asarray(centre, dtype=F)
    plants = []                                           # (field, axis, position, size, the value it must produce)
    for k in range(3):
        e = np.zeros(3, dtype=F); e[k] = 1
        plants += [("center_min", k, c - F(10.25) * e, F(0.0625), c[k] - F(10.25)), ("center_max", k, c + F(10.25) * e, F(0.0625), c[k] + F(10.25)),
                   ("sphere_min", k, c - F(9.5) * e, F(4.0), c[k] - F(11.5)), ("sphere_max", k, c + F(9.5) * e, F(-4.0), c[k] + F(11.5))]
    plants.append(("max_radius", None, c, F(-2.5), F(1.25)))
    if centre[0] < 0:
        assert np.all(base["position"] + np.abs(base["size"])[:, None] < 0)         # every coordinate of every box corner is negative
    for idx in (0, 63, 64, 255, 256, P - 1):
        for field, k, pos, size, value in plants:
            keep = rec[idx].copy()
            rec[idx, :3], rec[idx, 3] = pos, size
            d[idx] = torch.from_numpy(rec[idx]).cuda()
            torch.cuda.synchronize()
            eng.upload_particles_device(d.data_ptr(), P, lay, IDENT)
            got = eng.particle_bounds()
            B.assert_bounds_equal(got, B.bounds(rec[:, :4]))
            assert (got[field] if k is None else got[field][k]) == value, (idx, field, k)
            rec[idx] = keep
            d[idx] = torch.from_numpy(keep).cuda()
    torch.cuda.synchronize()


def test_result_words_are_reinitialised_and_an_empty_upload_is_valid(eng, sc):
    big, small = cloud(5000, seed=1), cloud(300, seed=2)
    small["position"] *= F(0.25)
    lay = S.particle_layout()
    eng.upload_particles(big, lay, IDENT)
    b_big = eng.particle_bounds()
    eng.upload_particles(small, lay, IDENT)
    b_small = eng.particle_bounds()
    B.assert_bounds_equal(b_small, B.bounds(B.world_particles(small["position"], small["size"], IDENT)))
    assert np.all(b_small["sphere_min"] > b_big["sphere_min"]) and np.all(b_small["sphere_max"] < b_big["sphere_max"]) and b_small["counted"] == 300
    B.assert_bounds_equal(eng.particle_bounds(), b_small)                           # and a second call gives the same
    eng.upload_particles(small[:0], lay, IDENT)                                     # P = 0
    for m in frames(sc).values():
        e = eng.particle_bounds(m)
        B.assert_bounds_equal(e, B.bounds(np.zeros((0, 4), dtype=F)))
        assert e["counted"] == e["skipped"] == 0 and e["max_radius"] == 0
        assert np.all(np.isposinf(e["center_min"])) and np.all(np.isposinf(e["sphere_min"]))
        assert np.all(np.isneginf(e["center_max"])) and np.all(np.isneginf(e["sphere_max"]))


# ---- 3. skipping, and the reference's box ----------------------------------------------------------------------------------------------------
def test_non_finite_particles_are_skipped_as_the_bin_skips_them(eng, sc):
    p = cloud(1000, seed=9)
    bad = {0: ("position", 0, np.nan), 63: ("position", 1, np.inf), 64: ("position", 2, -np.inf), 255: ("size", None, np.nan),
           256: ("size", None, np.inf), 640: ("size", None, -np.inf), 999: ("position", 0, -np.inf)}
    for i, (f, k, v) in bad.items():
        if k is None:
            p[f][i] = v
        else:
            p[f][i, k] = v
    lay = S.particle_layout()
    eng.upload_particles(p, lay, IDENT)
    clean = np.delete(p, list(bad))
    for name, m in frames(sc).items():
        got = eng.particle_bounds(m)
        B.assert_bounds_equal(got, B.bounds(B.world_particles(p["position"], p["size"], IDENT), m))
        assert (got["counted"], got["skipped"]) == (993, 7)
        want = B.bounds(B.world_particles(clean["position"], clean["size"], IDENT), m)
        want["skipped"] = 7
        B.assert_bounds_equal(got, want)                                              # the boxes of the cloud without them
    # the bin skips the same seven
    eng.bin_resident()
    cov = eng.particle_coverage(per_particle=True)
    assert cov["skipped"] == 7 and not cov["mv_per_particle"][list(bad)].any()
    # only skipped particles: the empty result
    eng.upload_particles(p[[0, 255]], lay, IDENT)
    e = eng.particle_bounds()
    assert (e["counted"], e["skipped"]) == (0, 2) and np.all(np.isposinf(e["sphere_min"])) and np.all(np.isneginf(e["center_max"])) and e["max_radius"] == 0


def test_particle_aabb_is_the_references_loop():
    """AABBForParticles.FindAABB (AABBForParticles.cs:26-62), restated literally in float32."""
    sc = S.make_scene("T1")
    m = MetavoxelManager(numMetavoxelsX=6, numMetavoxelsY=6, numMetavoxelsZ=6, numVoxelsInMetavoxel=32, screenWidth=160, screenHeight=120, device=0)
    m.Start()
    m.SetLight(sc.light_to_world)
    m.psysLocalToWorld = MOVED
    m.BinParticlesToMetavoxels(sc.particles, sc.layout)
    cam = sc.camera()
    centre, size = m.ParticleAABB(cam)
    l2w, w2c = B.rows_of(MOVED), B.rows_of(list(cam.world_to_camera))

    def mul_point_3x4(mat, v):                             # Matrix4x4.MultiplyPoint3x4
        return np.array([((mat[r, 0] * v[0] + mat[r, 1] * v[1]) + mat[r, 2] * v[2]) + mat[r, 3] for r in range(3)], dtype=F)
    mx = mn = None
    for rec in sc.particles:
        cs = mul_point_3x4(w2c, mul_point_3x4(l2w, rec["position"]))                  # :37-40
        radius = rec["size"] * F(0.5)                                                 # :42
        r3 = np.array([radius, radius, -radius], dtype=F)
        cs_max, cs_min = cs + r3, cs - r3                                             # :43-44
        if mx is None:
            mx, mn = cs_max, cs_min                                                   # :46-51
        else:
            mx = np.array([max(cs_max[0], mx[0]), max(cs_max[1], mx[1]), min(cs_max[2], mx[2])], dtype=F)     # :54
            mn = np.array([min(cs_min[0], mn[0]), min(cs_min[1], mn[1]), max(cs_min[2], mn[2])], dtype=F)     # :55
    assert centre.dtype == F and size.dtype == F
    assert np.array_equal(centre, (mx + mn) / F(2.0)) and np.array_equal(size, mx - mn)                       # :60
    assert size[0] > 0 and size[1] > 0 and size[2] < 0                                # camera space looks down -z
    m.OnDestroy()


# ---- 4. coverage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["T1", "N6_small", "N5", "T1_slab_2_4"])
def test_coverage_equals_counts_rebuilt_from_the_bin_lists(which):
    slab = (0, 0)
    if which == "N6_small":
        sc = S.make_scene("T1", size_range=(0.1, 0.3))
    elif which == "N5":
        sc = S.make_scene(dims=(5, 16, 400, 96, 64))
    else:
        sc = S.make_scene("T1")
        slab = (2, 4) if which.endswith("slab_2_4") else slab
    eng = E.Engine(sc.config(device=0, slab=slab))
    eng.set_frame(sc.light_to_world, sc.grid_center)
    eng.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    lists, counts = B.lists_of(eng)
    if slab != (0, 0):
        assert not counts[:2].any() and not counts[4:].any() and counts[2:4].any()   # only the owned slab's lists count
    want, per = B.coverage(len(sc.particles), lists, np.ones(len(sc.particles), dtype=bool))
    got = eng.particle_coverage(per_particle=True)
    assert np.array_equal(got.pop("mv_per_particle"), per)
    assert got == want, (got, want)
    assert got["pairs"] == eng.stats()["pairs"] == int(counts.sum())
    assert got["covered"] + got["uncovered"] + got["skipped"] == got["particles"] == 400
    assert eng.particle_coverage() == got                                             # without the per-particle array, and repeatable
    print(f"{which}: {got}")
    if which == "N6_small":
        assert got["uncovered"] > 0                       # reference quirks Q1 / Q2: dropped on a grid that contains them
        b = eng.particle_bounds(E.rigid_inverse(sc.light_to_world))
        fit = E.fit_grid(sc.light_to_world, b["sphere_min"], b["sphere_max"], sc.N, sc.mv_scale, 0.0)
        assert fit["min_mv_scale"] < sc.mv_scale          # (the cloud is smaller than the grid)
    assert got["covered"] > 0 and got["max_mv_per_particle"] >= 1
    eng.close()


# ---- 5. end to end: a cloud the host never sees ----------------------------------------------------------------------------------------------
def test_a_drifted_device_cloud_is_found_fitted_and_rendered():
    sc, host_em, _ = S.make_demo_scene(width=160, height=120)                        # N = 10, s = 3, emitter size 4: Q1 / Q2 cannot drop anything
    host_em.close()
    drift = np.array([100.0, 40.0, -60.0])
    psys = B.rows_of(sc.psys_local_to_world).astype(np.float64)
    psys[:3, 3] += drift
    sc.cam_to_world = sc.cam_to_world.copy()
    sc.cam_to_world[:3, 3] += drift
    sc.world_to_cam, sc.cam_pos = np.linalg.inv(sc.cam_to_world), (sc.cam_pos + drift).astype(F)
    psys16 = S.to_colmajor16(psys)
    eng = E.Engine(sc.config(device=0))
    em = S.DeviceEmitter(eng, seed=7, prewarm=True)
    n = em.step(1 / 30)
    eng.set_frame(sc.light_to_world, sc.grid_center)
    eng.upload_particles_from_emitter(em, psys16)
    eng.bin_resident()
    counted = eng.particle_bounds()["counted"]
    cov = eng.particle_coverage()
    assert counted == n == cov["particles"] and cov["uncovered"] == counted and cov["covered"] == 0 and cov["pairs"] == 0
    eng.fill(sc.fill_params())
    assert not eng.raymarch(sc.camera(), sc.raymarch_params())[..., 3].any()          # unfitted: the image is empty
    voxel = sc.mv_scale / (sc.nv - 2 * sc.border)
    fit = eng.fit_grid_to_particles(sc.light_to_world, snap=voxel)
    assert fit["fits"] == 1 and np.linalg.norm(fit["grid_center"] - (sc.grid_center + drift)) < 15.0
    q = fit["ls_center"].astype(np.float64) / float(F(voxel))
    assert np.all(np.abs(q - np.rint(q)) < 1e-3)                                      # snapped to the voxel lattice in light space
    eng.set_frame(sc.light_to_world, fit["grid_center"])
    eng.bin_resident()
    cov = eng.particle_coverage()
    assert cov["uncovered"] == 0 and cov["covered"] == counted and cov["pairs"] == eng.stats()["pairs"] > 0
    eng.fill(sc.fill_params())
    img = eng.raymarch(sc.camera(), sc.raymarch_params())
    assert (img[..., 3] > 0).any()
    em.close(); eng.close()


# ---- 6. no side effects ----------------------------------------------------------------------------------------------------------------------
def test_the_queries_change_nothing_the_frame_computes():
    sc = S.make_scene("T1")
    a, b = E.Engine(sc.config(device=0)), E.Engine(sc.config(device=0))
    light_frame = E.rigid_inverse(sc.light_to_world)
    for e in (a, b):
        e.set_frame(sc.light_to_world, sc.grid_center)
        e.upload_particles(sc.particles, sc.layout, sc.psys_local_to_world)
    first = a.particle_bounds(light_frame)                                            # after the upload
    a.fit_grid_to_particles(sc.light_to_world, snap=0.1)
    for e in (a, b):
        e.bin_resident()
    a.particle_bounds()
    cov = a.particle_coverage(per_particle=True)                                      # after the bin
    for e in (a, b):
        e.fill(sc.fill_params())
    B.assert_bounds_equal(a.particle_bounds(light_frame), first)                      # after the fill
    assert a.particle_coverage()["covered"] == cov["covered"]
    img_a, img_b = (e.raymarch(sc.camera(), sc.raymarch_params()) for e in (a, b))
    a.particle_coverage()
    ca, cb = a.bin_counts(), b.bin_counts()
    assert np.array_equal(ca, cb) and ca.any()
    for zz, yy, xx in np.argwhere(ca > 0):
        assert np.array_equal(a.bin_list(xx, yy, zz), b.bin_list(xx, yy, zz)), (xx, yy, zz)
        assert a.read_brick(xx, yy, zz).tobytes() == b.read_brick(xx, yy, zz).tobytes(), (xx, yy, zz)
    assert img_a.tobytes() == img_b.tobytes() and (img_a[..., 3] > 0.01).any()
    a.close(); b.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_results_in_effect():
    L = E.lib()
    sc = S.make_scene("T0")
    eng = E.Engine(sc.config(device=0))
    out_b, out_c = abi.vp_particle_bounds(), abi.vp_particle_coverage()
    out_b.counted = out_c.covered = 77
    # before an upload / before a bin
    assert L.vp_particle_bounds(eng.h, None, C.byref(out_b)) == abi.VP_ERR_STATE
    assert L.vp_particle_coverage(eng.h, C.byref(out_c), None) == abi.VP_ERR_STATE
    eng.set_frame(sc.light_to_world, sc.grid_center)
    eng.upload_particles(sc.particles, sc.layout, sc.psys_local_to_world)
    assert L.vp_particle_coverage(eng.h, C.byref(out_c), None) == abi.VP_ERR_STATE   # uploaded, not binned
    assert out_b.counted == 77 and out_c.covered == 77                                # a refused call writes nothing
    good = eng.particle_bounds()
    eng.bin_resident()
    good_cov = eng.particle_coverage()
    # frames that are not rigid, and null outputs
    scaled = np.array(IDENT, dtype=F); scaled[0] = F(1.01)
    sheared = np.array(IDENT, dtype=F); sheared[4] = F(0.01)
    affine = np.array(IDENT, dtype=F); affine[3] = F(0.25)
    nan = np.array(IDENT, dtype=F); nan[12] = np.nan
    for bad in (scaled, sheared, affine, nan):
        with pytest.raises(E.VpfxError) as ei:
            eng.particle_bounds(bad)
        assert ei.value.code == abi.VP_ERR_BAD_ARG
        B.assert_bounds_equal(eng.particle_bounds(), good)
    assert L.vp_particle_bounds(eng.h, None, None) == abi.VP_ERR_BAD_ARG
    assert L.vp_particle_coverage(eng.h, None, None) == abi.VP_ERR_BAD_ARG
    assert L.vp_particle_bounds(None, None, C.byref(out_b)) == abi.VP_ERR_BAD_ARG
    B.assert_bounds_equal(eng.particle_bounds(), good)
    assert eng.particle_coverage() == good_cov
    assert np.array_equal(eng.bin_counts().sum(), good_cov["pairs"])                  # and the bins are still the bins
    # a new upload invalidates the bins: coverage waits for the next bin, bounds does not
    eng.upload_particles(sc.particles[:50], sc.layout, sc.psys_local_to_world)
    with pytest.raises(E.VpfxError) as ei:
        eng.particle_coverage()
    assert ei.value.code == abi.VP_ERR_STATE
    assert eng.particle_bounds()["counted"] == 50
    eng.close()


def test_fanout_contexts_do_not_take_the_queries():
    sc = S.make_scene("T1")
    fan = E.Engine(sc.config(devices=[0, 0], multi_flags=abi.VP_MULTI_PEER_COPY))
    fan.set_frame(sc.light_to_world, sc.grid_center)
    fan.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    before = fan.bin_counts()
    for call in (fan.particle_bounds, fan.particle_coverage, lambda: fan.fit_grid_to_particles(sc.light_to_world)):
        with pytest.raises(E.VpfxError) as ei:
            call()
        assert ei.value.code == abi.VP_ERR_UNSUPPORTED
    assert np.array_equal(fan.bin_counts(), before) and before.any()
    fan.close()
