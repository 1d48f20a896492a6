"""GPU: triangle-mesh occluders (vp_set_occluder_meshes / vp_set_occluder_instances) in both depth inputs -- against the analytic solids
they can reproduce exactly (a cube is a box), against the float64 reference ray caster of tests/mesh_reference.py, watertightness, culling,
the per-pixel minimum with the solids, whole frames, the kept-map cache, refusals, scale and the fan-out."""
import time

import numpy as np
import pytest

import mesh_reference as MR
from vpfx_amd import abi, engine as E, scene as S
from vpfx_amd.manager import MetavoxelManager

pytestmark = pytest.mark.gpu

CUBE = S.unity_cube_mesh()


def _light_frame(sc):
    L = np.asarray(sc.light_to_world, dtype=np.float64).reshape(4, 4).T
    return L[:3, :3]


def _engine(sc):
    e = E.Engine(sc.config())
    e.set_frame(sc.light_to_world, sc.grid_center)
    return e


def _maps(e, sc, cam=None):
    return e.render_light_depth(), e.render_scene_depth(cam if cam is not None else sc.camera())


def _meshes_engine(sc, meshes, instances):
    e = _engine(sc)
    e.set_occluder_meshes(meshes)
    e.set_occluder_instances(instances)
    return e


def _check_against(dl, de, rl, re_, exempt_l, exempt_e, min_hit=0.02):
    """GPU maps (dl, de) vs expected maps (rl, re_): hit / miss equal outside the exempt pixels, depths within 1e-6 (light, normalised) and
    rtol 1e-5 (eye) where both hit outside them."""
    hl, hr = dl < 1.0, rl < 1.0
    assert hr.mean() > min_hit, "the scene was meant to cover part of the light map"
    assert not ((hl != hr) & ~exempt_l).any(), np.argwhere((hl != hr) & ~exempt_l)[:5]
    both = hl & hr & ~exempt_l
    np.testing.assert_allclose(dl[both], rl[both], rtol=0, atol=1e-6)
    he, hr2 = de < 1e30, re_ < 1e30
    assert hr2.mean() > min_hit, "the scene was meant to cover part of the image"
    assert not ((he != hr2) & ~exempt_e).any(), np.argwhere((he != hr2) & ~exempt_e)[:5]
    both = he & hr2 & ~exempt_e
    np.testing.assert_allclose(de[both], re_[both], rtol=1e-5)


def _cube_boxes(sc):
    R = _light_frame(sc)
    q = S.quat_to_matrix((0.2, -0.1, 0.3, 0.927)).T
    return [S.make_box((-2.0, 1.0, -1.0), (1.0, 2.0, 1.5), q),                                 # rotated, scaled
            S.make_box(R[:, 2] * 2.0 + R[:, 0] * 3.0, (1.5, 2.0, 0.05), R.T),                   # thin, facing the light
            S.make_box((1.5, -1.5, 1.0), (0.7, 0.4, 1.1), S.quat_to_matrix((0.5, 0.5, -0.5, 0.5)).T),
            S.make_box((0.5, 2.5, -2.0), (0.8, 0.6, 0.5), S.quat_to_matrix((-0.3, 0.1, 0.2, 0.927)).T)]   # placed mirrored below


def _cube_instances(boxes):
    inst = []
    for i, b in enumerate(boxes):
        m = S.box_instance_matrix(b)
        if i == len(boxes) - 1:
            m = m @ np.diag([-1.0, 1.0, 1.0, 1.0])           # mirrored: det < 0, the same point set
            assert np.linalg.det(m[:3, :3]) < 0
        inst.append(S.make_instance(0, m))
    return inst


def test_mesh_cube_equals_the_analytic_box():
    sc = S.make_scene("T0")
    boxes = _cube_boxes(sc)
    es = _engine(sc)
    es.set_occluders(boxes)
    rl, re_ = _maps(es, sc)
    inst = _cube_instances(boxes)
    em = _meshes_engine(sc, [CUBE], inst)
    dl, de = _maps(em, sc)
    _, exl, _ = MR.render(MR.View.light(sc), [CUBE], inst)
    _, exe, _ = MR.render(MR.View.eye(sc, sc.camera()), [CUBE], inst)
    _check_against(dl, de, rl, re_, exl, exe)


@pytest.mark.parametrize("seed", [3, 11])
def test_meshes_match_the_float64_reference(seed):
    sc = S.make_scene("T0")
    rng = np.random.default_rng(seed)
    meshes = [S.torus_mesh(), S.icosphere_mesh(3), S.prism_mesh(20)]
    inst = []
    for k in range(9):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        m = S.trs(rng.uniform(-3.5, 3.5, 3), S.quat_to_matrix(q), rng.uniform(0.8, 3.0, 3) * rng.choice([-1.0, 1.0], 3))
        inst.append(S.make_instance(k % len(meshes), m))
    e = _meshes_engine(sc, meshes, inst)
    dl, de = _maps(e, sc)
    rl, exl, _ = MR.render(MR.View.light(sc), meshes, inst)
    re_, exe, _ = MR.render(MR.View.eye(sc, sc.camera()), meshes, inst)
    _check_against(dl, de, rl.astype(np.float32), re_.astype(np.float32), exl, exe)


def _tessellated_box(n):
    """A closed cube [-0.5, 0.5]^3 whose faces are n x n grids (12 n^2 triangles; vertices repeated along the cube's edges)."""
    p, t = S.grid_mesh(n, n)                                 # y = 0, facing +y
    pos, tri = [], []
    for R in (np.eye(3), np.diag([1.0, -1.0, -1.0]), S.quat_to_matrix((0.0, 0.0, 0.70710678, 0.70710678)), S.quat_to_matrix((0.0, 0.0, -0.70710678, 0.70710678)),
              S.quat_to_matrix((0.70710678, 0.0, 0.0, 0.70710678)), S.quat_to_matrix((-0.70710678, 0.0, 0.0, 0.70710678))):
        q = (p.astype(np.float64) + [0.0, 0.5, 0.0]) @ np.asarray(R).T
        tri.append(t + sum(len(x) for x in pos))
        pos.append(q)
    pos, tri = np.concatenate(pos).astype(np.float32), np.concatenate(tri).astype(np.int32)
    S._assert_outward(pos.astype(np.float64), tri, lambda c: np.zeros_like(c))
    return pos, tri


def test_closed_fine_meshes_are_watertight():
    sc = S.make_scene("T0", dims=(4, 32, 10, 192, 128))
    R = _light_frame(sc)
    LW = sc.N[0] * sc.nv
    pitch = sc.N[0] * sc.mv_scale / LW                        # one texel
    box = _tessellated_box(42)
    sphere = S.icosphere_mesh(5)
    assert len(box[1]) >= 20000 and len(sphere[1]) >= 20000
    # the box aligned with the light camera, its grid lines on texel-centre rays (vertex spacing = 1 texel, offset half a texel)
    origin = np.asarray(sc.grid_center, np.float64) + R[:, 0] * (-5.5 * pitch + 0.5 * pitch) + R[:, 1] * (8.0 * pitch + 0.5 * pitch)
    inst = [S.make_instance(0, S.trs(origin, R, (42 * pitch, 42 * pitch, 42 * pitch))),
            S.make_instance(1, S.trs((-2.5, -1.5, 1.0), S.quat_to_matrix((0.1, 0.3, 0.2, 0.927)), (4.1, 3.3, 3.7)))]
    meshes = [box, sphere]
    e = _meshes_engine(sc, meshes, inst)
    for view, got in ((MR.View.light(sc), e.render_light_depth()), (MR.View.eye(sc, sc.camera()), e.render_scene_depth(sc.camera()))):
        ref, _, near_sil = MR.render(view, meshes, inst)
        cleared = np.float32(1.0) if view.kind == "light" else np.float32(3e38)
        inside = (ref != cleared) & ~near_sil
        assert inside.sum() > 2000
        holes = inside & (got == cleared)
        assert not holes.any(), (view.kind, np.argwhere(holes)[:8])


def test_ground_plane_through_the_near_plane_has_no_hole():
    sc = S.make_scene("T0")
    sc.set_camera((-3.0, -4.0, -12.0), (0.0, -5.5, 0.0))
    cam = sc.camera()
    plane = S.grid_mesh(4, 4)
    e = _meshes_engine(sc, [plane], [S.make_instance(0, S.trs((0.0, -6.5, 0.0), np.eye(3), (200.0, 1.0, 200.0)))])
    de = e.render_scene_depth(cam)
    es = _engine(sc)
    es.set_occluders([S.make_box((0.0, -7.0, 0.0), (100.0, 0.5, 100.0))])
    ds = es.render_scene_depth(cam)
    assert (ds[0] < 1e30).all(), "the reference box was meant to fill the bottom row"
    assert (de[0] < 1e30).all(), "hole at the bottom of the screen"
    assert ((de < 1e30) == (ds < 1e30)).mean() > 0.999
    both = (de < 1e30) & (ds < 1e30)
    np.testing.assert_allclose(de[both], ds[both], rtol=1e-5)


def test_culling_follows_the_reference():
    sc = S.make_scene("T0")
    R = _light_frame(sc)
    fwd = R[:, 2] / np.linalg.norm(R[:, 2])
    quad = S.grid_mesh(1, 1)                                 # facing local +y
    # local +y -> -fwd: the quad faces the light; the camera looks at it from the light's side
    rot = np.stack([R[:, 0], -fwd, np.cross(R[:, 0], -fwd)], 1)
    m = S.trs((0.0, 0.0, 0.0), rot, (4.0, 1.0, 4.0))
    sc.set_camera(tuple(-fwd * 15.0 + R[:, 1] * 1.0), (0.0, 0.0, 0.0))
    flipped = (quad[0], quad[1][:, [0, 2, 1]].copy())
    for mesh, light_has, eye_has in ((quad, False, True), (flipped, True, False)):
        e = _meshes_engine(sc, [mesh], [S.make_instance(0, m)])
        dl, de = _maps(e, sc)
        assert ((dl < 1).any()) == light_has
        assert ((de < 1e30).any()) == eye_has
        if light_has:
            assert (dl < 1).mean() > 0.05
        if eye_has:
            assert (de < 1e30).mean() > 0.01


def test_solids_and_meshes_combine_by_a_minimum_bit_for_bit():
    sc = S.make_scene("T0")
    solids = [S.make_box((0.5, -0.5, 0.5), (1.5, 0.7, 1.0)), S.make_solid(abi.VP_OCC_ELLIPSOID, (-1.0, 1.0, 0.0), (1.2, 0.8, 1.0))]
    meshes = [S.torus_mesh(), CUBE]
    inst = [S.make_instance(0, S.trs((0.0, 0.5, 0.0), S.quat_to_matrix((0.3, 0.1, 0.0, 0.949)), (4.0, 4.0, 4.0))),
            S.make_instance(1, S.trs((1.5, 1.0, -1.0), np.eye(3), (1.0, 2.0, 1.0)))]
    es = _engine(sc)
    es.set_occluders(solids)
    em = _meshes_engine(sc, meshes, inst)
    eb = _meshes_engine(sc, meshes, inst)
    eb.set_occluders(solids)
    for a, b, both in zip(_maps(es, sc), _maps(em, sc), _maps(eb, sc)):
        assert np.array_equal(both, np.minimum(a, b))
        assert (both != a).any() and (both != b).any()


def _frame(e, sc, fill=True):
    e.set_frame(sc.light_to_world, sc.grid_center)
    if fill:
        e.bin(sc.particles, sc.layout, sc.psys_local_to_world)
        e.fill(sc.fill_params())
    return e.read_lightmap(), e.raymarch(sc.camera(), sc.raymarch_params())


def test_demo_boxes_as_mesh_cubes_give_the_same_frame():
    sc, em_, solids = S.make_demo_scene(width=256, height=192)
    boxes = [s for s in solids if s.type == abi.VP_OCC_BOX]
    others = [s for s in solids if s.type != abi.VP_OCC_BOX]
    assert len(boxes) == 4
    inst = [S.make_instance(0, S.box_instance_matrix(b)) for b in boxes]
    a = E.Engine(sc.config())
    a.set_occluders(solids)
    b = E.Engine(sc.config())
    b.set_occluders(others)
    b.set_occluder_meshes([CUBE])
    b.set_occluder_instances(inst)
    la, ia = _frame(a, sc)
    lb, ib = _frame(b, sc)
    np.testing.assert_allclose(lb, la, rtol=1e-5, atol=1e-9)
    bad = (np.abs(ia - ib).max(axis=-1) > 1e-3).sum()
    assert bad <= 3, bad
    assert ia[..., 3].max() > 0.05
    # the same through the host mirror's SyncOccluders
    frames = []
    for use_meshes in (False, True):
        m = MetavoxelManager(10, 10, 10, 3.0, 32, 1, sc.width, sc.height)
        m.Start()
        m.SetLight(sc.light_to_world)
        m.SetGridCenter(sc.grid_center)
        m.psysLocalToWorld = sc.psys_local_to_world
        m.SetDisplacementTexture(sc.cubemap)
        if use_meshes:
            m.SetOccluders(others)
            m.SetOccluderMeshes([CUBE], inst)
        else:
            m.SetOccluders(solids)
        frames.append(m.OnPostRender(0, sc.particles, sc.layout, sc.camera()))
    bad = (np.abs(frames[0] - frames[1]).max(axis=-1) > 1e-3).sum()
    assert bad <= 3, bad
    assert np.abs(frames[0] - ia).max() <= 1e-3 or (np.abs(frames[0] - ia).max(axis=-1) > 1e-3).sum() <= 3


def test_kept_maps_are_rerendered_exactly_when_needed():
    sc = S.make_scene("T0")
    meshes = [S.torus_mesh(), CUBE]
    inst = [S.make_instance(0, S.trs((0.0, 0.5, 0.0), S.quat_to_matrix((0.3, 0.1, 0.0, 0.949)), (4.0, 4.0, 4.0))),
            S.make_instance(1, S.trs((1.5, 1.0, -1.0), np.eye(3), (1.0, 2.0, 1.0)))]
    moved = [inst[0], S.make_instance(1, S.trs((0.5, -1.0, -1.0), np.eye(3), (2.0, 2.0, 1.0)))]
    meshes2 = [S.icosphere_mesh(2), CUBE]
    D = 0.8 * sc.N[0] * sc.mv_scale

    def fresh(meshes_, inst_, cam=None):
        e = E.Engine(sc.config())
        if meshes_ is not None:
            e.set_occluder_meshes(meshes_)
            e.set_occluder_instances(inst_)
        return _frame(e, sc)[0], e.raymarch(cam if cam is not None else sc.camera(), sc.raymarch_params())

    e = E.Engine(sc.config())
    e.set_occluder_meshes(meshes)
    e.set_occluder_instances(inst)
    lm, img = _frame(e, sc)
    fl, fi = fresh(meshes, inst)
    assert np.array_equal(lm, fl) and np.array_equal(img, fi)
    e.set_occluder_instances(moved)                                                  # move one instance
    lm, img = _frame(e, sc)
    fl, fi = fresh(meshes, moved)
    assert np.array_equal(lm, fl) and np.array_equal(img, fi)
    e.set_occluder_meshes(meshes2)                                                   # change the shape list (removes the instances)
    e.set_occluder_instances(moved)
    lm, img = _frame(e, sc)
    fl, fi = fresh(meshes2, moved)
    assert np.array_equal(lm, fl) and np.array_equal(img, fi)
    sc.set_camera((0.3 * D, 0.2 * D, -D))                                            # move the camera
    cam2 = sc.camera()
    img = e.raymarch(cam2, sc.raymarch_params())
    _, fi = fresh(meshes2, moved, cam2)
    assert np.array_equal(img, fi)
    rp = sc.raymarch_params()                                                        # a caller's map overrides everything
    depth = np.full((sc.height, sc.width), 3e38, np.float32)
    depth[: sc.height // 2] = 1.0
    rp.scene_depth = depth.ctypes.data_as(abi.c_float_p)
    img_caller = e.raymarch(cam2, rp)
    f = E.Engine(sc.config())                                                        # (its light depth map still comes from the meshes)
    f.set_occluder_meshes(meshes2)
    f.set_occluder_instances(moved)
    _frame(f, sc)
    assert np.array_equal(img_caller, f.raymarch(cam2, rp))
    e.set_occluder_meshes([])                                                        # clear: as a context that never had meshes
    lm, img = _frame(e, sc)
    g = E.Engine(sc.config())
    gl, gi = _frame(g, sc)
    assert np.array_equal(lm, gl) and np.array_equal(e.raymarch(cam2, sc.raymarch_params()), g.raymarch(cam2, sc.raymarch_params()))


def test_refused_input_changes_nothing():
    sc = S.make_scene("T0")
    meshes = [S.torus_mesh(), CUBE]
    inst = [S.make_instance(0, S.trs((0.0, 0.5, 0.0), np.eye(3), (4.0, 4.0, 4.0))), S.make_instance(1, S.trs((1.5, 1.0, -1.0), np.eye(3), (1.0, 2.0, 1.0)))]
    e = _meshes_engine(sc, meshes, inst)
    before = _maps(e, sc)
    L, h = e.L, e.h
    pos, tri = CUBE

    def mesh_call(p, t, nv=None, nt=None):
        arr = (abi.vp_mesh * 1)()
        arr[0] = abi.vp_mesh(p.ctypes.data if p is not None else None, t.ctypes.data if t is not None else None,
                             len(p) if nv is None else nv, len(t) if nt is None else nt)
        return L.vp_set_occluder_meshes(h, arr, 1)

    bad_idx = tri.copy(); bad_idx[3, 1] = 24
    neg_idx = tri.copy(); neg_idx[0, 0] = -1
    nan_pos = pos.copy(); nan_pos[5, 2] = np.nan
    inf_pos = pos.copy(); inf_pos[0, 0] = np.inf
    assert mesh_call(pos, bad_idx) == abi.VP_ERR_BAD_ARG
    assert mesh_call(pos, neg_idx) == abi.VP_ERR_BAD_ARG
    assert mesh_call(nan_pos, tri) == abi.VP_ERR_BAD_ARG
    assert mesh_call(inf_pos, tri) == abi.VP_ERR_BAD_ARG
    assert mesh_call(pos, None, nt=12) == abi.VP_ERR_BAD_ARG
    assert mesh_call(pos, tri, nv=-1) == abi.VP_ERR_BAD_ARG
    assert L.vp_set_occluder_meshes(h, None, 2) == abi.VP_ERR_BAD_ARG
    assert L.vp_set_occluder_meshes(h, None, -1) == abi.VP_ERR_BAD_ARG

    def inst_call(insts):
        arr = (abi.vp_mesh_instance * len(insts))(*insts)
        return L.vp_set_occluder_instances(h, arr, len(insts))

    good = S.make_instance(1, np.eye(4))
    for mut in ("nan", "inf", "affine", "mesh_hi", "mesh_neg", "reserved"):
        b = S.make_instance(1, np.eye(4))
        if mut == "nan": b.object_to_world[5] = float("nan")
        elif mut == "inf": b.object_to_world[12] = float("inf")
        elif mut == "affine": b.object_to_world[3] = 0.5
        elif mut == "mesh_hi": b.mesh = 2
        elif mut == "mesh_neg": b.mesh = -1
        elif mut == "reserved": b.reserved[1] = 1
        assert inst_call([good, b]) == abi.VP_ERR_BAD_ARG, mut
    assert L.vp_set_occluder_instances(h, None, 1) == abi.VP_ERR_BAD_ARG
    assert L.vp_set_occluder_instances(h, None, -3) == abi.VP_ERR_BAD_ARG
    # more than 2^24 instanced triangles: VP_ERR_UNSUPPORTED (the torus has 576)
    many = (abi.vp_mesh_instance * (abi.VP_MESH_MAX_TRIANGLES // 576 + 1))()
    for i in range(len(many)):
        many[i].object_to_world[0] = many[i].object_to_world[5] = many[i].object_to_world[10] = many[i].object_to_world[15] = 1.0
    assert L.vp_set_occluder_instances(h, many, len(many)) == abi.VP_ERR_UNSUPPORTED
    after = _maps(e, sc)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # degenerate input adds nothing: a flattened instance and a zero-area triangle
    flat = S.make_instance(1, S.trs((0.0, 0.0, 0.0), np.eye(3), (1.0, 0.0, 1.0)))
    e.set_occluder_instances(inst + [flat])
    again = _maps(e, sc)
    assert np.array_equal(before[0], again[0]) and np.array_equal(before[1], again[1])
    e.set_occluder_meshes(meshes + [(np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32), np.array([[0, 1, 2]], np.int32))])
    e.set_occluder_instances(inst + [S.make_instance(2, S.trs((0.0, 0.0, 0.0), np.eye(3), (3.0, 3.0, 3.0)))])
    again = _maps(e, sc)
    assert np.array_equal(before[0], again[0]) and np.array_equal(before[1], again[1])


def test_a_million_triangles_render_deterministically():
    sc = S.make_scene("big", dims=(32, 32, 10, 1920, 1080))       # C3's light map (1024^2) and 1080p
    sphere = S.icosphere_mesh(5)                                 # 20 480 triangles
    rng = np.random.default_rng(5)
    n = 50
    D = sc.N[0] * sc.mv_scale
    inst = [S.make_instance(0, S.trs(rng.uniform(-0.3 * D, 0.3 * D, 3), np.eye(3), rng.uniform(2.0, 8.0, 3))) for _ in range(n)]
    assert n * len(sphere[1]) >= 1_000_000
    e = _meshes_engine(sc, [sphere], inst)
    cam = sc.camera()
    _maps(e, sc, cam)                                            # warm-up
    t0 = time.perf_counter()
    a = _maps(e, sc, cam)
    dt = time.perf_counter() - t0
    b = _maps(e, sc, cam)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert dt < 10.0, dt
    assert (a[0] < 1).mean() > 0.05 and (a[1] < 1e30).mean() > 0.05
    # a sample of pixels against the float64 reference (the hit pixels and their neighbours are where the work is)
    for view, got in ((MR.View.light(sc), a[0]), (MR.View.eye(sc, cam), a[1])):
        hit = np.argwhere(got != view.clear)
        pick = hit[rng.choice(len(hit), 150, replace=False)]
        pix = [(int(x), int(y)) for y, x in pick] + [(int(rng.integers(view.W)), int(rng.integers(view.H))) for _ in range(50)]
        ref, near = MR.sample(view, [sphere], inst, pix)
        g = np.asarray([got[y, x] for x, y in pix], dtype=np.float64)
        assert not (((ref != view.clear) != (g != view.clear)) & ~near).any()
        both = (ref != view.clear) & (g != view.clear) & ~near
        if view.kind == "light":
            np.testing.assert_allclose(g[both], ref[both], rtol=0, atol=1e-6)
        else:
            np.testing.assert_allclose(g[both], ref[both], rtol=1e-5)


@pytest.mark.parametrize("world", [2, 4])
def test_fanout_slabs_render_the_same_mesh_maps(world):
    sc = S.make_scene("C1", cubemap="r8")
    D = 0.8 * sc.N[0] * sc.mv_scale
    meshes = [S.torus_mesh(), CUBE]
    inst = [S.make_instance(0, S.trs((0.0, -0.1 * D, 0.0), S.quat_to_matrix((0.3, 0.1, 0.0, 0.949)), (0.5 * D, 0.5 * D, 0.5 * D))),
            S.make_instance(1, S.trs((0.15 * D, 0.1 * D, -0.3 * D), np.eye(3), (0.2 * D, 0.25 * D, 0.2 * D)))]
    single = E.Engine(sc.config())
    m = E.Engine(sc.config(devices=[0] * world, multi_flags=abi.VP_MULTI_PEER_COPY | abi.VP_MULTI_TEST_HOOKS | abi.VP_MULTI_TEST_SHARED_DEVICE))
    imgs = []
    for eng in (single, m):
        eng.set_occluder_meshes(meshes)
        eng.set_occluder_instances(inst)
        imgs.append(_frame(eng, sc)[1])
    assert (single.render_light_depth() < 1).mean() > 0.05
    assert np.abs(imgs[0] - imgs[1]).max() <= 2e-5
    np.testing.assert_allclose(m.read_lightmap(), single.read_lightmap(), rtol=2e-5, atol=1e-9)
    # the slab contexts each render the full maps: the fan-out context's own render (its first slab) is bit-identical to the single context's,
    # and the propagated light above (which reads every slab's depth map) agrees
    assert np.array_equal(m.render_light_depth(), single.render_light_depth())
    assert np.array_equal(m.render_scene_depth(sc.camera()), single.render_scene_depth(sc.camera()))
    m.close(); single.close()
