"""GPU: the ray-march's voxel-box clip (csrc/mv_box.h -> bin.hip -> march_mv in csrc/raymarch_kernels.h) starts a metavoxel visit at the box
of the voxels its particles can cover instead of at the far face of the unit cube -- and changes nothing else.

Every case renders the same frame in a context that clips in every launch (VPFX_RM_NO_BOX_CLIP=0) and in one created under
VPFX_RM_NO_BOX_CLIP=1 (the clip off) and asks for
 * bit-identical images, equal `samples`, equal `bricks_sampled` (also with the early-out off);
 * the clipping context against the CPU oracle as tests/test_gpu_parity.py does: equal sample counts with the early-out off, RGBA within 1e-3.
The scenes are 3^3 - 4^3 grids at 64 x 48 to 128 x 96 pixels with a handful of particles placed so that bricks are partly empty: a small
sphere in a brick corner, one straddling a face, a brick whose list holds only a sphere that barely touches it.  The skipped samples are not
visible in any statistic (the counts are the reference's by design), so the case that shows work being removed is a float64 model of one
metavoxel visit per pixel (test_model_one_corner_sphere)."""
import math
import os

import numpy as np
import pytest

from vpfx_amd import abi, engine as E, scene as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SWITCH = "VPFX_RM_NO_BOX_CLIP"


def _engine(cfg, clip, **kw):
    """A context with the clip in every launch (VPFX_RM_NO_BOX_CLIP=0), without it (=1), or as a default context (None).  The switch is read
    by vp_create only."""
    old = os.environ.pop(SWITCH, None)
    try:
        if clip is not None:
            os.environ[SWITCH] = "0" if clip else "1"
        return E.Engine(cfg, **kw)
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def _prepare(eng, sc):
    eng.set_frame(sc.light_to_world, sc.grid_center)
    eng.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    eng.fill(sc.fill_params())
    return eng


def _flagged(sc, flags):
    rp = sc.raymarch_params()
    rp.flags = flags
    return rp


def _look(sc, pos, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    sc.cam_to_world, sc.world_to_cam = S.look_at_camera(pos, target, up)
    sc.cam_pos = np.asarray(pos, dtype=np.float32)
    return sc


def sparse_scene(n=4, nv=16, w=96, h=64, border=1, seed=1, axis_aligned=True, extra=0):
    """Partly empty bricks on an n^3 grid (cell size s, cell (x, y, z) centred at (c + 0.5 - n / 2) s on an axis-aligned grid):
    a small sphere in the corner of cell (1, 1, 1); one straddling the face between (2, 1, 1) and (3, 1, 1) -- well, the face of the last
    column on a 3^3 grid --; one in cell (0, 2, 1) whose radius reaches 1 % of a cell into (1, 2, 1), which holds nothing else; and
    `extra` random small ones."""
    sc = S.make_scene("fuzz", seed=seed, dims=(n, nv, 3 + extra, w, h), border=border)
    if axis_aligned:
        sc.light_to_world = S.to_colmajor16(S.trs((0.0, 0.0, -44.34), np.eye(3)))
    s = sc.mv_scale
    centre = lambda c: np.array([(v + 0.5 - 0.5 * n) * s for v in c])
    pos = [centre((1, 1, 1)) + 0.36 * s, centre((n - 2, 1, 1)) + np.array([0.5 * s, 0.0, 0.1 * s]), centre((0, 2, 1)) + np.array([0.3 * s, 0.0, 0.0])]
    size = [0.2 * s, 0.5 * s, 0.42 * s]
    rng = np.random.default_rng(seed)
    for _ in range(extra):
        pos.append(rng.uniform(-0.45 * n * s, 0.45 * n * s, 3))
        size.append(s * rng.uniform(0.1, 0.7))
    sc.particles["position"] = np.array(pos, dtype=np.float32)
    sc.particles["size"] = np.array(size, dtype=np.float32)
    return sc


_oracles = {}


def _oracle(key, sc):
    """The CPU oracle of a scene, binned and filled once per module (the views of a scene share it; it is only read afterwards)."""
    if key not in _oracles:
        _oracles[key] = _prepare(O.Oracle(sc.config()), sc)
    return _oracles[key]


def check_pair(sc, key=None, engines=None):
    """The frame of `sc` with and without the clip; returns the samples of the clipping context.  engines = (on, off) already prepared."""
    cam, rp = sc.camera(), sc.raymarch_params()
    a, b = engines if engines else (_prepare(_engine(sc.config(), True), sc), _prepare(_engine(sc.config(), False), sc))
    try:
        ia, ib = a.raymarch(cam, rp), b.raymarch(cam, rp)
        sa, sb = a.stats(), b.stats()
        assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))                          # byte for byte
        assert sa["samples"] == sb["samples"] and sa["bricks_sampled"] == sb["bricks_sampled"]
        rq = _flagged(sc, abi.VP_RM_NO_EARLY_OUT)
        fa, fb = a.raymarch(cam, rq), b.raymarch(cam, rq)
        full_a, full_b = a.stats(), b.stats()
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
        assert full_a["samples"] == full_b["samples"] >= sa["samples"] and full_a["bricks_sampled"] == full_b["bricks_sampled"]
        if key is not None:
            o = _oracle(key, sc)
            io = o.raymarch(cam, rp)
            assert o.stats()["samples"] == full_a["samples"], (o.stats()["samples"], full_a["samples"])
            assert np.abs(io - ia).max() <= 1e-3 and np.abs(io - fa).max() <= 1e-3
        return sa["samples"]
    finally:
        if not engines:
            a.close()
            b.close()


VIEWS = {"+x": (14.0, 0.0, 0.0), "-x": (-14.0, 0.0, 0.0), "+y": (0.0, 14.0, 0.0), "-y": (0.0, -14.0, 0.0), "+z": (0.0, 0.0, 14.0),
         "-z": (0.0, 0.0, -14.0), "oblique": (-9.0, 6.0, -10.0), "oblique2": (7.5, -4.0, 11.0)}


@pytest.fixture(scope="module")
def nv16_pair():
    sc = sparse_scene(4, 16, 97, 65, extra=6)                 # odd image: pixel centres on the optical axis (exact zeros in a ray's direction)
    a, b = _prepare(_engine(sc.config(), True), sc), _prepare(_engine(sc.config(), False), sc)
    yield sc, a, b
    a.close()
    b.close()


@pytest.mark.parametrize("view", list(VIEWS))
def test_views_along_every_axis_and_oblique(nv16_pair, view):
    """Axis-aligned grid, camera on a grid axis: whole pixel rows / columns of rays do not move along one brick axis (1 / fs = inf)."""
    sc, a, b = nv16_pair
    _look(sc, VIEWS[view], up=(0.0, 0.0, 1.0) if view in ("+y", "-y") else (0.0, 1.0, 0.0))
    assert check_pair(sc, key="nv16", engines=(a, b)) > 0


@pytest.mark.parametrize("nv,border,n,w,h", [(32, 1, 4, 128, 96), (32, 2, 3, 96, 64), (24, 2, 3, 96, 64), (24, 1, 4, 64, 48), (64, 1, 3, 96, 64), (16, 2, 3, 64, 48)])
def test_voxel_counts_and_borders(nv, border, n, w, h):
    """nv = 24 runs the run-time-nv kernels (raymarch_generic.hip); nv = 64 the widest byte fields of the packed box."""
    sc = sparse_scene(n, nv, w, h, border=border, seed=nv + border, extra=4)
    for view in ("oblique", "-z"):
        _look(sc, VIEWS[view])
        assert check_pair(sc, key=("vc", nv, border, n)) > 0
    _oracles.pop(("vc", nv, border, n)).close()


def test_rotated_light_random_cloud():
    """The scene family of the parity tests: light-aligned grid turned against the world, 40 particles, default camera."""
    sc = S.make_scene("fuzz", seed=21, dims=(4, 16, 40, 128, 96))
    sc.particles["size"] *= np.float32(0.5)
    assert check_pair(sc, key="cloud") > 0
    d = _prepare(_engine(sc.config(), None), sc)                                              # the default context: the same frame
    c = _prepare(_engine(sc.config(), True), sc)
    assert np.array_equal(d.raymarch(sc.camera(), sc.raymarch_params()).view(np.uint32), c.raymarch(sc.camera(), sc.raymarch_params()).view(np.uint32))
    assert d.stats()["samples"] == c.stats()["samples"]
    d.close()
    c.close()
    _oracles.pop("cloud").close()


def test_coloured_ambient_rgba_bricks():
    sc = sparse_scene(4, 16, 96, 64, seed=3, extra=8)
    sc.ambient = (0.3, 0.15, 0.05)
    _look(sc, VIEWS["oblique"])
    a, b = _prepare(_engine(sc.config(), True), sc), _prepare(_engine(sc.config(), False), sc)
    assert a.stats()["brick_format"] == abi.VP_BRICKS_RGBA16F
    assert check_pair(sc, key="rgba", engines=(a, b)) > 0
    a.close()
    b.close()
    _oracles.pop("rgba").close()


def test_camera_inside_the_volume_with_the_soft_fade():
    """Visits that start behind the camera's lattice index and end inside the soft-particle range: the clip moves neither bound."""
    sc = sparse_scene(4, 16, 96, 64, seed=4, extra=10)
    sc.soft_distance = 12
    for pos, target in (((0.5, 0.3, 1.0), (0.0, 0.0, 0.0)), ((-1.4, -1.2, -1.6), (4.0, 3.0, 2.0)), ((0.2, -1.0, -2.4), (-3.0, -1.5, 4.0))):
        _look(sc, pos, target)
        assert check_pair(sc, key="inside") > 0
    _oracles.pop("inside").close()


def test_border_less_bricks_keep_the_literal_path():
    """border = 0: the footprint wraps to the opposite face, the launch does not clip; the switch changes nothing."""
    sc = sparse_scene(3, 16, 64, 48, border=0, seed=5, extra=4)
    _look(sc, VIEWS["oblique"])
    assert check_pair(sc, key="b0") > 0
    _oracles.pop("b0").close()


def test_slab_context_partial_images():
    """PARTIAL kernels: both partial images and the sample counts of two slab contexts, blended against the oracle."""
    import torch
    sc = sparse_scene(4, 16, 96, 64, seed=6, extra=10)
    _look(sc, VIEWS["oblique2"])
    dev = torch.device("cuda", 0)
    cam, rp = sc.camera(), sc.raymarch_params()
    bounds = [(0, 2), (2, 4)]
    lm = (sc.N[1] * sc.nv, sc.N[0] * sc.nv)
    results = []
    for clip in (True, False):
        engs = []
        for bnd in bounds:
            e = _engine(sc.config(device=0, slab=bnd), clip)
            e.set_frame(sc.light_to_world, sc.grid_center)
            e.upload_particles(sc.particles, sc.layout, sc.psys_local_to_world)
            e.bin_resident()
            engs.append(e)
        tau = torch.empty((2,) + lm, device=dev)
        for r, e in enumerate(engs):
            e.fill_local(sc.fill_params(), tau[r].data_ptr())
        for r, e in enumerate(engs):
            e.fill_finish_gathered(tau.data_ptr(), r, 2)
        img = torch.full((2, 2, sc.height, sc.width, 4), -1.0, device=dev)
        kinds = []
        ptrs = []
        zb = engs[0].z_boundary(cam)
        for r, e in enumerate(engs):
            e.raymarch_partial_device(cam, rp, img[r, 0].data_ptr(), img[r, 1].data_ptr())
        # compositing order of the slab images (VPR.cs:652-711): phase-A images (zz <= zBoundary) OVER, slab by slab, then phase-B images UNDER
        for r in range(2):
            ptrs.append(img[r, 0].data_ptr()); kinds.append(0)
        for r in range(2):
            ptrs.append(img[r, 1].data_ptr()); kinds.append(1)
        out = torch.empty((sc.height, sc.width, 4), device=dev)
        engs[0].blend_partials_device(ptrs, kinds, out.data_ptr())
        for e in engs:
            e.sync()
        results.append((img.cpu().numpy(), [e.stats()["samples"] for e in engs], [e.stats()["bricks_sampled"] for e in engs], out.cpu().numpy(), zb))
        for e in engs:
            e.close()
    (ia, sa, ba, oa, _), (ib, sb, bb, ob, _) = results
    assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)) and np.array_equal(oa.view(np.uint32), ob.view(np.uint32))
    assert sa == sb and ba == bb and sum(sa) > 0
    o = _prepare(O.Oracle(sc.config()), sc)
    assert np.abs(o.raymarch(cam, rp) - oa).max() <= 1e-3
    o.close()


def _replay(eng, sc, cells):
    """The reference's draw loop over `cells` through vp_render_metavoxel (all UNDER, near to far is not needed for the comparison: both
    contexts replay the same sequence)."""
    eng.clear_particles_rt()
    for i, (xx, yy, zz) in enumerate(cells):
        eng.render_metavoxel(sc.camera(), sc.raymarch_params(), xx, yy, zz, blend_over=False, order_index=i)
    return eng.read_particles_rt()


def test_render_metavoxel_replay():
    sc = sparse_scene(3, 16, 64, 48, seed=7, extra=3)
    _look(sc, VIEWS["oblique"])
    """k_raymarch_one is a flag-path kernel (it serves the debug views): it keeps the literal path in both contexts.  One metavoxel drawn alone
    is also that metavoxel's contribution to the frame where nothing else lies on the ray: the single-sphere frame equals its replay."""
    a, b = _prepare(_engine(sc.config(), True), sc), _prepare(_engine(sc.config(), False), sc)
    cells = [(xx, yy, zz) for zz in range(3) for yy in range(3) for xx in range(3)]
    ia, ib = _replay(a, sc, cells), _replay(b, sc, cells)
    assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)) and ia[..., 3].max() > 0
    for x in (a, b):
        x.close()
    one = S.make_scene("fuzz", seed=12, dims=(3, 16, 1, 64, 48))
    one.light_to_world = S.to_colmajor16(S.trs((0.0, 0.0, -44.34), np.eye(3)))
    one.particles["position"] = np.array([[0.3, -0.2, 0.4]], dtype=np.float32)                # inside the core of cell (1, 1, 1), away from its faces
    one.particles["size"] = np.float32(0.2 * one.mv_scale)
    _look(one, VIEWS["oblique"])
    e = _prepare(_engine(one.config(), True), one)
    assert e.stats()["occupied_mv"] == 1
    frame = e.raymarch(one.camera(), one.raymarch_params())
    assert np.array_equal(_replay(e, one, [(1, 1, 1)]).view(np.uint32), frame.view(np.uint32)) and frame[..., 3].max() > 0
    e.close()


def test_rebin_without_a_whole_refill():
    """vp_bin invalidates the fill, and the only way back to a ray-march without refilling every brick is the per-metavoxel fill: bin A, fill,
    bin B (other particles: other lists, other boxes, brick slots dealt out anew), vp_fill_begin, vp_fill_metavoxel for SOME cells.  The bricks
    that were not refilled hold whatever fill A left in their slot; their boxes must not be bin B's.  A ray-march straight after the re-bin is
    refused."""
    sc_a = sparse_scene(3, 16, 64, 48, seed=8, extra=12)
    sc_b = sparse_scene(3, 16, 64, 48, seed=9, extra=5)
    sc_b.particles["size"] *= np.float32(0.6)                  # smaller spheres: bin B's boxes are tighter than fill A's density
    _look(sc_b, VIEWS["oblique"])
    cam, rp = sc_b.camera(), sc_b.raymarch_params()
    imgs = []
    for clip in (True, False):
        e = _prepare(_engine(sc_a.config(), clip), sc_a)
        e.raymarch(cam, rp)
        e.bin(sc_b.particles, sc_b.layout, sc_b.psys_local_to_world)
        with pytest.raises(E.VpfxError):
            e.raymarch(cam, rp)
        occ = e.bin_counts().reshape(3, 3, 3) > 0              # [zz][yy][xx]
        cells = [(xx, yy, zz) for zz in range(3) for yy in range(3) for xx in range(3) if occ[zz, yy, xx]]
        assert len(cells) >= 4
        e.fill_begin(sc_b.fill_params())
        for c in cells[::2]:                                   # every other occupied cell: the rest keep stale bricks
            e.fill_metavoxel(*c)
        first = e.raymarch(cam, rp)
        st = e.stats()
        for c in cells[1::2]:                                  # ... and now the rest: the frame of bin B
            e.fill_metavoxel(*c)
        second = e.raymarch(cam, rp)
        e.fill(sc_b.fill_params())                             # a whole fill of the same bin
        third = e.raymarch(cam, rp)
        imgs.append((first, st["samples"], st["bricks_sampled"], second, third, e.stats()["samples"]))
        e.close()
    (f1, s1, b1, g1, h1, t1), (f2, s2, b2, g2, h2, t2) = imgs
    assert np.array_equal(f1.view(np.uint32), f2.view(np.uint32)) and s1 == s2 and b1 == b2
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
    assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and t1 == t2 > 0
    o = _prepare(O.Oracle(sc_b.config()), sc_b)
    assert np.abs(o.raymarch(cam, rp) - h1).max() <= 1e-3
    o.close()


def test_model_one_corner_sphere():
    """Work is removed: one metavoxel, one small sphere in its corner, camera on the far side of the brick from the sphere.  A float64 model of the visit
    (the reference's lattice: tEntry / tExit of the unit cube, texel = (p + 0.5)(nv - 2b) + b - 0.5) counts, per pixel, the leading samples
    -- back to front, from tExit -- whose 2 x 2 x 2 footprint misses the box of the voxels within the sphere's radius widened by two voxels
    (the box the library holds is wider than the exact one by its margin, at most one voxel a side here: tests/test_mv_box_cpu.py; the second
    voxel covers the clip's own margin and float32).  Those are samples the clip skips; the frame is still the oracle's."""
    n, nv, b = 3, 32, 1
    sc = S.make_scene("fuzz", seed=11, dims=(n, nv, 1, 96, 64), border=b)
    sc.light_to_world = S.to_colmajor16(S.trs((0.0, 0.0, -44.34), np.eye(3)))
    s = sc.mv_scale
    sc.particles["position"] = np.array([[0.3 * s, 0.3 * s, 0.3 * s]], dtype=np.float32)     # cell (1, 1, 1) is centred on the origin
    sc.particles["size"] = np.float32(0.25 * s)
    _look(sc, (6.0, 5.0, 9.0))                                                               # the sphere is at the NEAR corner: the far part of every visit is empty
    assert check_pair(sc, key="model") > 0
    _oracles.pop("model").close()
    # ---- the model (float64; the geometry of oracle/numpy_twin.py for the one metavoxel at the origin) ----
    W, H = sc.width, sc.height
    w2c, c2w = np.asarray(sc.world_to_cam, np.float64), np.asarray(sc.cam_to_world, np.float64)
    col, row = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5, indexing="xy")
    d = np.stack([(2 * col / W - 1) * (W / H), 2 * row / H - 1, np.full_like(col, -1 / math.tan(math.radians(sc.fov_y_deg) / 2))], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    halfz = 1.73205 * 0.5 * n * s
    zmin = (w2c @ np.array([0.0, 0.0, 0.0, 1.0]))[2] + halfz
    start = d * (zmin / d[..., 2:3])
    step = ((2 * halfz) / s) / (n * sc.steps)
    c2m = np.linalg.inv(S.trs((0.0, 0.0, 0.0), np.eye(3), s)) @ c2w
    o = start @ c2m[:3, :3].T + c2m[:3, 3]
    dm = d @ c2m[:3, :3].T
    dm /= np.linalg.norm(dm, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        tb, tt = (-0.5 - o) / dm, (0.5 - o) / dm
    t1, t2 = np.fmax.reduce(np.fmin(tt, tb), axis=-1), np.fmin.reduce(np.fmax(tt, tb), axis=-1)
    cover = t1 <= t2
    t_entry = np.maximum(np.ceil(t1 / step), np.trunc(np.linalg.norm(c2m[:3, 3] - o, axis=-1) / step))
    t_exit = np.floor(t2 / step)
    # exact box of the covered voxels, voxel (px, py, sl) at (px + 0.5, py + 0.5, sl) in voxel-index coordinates, brick edge sb = s nv / (nv - 2b)
    sb = s * nv / (nv - 2 * b)
    c = np.array([0.3, 0.3, 0.3]) * s * nv / sb + 0.5 * nv
    r = 0.5 * 0.25 * s * nv / sb
    ax = np.arange(nv)
    dz, dy, dx = np.meshgrid(ax - c[2], ax + 0.5 - c[1], ax + 0.5 - c[0], indexing="ij")
    zs, ys, xs = np.nonzero(dx * dx + dy * dy + dz * dz <= r * r)
    lo = np.array([xs.min(), ys.min(), zs.min()]) - 2
    hi = np.array([xs.max(), ys.max(), zs.max()]) + 2
    skipped = executed = 0
    kmax, kmin = int(np.nanmax(np.where(cover, t_exit, -1e9))), int(np.nanmin(np.where(cover, t_entry, 1e9)))
    leading = cover.copy()
    for k in range(kmax, kmin - 1, -1):
        act = cover & (k <= t_exit) & (k >= t_entry)
        f = ((o + k * step * dm) + 0.5) * (nv - 2 * b) + (b - 0.5)
        f0 = np.floor(f)
        outside = ((f0 + 1 < lo) | (f0 > hi)).any(-1)
        leading &= ~act | outside                              # a ray stops being "leading" at its first sample that can meet the box
        skipped += int((act & leading).sum())
        executed += int(act.sum())
    print(f"model: {executed} lattice samples in the metavoxel, {skipped} leading ones outside the box ({100.0 * skipped / executed:.1f} %)")
    # the widened box spans under 0.4 of each brick axis, in the corner nearest the camera: it holds under a tenth of the cube's lattice samples, and of the
    # rest only those in front of it on a ray that meets it are not leading -- more than half of all samples are skipped (the model: 91 %)
    assert executed > 1000 and 2 * skipped > executed
