"""GPU: the ray-march's empty-slab skipping (per-slab rectangles of the occupied cells, csrc/raymarch.hip: slab_rect -> k_raymarch) removes
work only where no occupied cell can be reached.

Every case renders the same frame in a context that skips (VPFX_RM_NO_SPACE_SKIP=0: as a default context does in a launch that does not fit
the GPU at once) and in one created under VPFX_RM_NO_SPACE_SKIP=1 (skipping off) and asks for
 * bit-identical images, equal `samples` and `bricks_sampled`, equal per-pixel VP_RM_SHOW_RAY_SAMPLES sums;
 * the skipping context against the CPU oracle as tests/test_gpu_parity.py does: equal sample counts with the early-out off, RGBA within 1e-3.
The shapes are T0 / T1 sized (4^3 x 16^3 at 96 x 64, 6^3 x 32^3 at 160 x 120): the smallest at which each part can go wrong."""
import os

import numpy as np
import pytest

from vpfx_amd import abi, engine as E, scene as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

T0 = (4, 16, 120, 96, 64)
T1 = (6, 32, 400, 160, 120)
SWITCH = "VPFX_RM_NO_SPACE_SKIP"


def _engine(cfg, skip, **kw):
    """A context with the skipping on or off (the switch is read by vp_create only).  skip = True is VPFX_RM_NO_SPACE_SKIP=0: a default
    context skips in the same way, but only in launches that do not fit the GPU at once (launch_raymarch) -- none of these small images;
    skip = None is that default context."""
    old = os.environ.pop(SWITCH, None)
    try:
        if skip is not None:
            os.environ[SWITCH] = "0" if skip else "1"
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


def _ray_samples(eng, sc, flags=0):
    n = eng.raymarch(sc.camera(), _flagged(sc, abi.VP_RM_SHOW_RAY_SAMPLES | flags))
    return n[..., 0].astype(np.int64)


def check_pair(sc, oracle=True, occupied=None):
    """The frame of `sc` with and without the skipping; returns (image, samples) of the skipping context."""
    cam, rp = sc.camera(), sc.raymarch_params()
    a, b = _prepare(_engine(sc.config(), True), sc), _prepare(_engine(sc.config(), False), sc)
    try:
        if occupied is not None:
            assert a.stats()["occupied_mv"] == occupied
        ia, ib = a.raymarch(cam, rp), b.raymarch(cam, rp)
        sa, sb = a.stats(), b.stats()
        assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))                          # bit for bit
        assert sa["samples"] == sb["samples"] and sa["bricks_sampled"] == sb["bricks_sampled"]
        na, nb = _ray_samples(a, sc), _ray_samples(b, sc)                                     # (a FLAGS view: it skips nothing in either context)
        assert int(na.sum()) == int(nb.sum())
        # every lattice sample, early-out off: the two paths, the per-ray view and the oracle agree
        rq = _flagged(sc, abi.VP_RM_NO_EARLY_OUT)
        fa, fb = a.raymarch(cam, rq), b.raymarch(cam, rq)
        full_a, full_b = a.stats()["samples"], b.stats()["samples"]
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and full_a == full_b >= sa["samples"]
        assert int(_ray_samples(a, sc, abi.VP_RM_NO_EARLY_OUT).sum()) == full_a
        if oracle:
            o = _prepare(O.Oracle(sc.config()), sc)
            io = o.raymarch(cam, rp)
            assert o.stats()["samples"] == full_a, (o.stats()["samples"], full_a)
            assert np.abs(io - ia).max() <= 1e-3 and np.abs(io - fa).max() <= 1e-3
            o.close()
        return ia, sa["samples"]
    finally:
        a.close()
        b.close()


def _axis_aligned(sc):
    """Grid axes = world axes (identity light rotation): exact zeros in a ray's grid-space direction become reachable."""
    sc.light_to_world = S.to_colmajor16(S.trs((0.0, 0.0, -44.34), np.eye(3)))
    return sc


def _look(sc, pos, target, up=(0.0, 1.0, 0.0)):
    sc.cam_to_world, sc.world_to_cam = S.look_at_camera(pos, target, up)
    sc.cam_pos = np.asarray(pos, dtype=np.float32)
    return sc


def _cells(sc, cells, radius=0.3):
    """Keep one small particle at the centre of each given cell (xx, yy, zz) of an axis-aligned grid."""
    n, s = sc.N[0], sc.mv_scale
    sc.particles = sc.particles[:len(cells)].copy()
    sc.particles["position"] = [[(c + 0.5 - 0.5 * n) * s for c in cell] for cell in cells]
    sc.particles["size"] = radius * s
    return sc


def test_cloud_in_one_grid_corner():
    """Most slabs and most of the screen are empty."""
    sc = S.make_scene("fuzz", seed=5, dims=T1)
    sc.particles["position"] = sc.particles["position"] * 0.3 + np.float32(0.27 * sc.N[0] * sc.mv_scale)
    img, samples = check_pair(sc)
    assert samples > 0 and (img[..., 3] == 0).mean() > 0.5
    d = _prepare(_engine(sc.config(), None), sc)                                              # the default context: the same frame
    assert np.array_equal(d.raymarch(sc.camera(), sc.raymarch_params()).view(np.uint32), img.view(np.uint32)) and d.stats()["samples"] == samples
    d.close()


def test_single_occupied_metavoxel():
    sc = _cells(_axis_aligned(S.make_scene("fuzz", seed=6, dims=T0)), [(2, 1, 1)])
    _look(sc, (-4.0, 3.0, -11.0), (0.0, 0.0, 0.0))
    _, samples = check_pair(sc, occupied=1)
    assert samples > 0


def test_empty_grid():
    sc = S.make_scene("fuzz", seed=7, dims=T0)
    sc.particles["position"] += np.float32(1000.0)
    img, samples = check_pair(sc, occupied=0)
    assert samples == 0 and not img.any()


def test_empty_slab_between_two_occupied_ones():
    sc = _cells(_axis_aligned(S.make_scene("fuzz", seed=8, dims=T0)), [(1, 2, 0), (1, 2, 2)])
    _look(sc, (1.0, 2.0, -12.0), (-1.0, 1.0, 0.0))
    _, samples = check_pair(sc, occupied=2)
    assert samples > 0


def test_camera_inside_an_occupied_cell():
    sc = S.make_scene("fuzz", seed=9, dims=T0)
    sc.set_camera((0.5, 0.3, 1.0))
    _, samples = check_pair(sc)
    assert samples > 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_camera_looking_along_a_grid_axis(axis):
    """Odd image sizes put a pixel centre on the optical axis: its ray -- and its whole pixel row / column -- has exact zeros in the grid-space
    direction (dgx == 0 / dgy == 0 / dgz == 0).  97 x 65 is also an image whose size is no multiple of the 8 x 8 wave block."""
    sc = _axis_aligned(S.make_scene("fuzz", seed=10 + axis, dims=(4, 16, 120, 97, 65)))
    pos = [0.0, 0.0, 0.0]
    pos[axis] = -11.0
    _look(sc, pos, (0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0) if axis == 1 else (0.0, 1.0, 0.0))
    _, samples = check_pair(sc)
    assert samples > 0


@pytest.mark.parametrize("pos,target", [((0.0, 0.0, -2.0), (0.0, 0.0, -30.0)), ((3.0, -2.0, 4.5), (30.0, 5.0, 9.0)), ((0.4, 0.2, -5.9), (0.0, 0.0, 0.0))])
def test_cloud_partly_behind_the_camera(pos, target):
    """Rays that start inside the cloud, with occupied slabs in front of the camera, around it and behind it."""
    sc = S.make_scene("fuzz", seed=14, dims=T0)
    _look(sc, pos, target)
    check_pair(sc)


def test_rolled_camera_transposes_the_wave_block():
    sc = S.make_scene("fuzz", seed=15, dims=T1)
    sc.particles["position"] = sc.particles["position"] * 0.5 + np.float32(0.15 * sc.N[0] * sc.mv_scale)
    _look(sc, sc.cam_pos.astype(np.float64), (0.0, 0.0, 0.0), up=(1.0, 0.0, 0.0))           # rolled 90 degrees: lanes run down screen columns
    _, samples = check_pair(sc)
    assert samples > 0


def test_rays_grazing_a_rectangle_corner():
    """One occupied cell diagonal to the rays' path: the camera slides in 64 sub-pixel steps, so rays pass the cell's corner -- and the corner
    of the widened rectangle test -- on either side at every distance.  The sample counts of the two paths are equal in every step."""
    sc = _cells(_axis_aligned(S.make_scene("fuzz", seed=16, dims=T0)), [(2, 2, 1)], radius=0.49)
    s = sc.mv_scale
    a, b = _engine(sc.config(), True), _engine(sc.config(), False)
    try:
        for e in (a, b):
            _prepare(e, sc)
        assert a.stats()["occupied_mv"] == 1
        rp = sc.raymarch_params()
        # the rays run mostly along grid x inside the slabs, a little down in y and z: they cross the x = 2, y = 2 corner of cell (2, 2, 1) diagonally
        pixel = 2.0 * 11.0 * np.tan(np.radians(30.0)) / sc.height
        total = 0
        for i in range(64):
            off = pixel * i / 64.0
            _look(sc, (-11.0 + off, 0.9 * s + off, -0.3 * s - off), (0.0, 0.02 * s + off, -0.45 * s - off))
            ia, ib = a.raymarch(sc.camera(), rp), b.raymarch(sc.camera(), rp)
            assert a.stats()["samples"] == b.stats()["samples"], i
            assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)), i
            total += a.stats()["samples"]
        assert total > 0
    finally:
        a.close()
        b.close()


def test_slab_context_with_the_hand_off_maps():
    """PARTIAL kernels: both partial images, both hand-off maps (one byte per pixel) and the sample counts of two slab contexts."""
    import torch
    sc = S.make_scene("fuzz", seed=17, dims=T0)
    sc.particles["position"] = sc.particles["position"] * 0.45 - np.float32(0.2 * sc.N[0] * sc.mv_scale)
    dev = torch.device("cuda", 0)
    cam, rp = sc.camera(), sc.raymarch_params()
    bounds = [(0, 2), (2, 4)]
    lm = (sc.N[1] * sc.nv, sc.N[0] * sc.nv)
    results = []
    for skip in (True, False):
        engs = []
        for bnd in bounds:
            e = _engine(sc.config(device=0, slab=bnd), skip)
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
        t_out = torch.full((2, 2, sc.height, sc.width), 77, device=dev, dtype=torch.uint8)
        engs[0].raymarch_partial_handoff_device(cam, rp, img[0, 0].data_ptr(), img[0, 1].data_ptr(), 0, 0, t_out[0, 0].data_ptr(), t_out[0, 1].data_ptr())
        engs[1].raymarch_partial_handoff_device(cam, rp, img[1, 0].data_ptr(), img[1, 1].data_ptr(), t_out[0, 1].data_ptr(), 1, t_out[1, 0].data_ptr(),
                                                t_out[1, 1].data_ptr())
        zb = engs[0].z_boundary(cam)
        out = torch.empty((sc.height, sc.width, 4), device=dev)
        assert zb == -1                                                                      # both slabs are UNDER images
        engs[0].blend_partials_device([img[0, 1].data_ptr(), img[1, 1].data_ptr()], [1, 1], out.data_ptr())
        for e in engs:
            e.sync()
        results.append((img.cpu().numpy(), t_out.cpu().numpy(), [e.stats()["samples"] for e in engs], [e.stats()["bricks_sampled"] for e in engs],
                        [e.zsamples() for e in engs], out.cpu().numpy()))
        for e in engs:
            e.close()
    (ia, ta, sa, ba, za, oa), (ib, tb, sb, bb, zb_, ob) = results
    assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32)) and np.array_equal(ta, tb)
    assert sa == sb and ba == bb and all(np.array_equal(x, y) for x, y in zip(za, zb_)) and sum(sa) > 0
    assert (ta[0, 0] == 0).any()                                                              # pixels no cell of slab 0 covers: transmittance 1
    o = _prepare(O.Oracle(sc.config()), sc)
    assert np.abs(o.raymarch(cam, rp) - oa).max() <= 1e-3
    o.close()


def test_run_time_voxel_count():
    """nv = 24: the NV = 0 kernels of raymarch_generic.hip get the same code through the shared template."""
    sc = S.make_scene("fuzz", seed=18, dims=(4, 24, 120, 96, 64), border=2)
    sc.particles["position"] = sc.particles["position"] * 0.4 + np.float32(0.2 * sc.N[0] * sc.mv_scale)
    _, samples = check_pair(sc)
    assert samples > 0


def test_a_flags_view_skips_nothing_and_colours_zero_sample_fragments():
    """VP_RM_SHOW_NUM_SAMPLES colours every rasterised fragment, also one in which no lattice sample falls: the FLAGS kernels skip nothing."""
    sc = _cells(_axis_aligned(S.make_scene("fuzz", seed=19, dims=T0)), [(0, 3, 0)], radius=0.2)
    _look(sc, (-2.0, 4.0, -12.0), (-4.0, 4.0, 0.0))
    cam, rq = sc.camera(), _flagged(sc, abi.VP_RM_SHOW_NUM_SAMPLES)
    a, b = _prepare(_engine(sc.config(), True), sc), _prepare(_engine(sc.config(), False), sc)
    o = _prepare(O.Oracle(sc.config()), sc)
    try:
        va, vb, vo = a.raymarch(cam, rq), b.raymarch(cam, rq), o.raymarch(cam, rq)
        assert np.array_equal(va.view(np.uint32), vb.view(np.uint32))
        assert np.abs(va - vo).max() <= 1e-3
        n = _ray_samples(a, sc, abi.VP_RM_NO_EARLY_OUT)
        assert ((va[..., 3] > 0) & (n == 0)).any()                                           # a coloured fragment without a sample
        assert np.array_equal(a.raymarch(cam, sc.raymarch_params()).view(np.uint32), b.raymarch(cam, sc.raymarch_params()).view(np.uint32))
    finally:
        for x in (a, b, o):
            x.close()
