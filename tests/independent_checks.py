"""Test infrastructure: checks of the hot path that do not run through oracle/vp_oracle.c.

Two kinds of evidence, both float64 numpy and both free of the C oracle (this module never imports oracle.oracle):
 * the float64 twin (oracle/numpy_twin.py) on a list of tiny scenes, SCENES, with one rule set, compare_with_twin, that takes the
   results of EITHER implementation as a plain dict of arrays -- tests/test_independent_checks_cpu.py feeds it from the oracle (and shows that
   the rules are satisfiable and that they trip on plausible transcription errors), tests/test_gpu_twin.py from the HIP engine;
 * closed forms: a uniform-density grid (every brick texel, the light map, alpha as an integer power), one undisplaced sphere, the
   OVER / UNDER blend recurrences and the final composite.

Where each bound comes from is said next to it; the measured distances of the oracle are in the docstring of test_independent_checks_cpu.py.
"""
from __future__ import annotations

import copy
import functools
import math

import numpy as np

from oracle.numpy_twin import Twin
from vpfx_amd import scene as S

BASE_DIMS = (3, 16, 50, 40, 24)


def _base(dims=BASE_DIMS, **kw):
    sc = S.make_scene("tiny", dims=dims, **kw)
    sc.set_camera((-1.0, 0.6, -7.5))                        # the scene of test_oracle_golden.py::test_twin_live_tiny_scene
    return sc


def _with(**attrs):
    def make():
        sc = _base()
        for k, v in attrs.items():
            setattr(sc, k, v)
        return sc
    return make


def _over():
    sc = _base()
    sc.set_camera((1.5, 10.0, 1.0))                         # z_boundary >= 0: the first slabs are blended OVER (phase A)
    return sc


def _inside():
    sc = _base()
    sc.set_camera((0.5, 0.3, 1.0))                          # camera inside the grid: visits cut at the camera's lattice index, faded samples
    sc.soft_distance = 12
    return sc


def _ldm():
    sc = _base()
    n = sc.N[0] * sc.nv                                     # an occluder plane through the grid centre: the light camera is 200 in front of it
    sc.light_depth_map = np.full((n, n), (200.0 - 0.3) / 999.7, dtype=np.float32)
    return sc


def _sdepth():
    sc = _base()
    sc.scene_depth = np.full((sc.height, sc.width), 8.0, dtype=np.float32)      # a wall behind the grid centre: the far metavoxels are rejected
    return sc


SCENES = [
    ("base", _base),
    ("border0", lambda: _base(border=0)),
    ("border2", lambda: _base(border=2)),
    ("nv12", lambda: _base((3, 12, 50, 40, 24))),
    ("nv24b2", lambda: _base((2, 24, 20, 40, 24), border=2)),
    ("nv32", lambda: _base((2, 32, 16, 40, 24))),
    ("fade_rad", lambda: _base(fade=1, rotation_in_radians=True)),
    ("rgb", _with(ambient=(0.3, 0.15, 0.05))),
    ("r8", lambda: _base(cubemap="r8")),
    ("D1", _with(displacement_scale=1.0)),
    ("over", _over),
    ("inside", _inside),
    ("ldm", _ldm),
    ("sdepth", _sdepth),
    ("steps7", _with(steps=7)),
    ("nv64", lambda: _base((2, 64, 8, 40, 24))),
    ("odd", lambda: _base((3, 16, 50, 97, 65))),            # odd image: pixel centres on the optical axis, partial pixel blocks
]
SCENE_NAMES = [n for n, _ in SCENES]


def scene(name):
    """A fresh copy of the named scene (the engines keep pointers into its arrays: hold on to it while they run)."""
    return dict(SCENES)[name]()


def twin_scene(sc):
    """What the twin reads: an 8-bit cube map as the texel values it stands for (byte / 255) in float64."""
    if sc.cubemap.dtype != np.uint8:
        return sc
    tw = copy.copy(sc)
    tw.cubemap = sc.cubemap.astype(np.float64) / 255.0
    return tw


def run_twin(sc, cls=Twin):
    """grid -> bin -> fill -> raymarch of a twin class on `sc`, as the dict compare_with_twin takes on its right-hand side."""
    tw = cls(twin_scene(sc))
    tw.grid()
    lists = tw.bin()
    tw.fill()
    rgba = tw.raymarch()
    counts = np.zeros((tw.Nz, tw.Ny, tw.Nx), dtype=np.int32)
    for k, ids in lists.items():
        counts[k] = len(ids)
    return dict(bin_counts=counts, lists={k: list(v) for k, v in lists.items()}, bricks=tw.bricks, lightmap=tw.light, rgba=rgba,
                samples=int(tw.samples), z_boundary=int(tw.z_boundary))


@functools.lru_cache(maxsize=None)
def twin_result(name):
    """The twin's answer for a scene of SCENES, computed once per process (0.5 - 2 s each) and only read afterwards."""
    return run_twin(scene(name))


def collect(eng, sc, rgba, samples, bricks=True):
    """The left-hand side of compare_with_twin from anything with the engine call surface (oracle.oracle.Oracle or vpfx_amd.engine.Engine),
    already binned and filled; `rgba` and `samples` are the caller's (the sample count is the one with every lattice sample executed)."""
    counts = eng.bin_counts()
    cells = [tuple(int(v) for v in c) for c in zip(*np.nonzero(counts))]
    got = dict(bin_counts=counts, lists={(zz, yy, xx): eng.bin_list(xx, yy, zz).tolist() for zz, yy, xx in cells},
               lightmap=eng.read_lightmap(), rgba=rgba, samples=int(samples))
    if bricks:
        got["bricks"] = {(zz, yy, xx): eng.read_brick(xx, yy, zz) for zz, yy, xx in cells}
    return got


def f16_ulp_diff(a, b):
    """|a - b| in fp16 ulps: the monotone integer mapping of binary16 that tests/test_gpu_parity.py uses."""
    def key(x):
        u = np.ascontiguousarray(x, dtype=np.float16).view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, 0x8000 - (u & 0x7fff) - 1, u + 0x8000)
    return np.abs(key(a) - key(b))


def check_image(rgba, twin_rgba):
    """The image rule of scripts/fuzz_twin.py: every pixel within 1e-3 of the twin, and at most max(3, npix // 2000) pixels beyond 1e-4
    (a lattice sample on a brick face, or a voxel centre on a sphere surface, may fall on the other side in fp32).  Returns (worst, count)."""
    d = np.abs(np.asarray(rgba, dtype=np.float64) - twin_rgba).max(axis=-1)
    worst, far = float(d.max()), int((d > 1e-4).sum())
    assert worst <= 1e-3, f"worst pixel {worst:.3e} > 1e-3"
    assert far <= max(3, d.size // 2000), f"{far} of {d.size} pixels beyond 1e-4 (worst {worst:.3e})"
    return worst, far


def compare_with_twin(got, twin, only=None):
    """Hold one implementation's results (`got`: bin_counts, lists, bricks, lightmap, rgba, samples) to the twin's.  `only` names the keys
    to check where an engine cannot give all of them (a fan-out context has no readable bricks); every key is required otherwise.
    Returns the measured distances."""
    keys = ("bin_counts", "lists", "bricks", "lightmap", "rgba", "samples") if only is None else tuple(only)
    m = {}
    if "bin_counts" in keys:        # integer work: identical
        np.testing.assert_array_equal(got["bin_counts"], twin["bin_counts"])
    if "lists" in keys:
        assert set(got["lists"]) == set(twin["lists"]), "occupied cells differ"
        for k, ids in twin["lists"].items():
            assert list(got["lists"][k]) == ids, f"bin list of cell (zz, yy, xx) = {k} differs"
    if "bricks" in keys:
        assert set(got["bricks"]) == set(twin["bricks"]), "filled cells differ"
        total = gt1 = gt2 = 0
        worst = 0.0
        for k, tb in twin["bricks"].items():
            gb = np.asarray(got["bricks"][k])
            assert gb.shape == tb.shape and gb.dtype == np.float16, (k, gb.shape, gb.dtype)
            worst = max(worst, float(np.abs(gb.astype(np.float64) - tb.astype(np.float64)).max()))
            u = f16_ulp_diff(gb, tb)
            total += u.size
            gt1 += int((u > 1).sum())
            gt2 += int((u > 2).sum())
        m.update(brick_abs=worst, brick_elems=total, brick_gt1=gt1, brick_gt2=gt2)
        # the bound of test_twin_live_tiny_scene (values are <= 1: 1e-3 is two fp16 ulp of [0.5, 1))
        assert worst <= 1e-3, f"worst brick element {worst:.3e} > 1e-3"
        # voxels whose centre sits on a smoothstep / surface decision fall on either side in fp32 and fp64: the oracle leaves <= 4.6e-4 of
        # the elements more than 1 ulp off, the HIP fill is within 1 ulp of the oracle, so its share beyond 2 ulp is bounded by that
        assert gt2 <= 1e-3 * total, f"{gt2} of {total} brick elements more than 2 fp16 ulp from the twin"
    if "lightmap" in keys:
        lm, tl = np.asarray(got["lightmap"], dtype=np.float64), twin["lightmap"]
        assert lm.shape == tl.shape
        m["light_rel"] = float((np.abs(lm - tl) / np.maximum(np.abs(tl), 1e-30)).max())
        np.testing.assert_allclose(lm, tl, rtol=1e-4, atol=1e-7)                   # the bound of test_twin_live_tiny_scene
    if "samples" in keys:           # the rule of scripts/fuzz_twin.py: a lattice sample exactly on a face is the legitimate disagreement
        m["samples"] = (twin["samples"], int(got["samples"]))
        assert abs(int(got["samples"]) - twin["samples"]) <= 1e-4 * twin["samples"] + 4, m["samples"]
    if "rgba" in keys:
        assert np.asarray(got["rgba"]).shape == twin["rgba"].shape
        m["pixel_worst"], m["pixels_gt_1e4"] = check_image(got["rgba"], twin["rgba"])
    return m


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def one_particle_scene(size, D, cubemap="f32"):
    """One particle at the origin of a 4^3 x 16^3 grid at 48 x 32 (the scene of tests/test_oracle_kat.py)."""
    sc = S.make_scene("one", dims=(4, 16, 1, 48, 32), cubemap=cubemap)
    sc.particles["position"][0] = (0.0, 0.0, 0.0)
    sc.particles["size"][0] = size
    sc.particles["rotation"][0] = 33.0
    sc.displacement_scale = D
    return sc


UNIFORM_CAMERAS = {"default": None, "over": (1.5, 14.0, 1.0), "side": (9.0, 1.0, 2.0)}      # all outside the grid; z_boundary -1, 0 and 2


def uniform_scene(cubemap="f32", camera="default"):
    """A particle so large that every voxel of all 64 metavoxels has the saturated density opacity_factor and ao 1; no soft fade beyond the
    camera's own lattice index (soft_distance 1).  With displacement 0 the cube map does not enter the result -- it picks the fill kernel."""
    sc = one_particle_scene(400.0, 0.0, cubemap)
    sc.soft_distance = 1
    if UNIFORM_CAMERAS[camera] is not None:
        sc.set_camera(UNIFORM_CAMERAS[camera])
    return sc


def uniform_closed_form(sc):
    """(texels, light): texels[zz, sl] = the float64 RGBA of every texel of slice sl of every brick of slab zz, light = the light map's
    one value.  With rho the fp32 opacity factor, light crossing a voxel is divided by 1 + rho (Fill.shader:245); a brick hands on the
    light in front of slice nv - b - 1 (the last one before the far border voxels, Fill.shader:240-253), so slice sl of slab zz sees
    (1 + rho)^-(zz (nv - b - 1) + sl) and the map ends at (1 + rho)^-(Nz (nv - b - 1))."""
    nv, b, nz = sc.nv, sc.border, sc.N[2]
    rho = float(np.float32(sc.opacity_factor))
    per = nv - min(max(b, 0), nv - 2) - 1
    zz, sl = np.meshgrid(np.arange(nz), np.arange(nv), indexing="ij")
    t = (1.0 + rho) ** -(zz * per + sl).astype(np.float64)
    tex = np.empty((nz, nv, 4))
    tex[..., :3] = 0.4 * t[..., None] + np.asarray(sc.ambient, dtype=np.float64)
    tex[..., 3] = rho
    return tex, (1.0 + rho) ** -(nz * per)


def check_uniform_fill(sc, read_brick, lightmap):
    """Every element of all bricks within 1 fp16 ulp of the round-to-nearest of the float64 value (a chain of <= 64 fp32 divisions is 4e-6
    relative, far below half an fp16 ulp of 4.9e-4 relative: only rounding-boundary flips remain), the light map within 1e-4 relative.
    Returns (worst ulp, worst light-map relative error)."""
    tex, light = uniform_closed_form(sc)
    nx, ny, nz = sc.N
    worst = 0
    for zz in range(nz):
        want = np.broadcast_to(tex[zz].astype(np.float32).astype(np.float16)[:, None, None, :], (sc.nv, sc.nv, sc.nv, 4))
        for yy in range(ny):
            for xx in range(nx):
                u = int(f16_ulp_diff(read_brick(xx, yy, zz), want).max())
                assert u <= 1, f"brick ({xx}, {yy}, {zz}): {u} fp16 ulp from the closed form"
                worst = max(worst, u)
    lm = np.asarray(lightmap, dtype=np.float64)
    assert lm.shape == (ny * sc.nv, nx * sc.nv)
    np.testing.assert_allclose(lm, light, rtol=1e-4, atol=0)
    return worst, float(np.abs(lm / light - 1.0).max())


def uniform_alpha_counts(sc, alpha):
    """Along a ray through uniform density alpha = 1 - (1 + rho16)^-n with n its integer number of full-weight samples (RM.shader:272-275;
    rho16 is the density as the bricks hold it; soft_distance 1 leaves weights 0 and 1 only, see uniform_ray_lattice).  Returns (mask, n):
    the pixels with 1e-3 < alpha < 0.999 and the real-valued n there, after asserting |n - rint(n)| < 2e-2 (the bound of
    test_uniform_density_alpha_is_integer_power)."""
    rho16 = float(np.float16(np.float32(sc.opacity_factor)))
    a = np.asarray(alpha, dtype=np.float64)
    mask = (a > 1e-3) & (a < 0.999)
    assert mask.sum() > 100
    n = -np.log1p(-a[mask]) / math.log1p(rho16)
    frac = float(np.abs(n - np.rint(n)).max())
    assert frac < 2e-2, f"alpha is not an integer power of 1 / (1 + rho): fractional part {frac:.3e}"
    return mask, n


def uniform_ray_lattice(sc):
    """(count, unweighted) per pixel, float64, for a grid whose metavoxels are all occupied and no scene depth: the lattice samples a ray
    executes -- per metavoxel stepIndex = max(ceil(tEntry), tCamera) .. floor(tExit) (RM.shader:236-254) -- and how many of them sit on the
    camera's own lattice index, stepIndex == tCamera.  Those get the weight (stepIndex - tCamera) / _SoftDistance = 0 (RM.shader:267-269):
    they are executed and counted but leave alpha as it was, so a ray's alpha is the integer power of its count MINUS these.  (tCamera is the
    DISTANCE between the camera and the ray's start on the bounding sphere's plane, so it is an index in front of the camera when the camera
    is far from the grid: from (1.5, 14, 1) a dozen rays enter the grid exactly there.)  The geometry is that of oracle/numpy_twin.py."""
    tw = Twin(sc)
    pos = tw.grid()
    W, H = sc.width, sc.height
    w2c, c2w = np.asarray(sc.world_to_cam, dtype=np.float64), np.asarray(sc.cam_to_world, dtype=np.float64)
    col, row = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5, indexing="xy")
    d = np.stack([(2 * col / W - 1) * (W / H), 2 * row / H - 1, np.full_like(col, -1 / math.tan(math.radians(sc.fov_y_deg) / 2))], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    maxdim = max(sc.N)
    halfz = 1.73205 * 0.5 * maxdim * tw.s
    start = d * (((w2c @ np.append(tw.gc, 1.0))[2] + halfz) / d[..., 2:3])
    step = ((2 * halfz) / tw.s) / (maxdim * sc.steps)
    count, unweighted = np.zeros((H, W), dtype=np.int64), np.zeros((H, W), dtype=np.int64)
    for cell in np.ndindex(pos.shape[:3]):
        c2m = np.linalg.inv(S.trs(pos[cell], tw.Rl, tw.s)) @ c2w
        o = start @ c2m[:3, :3].T + c2m[:3, 3]
        dm = d @ c2m[:3, :3].T
        dm /= np.linalg.norm(dm, axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            tb, tt = (-0.5 - o) / dm, (0.5 - o) / dm
        t1, t2 = np.fmax.reduce(np.fmin(tt, tb), axis=-1), np.fmin.reduce(np.fmax(tt, tb), axis=-1)
        exit_depth = -(start[..., 2] + d[..., 2] * t2 * tw.s)
        cover = (t1 <= t2) & (exit_depth > sc.near) & (exit_depth <= sc.far)
        t_cam = np.trunc(np.linalg.norm(c2m[:3, 3] - o, axis=-1) / step)
        t_entry, t_exit = np.maximum(np.ceil(t1 / step), t_cam), np.floor(t2 / step)
        run = cover & (t_entry <= t_exit)
        count += np.where(run, t_exit - t_entry + 1, 0).astype(np.int64)
        unweighted += run & (t_entry == t_cam)
    return count, unweighted


def check_uniform_rays(sc, alpha, per_ray=None):
    """alpha is the integer power of the ray's own sample count: on the pixels uniform_alpha_counts keeps, rint(n) + unweighted == the count.
    `per_ray` is the implementation's own per-ray count (the HIP samples-per-ray view); the equality is asked wherever that count is the
    float64 lattice's, and it may differ from the lattice on at most 4 of those pixels (a lattice sample exactly on a metavoxel face is the one
    legitimate disagreement between fp32 and float64; 4 is the absolute allowance of the sample rule).  Without `per_ray` (the oracle has
    no such view) the float64 count stands in, with the same allowance.  Returns (pixels, pixels off the lattice, worst fractional part)."""
    count, unweighted = uniform_ray_lattice(sc)
    mask, n = uniform_alpha_counts(sc, alpha)
    full = np.rint(n).astype(np.int64)
    executed = count[mask] if per_ray is None else np.asarray(per_ray)[mask].astype(np.int64)
    off_lattice = executed != count[mask]
    wrong = (full + unweighted[mask] != executed)
    if per_ray is None:
        off_lattice = wrong
    assert int(off_lattice.sum()) <= 4, f"{int(off_lattice.sum())} rays off the float64 lattice"
    assert not (wrong & ~off_lattice).any(), f"{int((wrong & ~off_lattice).sum())} rays whose alpha is not the power of their own sample count"
    return int(mask.sum()), int(off_lattice.sum()), float(np.abs(n - np.rint(n)).max())


def single_particle_scene():
    return one_particle_scene(4.0, 0.0)


def single_particle_density(sc, tw):
    """{(zz, yy, xx): density [sl][py][px]} for the metavoxels that hold the one particle (size 4, at the origin, displacement 0 => net
    displacement 1): opacity_factor * smoothstep(1, 0.7, 4 d^2) inside d^2 <= 1/4 (Fill.shader:119-127), d = (voxel - centre) / size.  The voxel
    centre has +0.5 in x and y but not along the light axis (quirk Q4, Fill.shader:103).  `tw` is a Twin of `sc` (grid and bin are run here).
    Also returns the bound of test_single_particle_density_closed_form: fp16 storage of a density <= opacity_factor plus 1e-3 relative
    (density is continuous at the sphere surface, so no voxel needs excluding)."""
    pos = tw.grid()
    lists = tw.bin()
    nv = sc.nv
    size = float(sc.particles["size"][0])
    centre = np.asarray(sc.particles["position"][0], dtype=np.float64)
    sl, py, px = np.meshgrid(np.arange(nv), np.arange(nv), np.arange(nv), indexing="ij")
    local = np.stack([(px + 0.5 - nv / 2) / nv, (py + 0.5 - nv / 2) / nv, (sl - nv / 2) / nv], -1) * tw.sb
    out = {}
    top = 0.0
    for (zz, yy, xx) in lists:
        world = local @ tw.Rl.T + pos[zz, yy, xx]
        d2 = ((world - centre) ** 2).sum(-1) / size ** 2
        t = np.clip((4 * d2 - 1.0) / (0.7 - 1.0), 0, 1)
        out[(zz, yy, xx)] = np.where(d2 <= 0.25, t * t * (3 - 2 * t) * sc.opacity_factor, 0.0)
        top = max(top, float(out[(zz, yy, xx)].max()))
    return out, 5e-4 * sc.opacity_factor / 0.04 + 1e-3 * top


def blend_closed_form(partials, kinds):
    """The ordered blend of premultiplied partial images into a cleared target in float64: kind 0 = OVER (dst = src + dst (1 - src.a)),
    kind 1 = UNDER (dst = src (1 - dst.a) + dst) -- the two blend states RenderMetavoxel sets on RM.shader:17 (VPR.cs:652-711)."""
    dst = np.zeros(np.asarray(partials[0]).shape, dtype=np.float64)
    for p, kind in zip(partials, kinds):
        src = np.asarray(p, dtype=np.float64)
        dst = src + dst * (1.0 - src[..., 3:4]) if kind == 0 else src * (1.0 - dst[..., 3:4]) + dst
    return dst


def composite_closed_form(p, scene_rgba):
    """CompositeParticles (Comp.shader:10, Blend One OneMinusSrcAlpha, One One): the particle image over the scene image, alphas added."""
    p, s = np.asarray(p, dtype=np.float64), np.asarray(scene_rgba, dtype=np.float64)
    return np.concatenate([p[..., :3] + s[..., :3] * (1.0 - p[..., 3:4]), p[..., 3:4] + s[..., 3:4]], -1)
