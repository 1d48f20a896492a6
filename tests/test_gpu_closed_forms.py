"""GPU: the HIP path against answers worked out in the test (tests/independent_checks.py) -- no oracle, no twin image: an empty grid; a grid of
uniform density, where every brick texel, the light map and every ray's alpha have closed forms; one undisplaced sphere; the OVER / UNDER blend
and the final composite in float64.  tests/test_independent_checks_cpu.py applies the same functions to the C oracle first.

Measured on an MI355X: uniform fill 0 fp16 ulp from the closed form in all four kernels, light map 1.4e-6 relative; fractional part of n <= 9.3e-4,
per-ray counts equal to the float64 lattice but for one ray (default camera, 198 623 samples for 198 622); single sphere 1.4e-5 of a 5.4e-4 bound."""
import numpy as np
import pytest

import independent_checks as ic
from oracle.numpy_twin import Twin
from vpfx_amd import abi, engine as E, scene as S

pytestmark = pytest.mark.gpu


def _prepared(sc, **kw):
    eng = E.Engine(sc.config(), **kw)
    eng.set_frame(sc.light_to_world, sc.grid_center)
    eng.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    eng.fill(sc.fill_params())
    return eng


def _flagged(sc, flags):
    rp = sc.raymarch_params()
    rp.flags = flags
    return rp


def test_empty_grid_is_transparent_and_unshadowed():
    sc = S.make_scene("e", dims=(4, 16, 0, 32, 24))
    eng = _prepared(sc)
    assert eng.stats()["occupied_mv"] == 0
    np.testing.assert_array_equal(eng.read_lightmap(), 1.0)
    np.testing.assert_array_equal(eng.raymarch(sc.camera(), sc.raymarch_params()), 0.0)
    assert eng.stats()["samples"] == 0
    eng.close()


@pytest.mark.parametrize("cubemap", ["f32", "r8"])               # k_fill / k_fill_lds (with displacement 0 the texels themselves do not matter)
@pytest.mark.parametrize("exact", [False, True])
def test_uniform_density_fill(exact, cubemap):
    sc = ic.uniform_scene(cubemap)
    eng = _prepared(sc, exact=exact)
    assert eng.stats()["occupied_mv"] == 64
    worst, rel = ic.check_uniform_fill(sc, eng.read_brick, eng.read_lightmap())
    print(f"exact={exact} {cubemap}: worst {worst} fp16 ulp from the closed form, light map {rel:.1e} relative")
    eng.close()


@pytest.fixture(scope="module")
def uniform_engine():
    sc = ic.uniform_scene()
    eng = _prepared(sc)
    yield eng
    eng.close()
    del sc


@pytest.mark.parametrize("camera", list(ic.UNIFORM_CAMERAS))
def test_uniform_density_alpha_is_the_power_of_the_rays_own_sample_count(uniform_engine, camera):
    eng, sc = uniform_engine, ic.uniform_scene(camera=camera)
    cam = sc.camera()
    img = eng.raymarch(cam, _flagged(sc, abi.VP_RM_NO_EARLY_OUT))
    total = eng.stats()["samples"]
    view = eng.raymarch(cam, _flagged(sc, abi.VP_RM_SHOW_RAY_SAMPLES | abi.VP_RM_NO_EARLY_OUT))
    per_ray = view[..., 0].astype(np.int64)
    assert np.array_equal(view[..., 0], per_ray) and int(per_ray.sum()) == eng.stats()["samples"] == total
    pixels, off, frac = ic.check_uniform_rays(sc, img[..., 3], per_ray)
    # the total against the twin's lattice (uniform_ray_lattice sums to Twin.samples: test_independent_checks_cpu.py), by the sample rule
    lattice = int(ic.uniform_ray_lattice(sc)[0].sum())
    assert abs(total - lattice) <= 1e-4 * lattice + 4, (total, lattice)
    print(f"{camera}: {pixels} pixels, {off} off the float64 lattice, fractional part {frac:.1e}, samples float64 / HIP {lattice} / {total}")


def test_single_particle_density():
    sc = ic.single_particle_scene()
    eng = _prepared(sc)
    want, bound = ic.single_particle_density(sc, Twin(sc))
    co = eng.bin_counts()
    assert set(want) == {tuple(int(v) for v in c) for c in zip(*np.nonzero(co))} and len(want) >= 1
    worst = 0.0
    for (zz, yy, xx), dens in want.items():
        worst = max(worst, float(np.abs(eng.read_brick(xx, yy, zz)[..., 3].astype(np.float64) - dens).max()))
    print(f"worst density error {worst:.2e}, bound {bound:.2e}")
    assert worst <= bound
    eng.close()


def _premultiplied(rng, shape):
    a = rng.random(shape + (1,)).astype(np.float32)
    return np.concatenate([rng.random(shape + (3,)).astype(np.float32) * a, a], -1)


@pytest.mark.parametrize("h,w", [(8, 8), (47, 61)])             # 64 pixels; 2867 = 44 * 64 + 51
def test_blend_partials(h, w):
    import torch
    rng = np.random.default_rng(5)
    sc = S.make_scene("b", dims=(2, 16, 0, w, h))
    eng = E.Engine(sc.config())
    dev = torch.device("cuda", 0)
    s = [_premultiplied(rng, (h, w)) for _ in range(5)]
    kinds = [0, 0, 1, 1, 1]
    want = ic.blend_closed_form(s, kinds)

    def blend(images, kinds, ranged):
        t = [torch.from_numpy(np.ascontiguousarray(i, dtype=np.float32)).to(dev) for i in images]
        out = torch.full((h, w, 4), -1.0, device=dev)
        eng.blend_partials_device([x.data_ptr() for x in t], kinds, out.data_ptr(), num_pixels=h * w if ranged else None)
        eng.sync()
        return out.cpu().numpy()
    for ranged in (False, True):                                  # vp_blend_partials_device and its pixel-range form
        full = blend(s, kinds, ranged)
        np.testing.assert_allclose(full, want, rtol=0, atol=2e-6)
        # (s0, s1) as one OVER partial and (s2, s3, s4) as one UNDER partial, as a slab hands them on
        grouped = blend([blend(s[:2], [0, 0], ranged), blend(s[2:], [1, 1, 1], ranged)], [0, 1], ranged)
        np.testing.assert_allclose(grouped, full, rtol=0, atol=2e-6)
    eng.close()


@pytest.mark.parametrize("h,w", [(4, 4), (47, 61)])
def test_composite(h, w):
    import torch
    rng = np.random.default_rng(6)
    sc = S.make_scene("c", dims=(2, 16, 0, w, h))
    eng = E.Engine(sc.config())
    p, scene_rgba = _premultiplied(rng, (h, w)), rng.random((h, w, 4)).astype(np.float32)
    dp, ds = torch.from_numpy(p).cuda(), torch.from_numpy(scene_rgba).cuda()
    eng.composite_device(dp.data_ptr(), ds.data_ptr())
    eng.sync()
    torch.cuda.synchronize()
    np.testing.assert_allclose(ds.cpu().numpy(), ic.composite_closed_form(p, scene_rgba), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(dp.cpu().numpy(), p)
    eng.close()
