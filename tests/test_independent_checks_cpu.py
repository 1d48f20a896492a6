"""CPU: the rules of tests/independent_checks.py are satisfiable and sharp -- shown on the C oracle before they are pointed at the HIP path
(tests/test_gpu_twin.py, tests/test_gpu_closed_forms.py).  This is the one place where the oracle meets those helpers.

Measured here, oracle against twin (elements of all bricks more than 1 / more than 2 fp16 ulp apart; worst absolute brick difference
4.88e-4 = one fp16 ulp of [0.5, 1) on every scene; bin counts and lists identical on every scene; no pixel beyond 1e-4 anywhere):

    scene      elems > 1 ulp / > 2 ulp / all    light-map rel   samples twin / oracle   worst pixel
    base          89 /  31 /   442 368             1.2e-5          78 340 /  78 340        3.1e-5
    border0      110 /  29 /   442 368             1.6e-5          78 340 /  78 340        2.8e-5
    border2       86 /  30 /   442 368             1.1e-5          78 340 /  78 340        3.3e-5
    nv12          38 /  11 /   186 624             9.6e-6          78 340 /  78 340        4.6e-5
    nv24b2        18 /   2 /   442 368             8.9e-6          18 027 /  18 027        4.6e-5
    nv32         103 /  28 / 1 048 576             6.2e-6          18 027 /  18 027        9.1e-6
    fade_rad      65 /  18 /   442 368             5.2e-6          78 340 /  78 340        2.0e-5
    rgb           89 /  31 /   442 368             1.2e-5          78 340 /  78 340        3.1e-5
    r8            87 /  33 /   442 368             1.2e-5          78 340 /  78 340        3.1e-5
    D1           202 /  89 /   442 368             2.3e-5          78 340 /  78 340        4.1e-5
    over          89 /  31 /   442 368             1.2e-5          46 621 /  46 621        3.2e-5
    inside        89 /  31 /   442 368             1.2e-5          76 916 /  76 916        2.1e-6
    ldm           89 /  31 /   442 368             7.1e-6          78 340 /  78 340        3.1e-5
    sdepth        89 /  31 /   442 368             1.2e-5          47 520 /  47 519        6.0e-5
    steps7        89 /  31 /   442 368             1.2e-5           8 549 /   8 549        9.2e-6
    nv64         198 /  59 / 5 242 880             9.5e-6          13 406 /  13 406        1.3e-5
    odd           89 /  31 /   442 368             1.2e-5         548 952 / 548 952        4.2e-5

The largest share of elements more than 1 ulp off is 4.6e-4 (D1): the cap of compare_with_twin, 1e-3 of the elements beyond 2 ulp, leaves an
implementation that is within 1 ulp of the oracle twice that room.  The twin takes 0.4 - 1.5 s per scene, 3.6 s on `odd`.

Closed forms on the oracle: uniform grid -- every brick element equal to the rounded float64 value (0 ulp), light map 1.4e-6 relative (1.3e-6
at border 2, where the exponent 4 * 13 = 52 is confirmed too, also by the twin).  Rays through it:

    camera     z_boundary   pixels kept   fractional part of n   samples twin / oracle   unweighted samples   rays off the float64 lattice
    default       -1          1 530          9.1e-4                198 622 / 198 623          0                    1
    over           1            970          5.4e-4                 81 943 /  81 943         12                    0
    side           2          1 507          9.1e-4                153 349 / 153 349          0                    0

From (1.5, 14, 1) twelve rays enter the grid on the camera's own lattice index (tEntry = tCamera): with _SoftDistance 1 that sample has weight
0, is executed and counted and leaves alpha alone, so alpha is the power of the count MINUS those samples (uniform_ray_lattice).  The restated
lattice sums to the twin's sample count exactly.  Single sphere: worst density error 1.4e-5 against a bound of 5.4e-4.

Sharpness (MUTATIONS): each transcription error is put into a copy of the twin's source and the ORACLE is held to the mutated twin with the same
rules; every one must trip.  No bound had to move for that.  The `<=` for `<` in the soft-particle test is the exception: at
stepIndex - tCamera == _SoftDistance the fade factor (stepIndex - tCamera) / _SoftDistance is exactly 1, so that twin computes the same image
(measured: identical below 1e-12 on `inside`, where 960 samples sit on the equality) and no bound on results can see it; the case asserts
exactly that, and the nearest error that does change a result (the fade reaching one sample less far) trips the image rule in its place:
worst pixel 1.06e-3, 907 of the 960 pixels beyond 1e-4 where 3 are allowed.

What trips, on the oracle's own results: slice + 0.5 -> brick elements off by 0.19; propagate index -1 / +1 -> bricks off by 0.043 / 0.041;
z weights swapped -> pixels off by 0.10; floor for ceil at the entry -> 81 286 samples for 78 340."""
import functools
import inspect

import numpy as np
import pytest

import independent_checks as ic
from oracle import numpy_twin
from oracle import oracle as O
from oracle.numpy_twin import Twin


def _prepared(sc):
    o = O.Oracle(sc.config())
    o.set_frame(sc.light_to_world, sc.grid_center)
    o.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    o.fill(sc.fill_params())
    return o


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """The oracle's results for a scene of SCENES in the form compare_with_twin takes (computed once, only read afterwards)."""
    sc = ic.scene(name)
    o = _prepared(sc)
    img = o.raymarch(sc.camera(), sc.raymarch_params())
    got = ic.collect(o, sc, img, o.stats()["samples"])
    o.close()
    return got


@pytest.mark.parametrize("name", ic.SCENE_NAMES)
def test_oracle_obeys_the_twin_rules(name):
    m = ic.compare_with_twin(oracle_result(name), ic.twin_result(name))
    print(f"{name}: > 1 ulp {m['brick_gt1']}, > 2 ulp {m['brick_gt2']} of {m['brick_elems']}; worst brick {m['brick_abs']:.2e}; light map {m['light_rel']:.1e}; "
          f"samples twin / oracle {m['samples']}; worst pixel {m['pixel_worst']:.1e}, {m['pixels_gt_1e4']} beyond 1e-4")
    # the floor the ulp cap was derived from: the oracle alone stays under half of it
    assert m["brick_gt1"] <= 5e-4 * m["brick_elems"]


def test_scene_list_reaches_what_it_is_meant_to():
    tw = {n: ic.twin_result(n) for n in ("base", "over", "inside", "sdepth", "ldm")}
    assert tw["base"]["z_boundary"] == -1 and tw["over"]["z_boundary"] >= 0 and tw["inside"]["z_boundary"] >= 0      # phase A (OVER) is reached
    assert tw["sdepth"]["samples"] < 0.7 * tw["base"]["samples"]                                                     # scene depth rejects metavoxels
    assert tw["ldm"]["lightmap"].mean() > 1.2 * tw["base"]["lightmap"].mean()                                        # the occluder stops the attenuation
    assert len(set(ic.SCENE_NAMES)) == len(ic.SCENE_NAMES) >= 17


# ---- sharpness: the rules trip on plausible transcription errors ---------------------------------------------------------------------------
def mutated_twin(old, new):
    """The Twin class of a copy of oracle/numpy_twin.py in which the one occurrence of `old` reads `new`."""
    src = inspect.getsource(numpy_twin)
    assert src.count(old) == 1, f"{old!r} occurs {src.count(old)} times in numpy_twin.py"
    ns = {"__name__": "numpy_twin_mutant"}
    exec(compile(src.replace(old, new), "numpy_twin_mutant", "exec"), ns)
    return ns["Twin"]


MUTATIONS = {
    # name: (scene, text of the twin, what it becomes)
    "slice_plus_half": ("base", "np.full_like(px, (0 - nv / 2) / nv)", "np.full_like(px, (0 + 0.5 - nv / 2) / nv)"),          # quirk Q4 "repaired"
    "bidx_minus_one": ("base", "bidx = nv - min(max(self.b, 0), nv - 2)", "bidx = nv - min(max(self.b, 0), nv - 2) - 1"),
    "bidx_plus_one": ("base", "bidx = nv - min(max(self.b, 0), nv - 2)", "bidx = nv - min(max(self.b, 0), nv - 2) + 1"),
    "z_weights_swapped": ("base", "(c00 * (1 - wy) + c10 * wy) * (1 - wz) + (c01 * (1 - wy) + c11 * wy) * wz",
                          "(c00 * (1 - wy) + c10 * wy) * wz + (c01 * (1 - wy) + c11 * wy) * (1 - wz)"),
    "entry_floor": ("base", "t_entry = np.ceil(t1 / step)", "t_entry = np.floor(t1 / step)"),
    "soft_one_short": ("inside", "soft = (k - t_cam) < sc.soft_distance", "soft = (k - t_cam) < sc.soft_distance - 1"),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_rules_trip_on_a_transcription_error(mutation):
    name, old, new = MUTATIONS[mutation]
    wrong = ic.run_twin(ic.scene(name), mutated_twin(old, new))
    with pytest.raises(AssertionError) as err:
        ic.compare_with_twin(oracle_result(name), wrong)
    print(f"{mutation} on {name}: {str(err.value).splitlines()[0][:200]}")


def test_soft_test_with_le_for_lt_is_the_same_function():
    """`stepIndex - tCamera <= _SoftDistance` for `<` (RM.shader:267): the sample on the equality is multiplied by _SoftDistance / _SoftDistance.
    The samples exist on `inside` and the image does not move: this error is not one a comparison of results can find."""
    sc = ic.scene("inside")
    on_equality = []


    def le_for_lt(act, k, t_cam, sd):
        on_equality.append(int((act & ((k - t_cam) == sd)).sum()))
        return (k - t_cam) <= sd
    cls = mutated_twin("soft = (k - t_cam) < sc.soft_distance", "soft = _soft(act, k, t_cam, sc.soft_distance)")
    cls.raymarch.__globals__["_soft"] = le_for_lt
    le = ic.run_twin(sc, cls)
    assert sum(on_equality) > 100
    assert np.abs(le["rgba"] - ic.twin_result("inside")["rgba"]).max() < 1e-12
    assert le["samples"] == ic.twin_result("inside")["samples"]
    print(f"samples on the equality: {sum(on_equality)}")


# ---- closed forms on the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [1, 2])
def test_uniform_fill_closed_form(border):
    sc = ic.uniform_scene()
    sc.border = border
    o = _prepared(sc)
    assert o.stats()["occupied_mv"] == 64
    worst, rel = ic.check_uniform_fill(sc, o.read_brick, o.read_lightmap())
    _, light = ic.uniform_closed_form(sc)
    rho = float(np.float32(sc.opacity_factor))
    assert light == (1.0 + rho) ** -(4 * (16 - border - 1))                  # 56 at border 1, 52 at border 2
    print(f"border {border}: worst {worst} fp16 ulp, light map {rel:.1e} relative")
    # the twin agrees with the closed form too (its bidx / prop logic is where the exponent comes from)
    tw = Twin(sc)
    tw.grid(); tw.bin(); tw.fill()
    # (the twin keeps the opacity factor as the double 0.04, the closed form as the float the engines get: 2.2e-8 of rho, 4.8e-8 after 56 voxels)
    np.testing.assert_allclose(tw.light, light, rtol=1e-7)
    o.close()


@functools.lru_cache(maxsize=None)
def uniform_twin(camera):
    return ic.run_twin(ic.uniform_scene(camera=camera))


@pytest.mark.parametrize("camera", list(ic.UNIFORM_CAMERAS))
def test_uniform_alpha_is_an_integer_power(camera):
    sc = ic.uniform_scene(camera=camera)
    o = _prepared(sc)
    img = o.raymarch(sc.camera(), sc.raymarch_params())
    pixels, off, frac = ic.check_uniform_rays(sc, img[..., 3])
    tw = uniform_twin(camera)
    count, unweighted = ic.uniform_ray_lattice(sc)
    assert int(count.sum()) == tw["samples"]                                 # the restated lattice is the twin's, sample for sample
    assert (int(unweighted.sum()) > 0) == (camera == "over")                 # 12 rays enter the grid on the camera's own lattice index
    assert ic.check_uniform_rays(sc, tw["rgba"][..., 3])[1] == 0             # and the twin's alpha is the power of its counts on every ray
    assert (tw["z_boundary"] >= 0) == (camera != "default")                  # "over" and "side" blend their first slabs OVER
    got = o.stats()["samples"]
    assert abs(got - tw["samples"]) <= 1e-4 * tw["samples"] + 4
    print(f"{camera}: z_boundary {tw['z_boundary']}, {pixels} pixels, {off} off the lattice, fractional part {frac:.1e}, samples twin / oracle {tw['samples']} / {got}, "
          f"{int(unweighted.sum())} unweighted")
    o.close()


def test_single_particle_density_closed_form():
    sc = ic.single_particle_scene()
    o = _prepared(sc)
    want, bound = ic.single_particle_density(sc, Twin(sc))
    co = o.bin_counts()
    assert set(want) == {tuple(int(v) for v in c) for c in zip(*np.nonzero(co))} and len(want) >= 1
    worst = 0.0
    for (zz, yy, xx), dens in want.items():
        worst = max(worst, float(np.abs(o.read_brick(xx, yy, zz)[..., 3].astype(np.float64) - dens).max()))
    print(f"worst density error {worst:.2e}, bound {bound:.2e}")
    assert worst <= bound
    o.close()


def test_blend_and_composite_closed_forms():
    rng = np.random.default_rng(5)

    def rnd(h, w):
        a = rng.random((h, w, 1)).astype(np.float32)
        return np.concatenate([rng.random((h, w, 3)).astype(np.float32) * a, a], -1)
    s = [rnd(8, 8) for _ in range(5)]
    kinds = [0, 0, 1, 1, 1]
    full = ic.blend_closed_form(s, kinds)
    np.testing.assert_allclose(O.blend_partials(8, 8, s, kinds), full, rtol=0, atol=2e-6)
    grouped = ic.blend_closed_form([ic.blend_closed_form(s[:2], [0, 0]), ic.blend_closed_form(s[2:], [1, 1, 1])], [0, 1])
    np.testing.assert_allclose(grouped, full, rtol=0, atol=1e-12)             # exact associativity of premultiplied OVER / UNDER
    for h, w in ((4, 4), (47, 61)):
        p, scn = rnd(h, w), rng.random((h, w, 4)).astype(np.float32)
        np.testing.assert_allclose(O.composite(p, scn), ic.composite_closed_form(p, scn), rtol=0, atol=1e-6)
