"""GPU: the HIP path held to the float64 twin (oracle/numpy_twin.py) directly -- bin lists, every brick, the light map, the lattice sample count
and the image of every scene of tests/independent_checks.py under the rules of compare_with_twin.  The C oracle is not part of this file: a
reading of the reference that the oracle and the kernels share cannot hide here.  The same rules are shown satisfiable (on the oracle) and sharp
(against transcription errors put into the twin) in tests/test_independent_checks_cpu.py; where the bounds come from is said there and in the
helper.

The main matrix runs a default-math context that takes the ray-march's slab skip and voxel-box clip in every launch (a default context would
take neither at these image sizes); three scenes also run the EXACT fill, a context with both switched off, a context as a caller gets it, and
one scene the fan-out inside the library (split fill with its finish pass, partial images, blend).  Between them: k_fill (f32 cube map) in both
maths and k_fill_lds (r8); the run-time-nv kernels (nv 12, 24) and the nv 16 / 32 / 64 instantiations; z-pair and RGBA16F bricks; the OVER
phase, scene-depth rejection and the light-depth shadow.  Each case costs the twin's CPU time (0.4 - 4 s, once per scene and process).

Measured on an MI355X (default math): lists identical; at most 203 of 442 368 brick elements more than 1 fp16 ulp and 88 more than 2 ulp from the
twin (D1; the oracle: 202 / 89), light map <= 2.3e-5 relative, lattice samples equal on 16 scenes and 47 519 for 47 520 on `sdepth` (as the
oracle), worst pixel 6.0e-5, no pixel beyond 1e-4; fan-out 1.2e-5 / 3.1e-5."""
import os

import pytest

import independent_checks as ic
from vpfx_amd import abi, engine as E

pytestmark = pytest.mark.gpu

SWITCHES = ("VPFX_RM_NO_SPACE_SKIP", "VPFX_RM_NO_BOX_CLIP")


def _engine(cfg, switch, **kw):
    """A context that skips empty slabs and clips to the voxel box in every launch (switch "0"), in none ("1"), or by the default rule (None).
    vp_create alone reads the switches."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        if switch is not None:
            for k in SWITCHES:
                os.environ[k] = switch
        return E.Engine(cfg, **kw)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _flagged(sc, flags):
    rp = sc.raymarch_params()
    rp.flags = flags
    return rp


def hold_to_twin(name, switch="0", **kw):
    """One engine on one scene: bin, fill, both ray-marches, everything read back and compared.  Returns (engine stats, measured distances)."""
    sc, twin = ic.scene(name), ic.twin_result(name)
    eng = _engine(sc.config(), switch, **kw)
    try:
        eng.set_frame(sc.light_to_world, sc.grid_center)
        eng.bin(sc.particles, sc.layout, sc.psys_local_to_world)
        eng.fill(sc.fill_params())
        assert eng.z_boundary(sc.camera()) == twin["z_boundary"]
        default = eng.raymarch(sc.camera(), sc.raymarch_params())
        executed = eng.stats()["samples"]
        full = eng.raymarch(sc.camera(), _flagged(sc, abi.VP_RM_NO_EARLY_OUT))
        st = eng.stats()
        assert 0 < executed <= st["samples"]
        m = ic.compare_with_twin(ic.collect(eng, sc, full, st["samples"]), twin)
        ic.check_image(default, twin["rgba"])                                   # the frame a caller gets obeys the image rule too
        print(f"{name}: > 1 ulp {m['brick_gt1']}, > 2 ulp {m['brick_gt2']} of {m['brick_elems']}; light map {m['light_rel']:.1e}; samples twin / HIP {m['samples']}; "
              f"worst pixel {m['pixel_worst']:.1e}")
        return st, m
    finally:
        eng.close()


RGBA_SCENES = ("border0", "rgb")                # a border-less brick or a coloured ambient keeps RGBA16F; grey ambient with a border packs z-pairs


@pytest.mark.parametrize("name", ic.SCENE_NAMES)
def test_default_math_with_the_skip_and_the_clip(name):
    st, _ = hold_to_twin(name)
    assert st["brick_format"] == (abi.VP_BRICKS_RGBA16F if name in RGBA_SCENES else abi.VP_BRICKS_GREY_ZPAIR)
    assert st["occupied_mv"] == len(ic.twin_result(name)["lists"])


EXTRA = ("base", "nv24b2", "r8")                # k_fill + nv 16, the run-time-nv kernels at border 2, k_fill_lds


@pytest.mark.parametrize("name", EXTRA)
def test_exact_fill(name):
    hold_to_twin(name, exact=True)


@pytest.mark.parametrize("name", EXTRA)
def test_skip_and_clip_switched_off(name):
    hold_to_twin(name, switch="1")


@pytest.mark.parametrize("name", EXTRA)
def test_context_as_a_caller_gets_it(name):
    hold_to_twin(name, switch=None)


def test_fan_out_inside_the_library():
    """Two slabs on one GPU: the split fill with its finish pass, partial images and the blend.  Bricks are not readable there."""
    sc, twin = ic.scene("base"), ic.twin_result("base")
    eng = E.Engine(sc.config(devices=[0, 0], multi_flags=abi.VP_MULTI_PEER_COPY))
    try:
        eng.set_frame(sc.light_to_world, sc.grid_center)
        eng.bin(sc.particles, sc.layout, sc.psys_local_to_world)
        eng.fill(sc.fill_params())
        img = eng.raymarch(sc.camera(), sc.raymarch_params())
        assert eng.multi_info()["world_size"] == 2
        m = ic.compare_with_twin(dict(lightmap=eng.read_lightmap(), rgba=img), twin, only=("lightmap", "rgba"))
        print(f"fan-out: light map {m['light_rel']:.1e}, worst pixel {m['pixel_worst']:.1e}")
    finally:
        eng.close()
