"""GPU: particles that never leave the device -- `vp_upload_particles_device` (records already in device memory) against the host upload,
and the device particle source (`vp_device_emitter_*`, csrc/emitter_device.hip) against the host emitter it restates: bit for bit on the live
count after every step, the order, lifetime, rotation, size and startLifetime; positions (two different math libraries) within
B = (16 + s) 2^-23 (cone_radius + |speed| lifetime) of the float64 twin of tests/emitter_twin.py, s = steps the particle has lived."""
import ctypes as C

import numpy as np
import pytest
import torch

import emitter_twin as T
from vpfx_amd import abi, engine as E, scene as S

pytestmark = pytest.mark.gpu


def to_device(records: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(records.tobytes(), dtype=np.uint8).copy()).cuda()


def frame(eng, sc):
    eng.bin_resident()
    eng.fill(sc.fill_params())
    return eng.raymarch(sc.camera(), sc.raymarch_params())


def assert_same_volume(a, b, img_a, img_b):
    """bin counts, every bin list, every occupied brick and the image: bit-identical"""
    ca, cb = a.bin_counts(), b.bin_counts()
    assert np.array_equal(ca, cb)
    for zz, yy, xx in np.argwhere(ca > 0):
        assert np.array_equal(a.bin_list(xx, yy, zz), b.bin_list(xx, yy, zz)), (xx, yy, zz)
        assert a.read_brick(xx, yy, zz).tobytes() == b.read_brick(xx, yy, zz).tobytes(), (xx, yy, zz)
    assert img_a.tobytes() == img_b.tobytes()
    return int((ca > 0).sum())


def repacked(sc):
    """The scene's particles as 37-byte records with unaligned field offsets and the rotation in radians."""
    lay = abi.vp_particle_layout()
    lay.stride, lay.off_position, lay.off_size, lay.off_rotation, lay.off_lifetime, lay.off_start_lifetime = 37, 1, 13, 18, 23, 31
    lay.rotation_in_radians = 1
    p = sc.particles
    rec = np.full((len(p), 37), 0xCD, dtype=np.uint8)

    def put(off, v):
        b = np.ascontiguousarray(v, dtype="<f4").reshape(len(p), -1).view(np.uint8)
        rec[:, off:off + b.shape[1]] = b
    put(1, p["position"]); put(13, p["size"]); put(18, np.radians(p["rotation"].astype(np.float64)).astype(np.float32))
    put(23, p["lifetime"]); put(31, p["startLifetime"])
    return rec.reshape(-1).view("V37"), lay


# ---- 1. device upload = host upload -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["unity84", "packed37_radians_moved"])
def test_device_upload_equals_host_upload(which):
    sc = S.make_scene("T1")
    records, lay, l2w = sc.particles, sc.layout, np.array(sc.psys_local_to_world, dtype=np.float32)
    if which != "unity84":
        records, lay = repacked(sc)
        l2w[12:15] += np.array([1.25, -0.75, 2.5], dtype=np.float32)            # column-major: the translation
    dev, host = E.Engine(sc.config(device=0)), E.Engine(sc.config(device=0))
    d = to_device(records)
    for e in (dev, host):
        e.set_frame(sc.light_to_world, sc.grid_center)
    dev.upload_particles_device(d.data_ptr(), len(records), lay, l2w)
    host.upload_particles(records, lay, l2w)
    occupied = assert_same_volume(dev, host, frame(dev, sc), frame(host, sc))
    assert occupied > 20 and dev.stats()["particles"] == 400
    # count = 0 works (and needs no pointer)
    dev.upload_particles_device(0, 0, lay, l2w)
    dev.bin_resident()
    assert not dev.bin_counts().any() and dev.stats()["particles"] == 0
    dev.close(); host.close()


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_uploads_leave_the_previous_particles_in_effect():
    sc = S.make_scene("T1")
    eng = E.Engine(sc.config(device=0))
    eng.set_frame(sc.light_to_world, sc.grid_center)
    d = to_device(sc.particles)
    eng.upload_particles_device(d.data_ptr(), len(sc.particles), sc.layout, sc.psys_local_to_world)
    eng.bin_resident()
    before = eng.bin_counts()
    assert before.any()
    half = np.ascontiguousarray(sc.particles[:200])
    bad_layout = S.particle_layout()
    bad_layout.off_size = bad_layout.stride - 2
    for ptr, n, lay in ((half.ctypes.data, len(half), sc.layout),          # unregistered host memory
                        (d.data_ptr(), 200, bad_layout),                    # a field outside the record
                        (0, 200, sc.layout),                                # NULL with count > 0
                        (d.data_ptr(), -1, sc.layout)):
        with pytest.raises(E.VpfxError) as ei:
            eng.upload_particles_device(ptr, n, lay, sc.psys_local_to_world)
        assert ei.value.code == abi.VP_ERR_BAD_ARG
    eng.bin_resident()
    assert np.array_equal(eng.bin_counts(), before) and eng.stats()["particles"] == 400
    eng.close()


def test_fanout_contexts_do_not_take_device_particles():
    sc = S.make_scene("T1")
    single = E.Engine(sc.config(device=0))
    em = S.DeviceEmitter(single)
    fan = E.Engine(sc.config(devices=[0, 0], multi_flags=abi.VP_MULTI_PEER_COPY))
    d = to_device(sc.particles)
    with pytest.raises(E.VpfxError) as ei:
        fan.upload_particles_device(d.data_ptr(), len(sc.particles), sc.layout, sc.psys_local_to_world)
    assert ei.value.code == abi.VP_ERR_UNSUPPORTED
    with pytest.raises(E.VpfxError) as ei:
        fan.upload_particles_from_emitter(em, sc.psys_local_to_world)
    assert ei.value.code == abi.VP_ERR_UNSUPPORTED
    h = C.c_void_p()
    assert E.lib().vp_device_emitter_create(fan.h, C.byref(em.cfg), C.byref(h)) == abi.VP_ERR_UNSUPPORTED and not h.value
    em.close(); fan.close(); single.close()


# ---- 3.-5. the device emitter against the host emitter -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    sc = S.make_scene("T0")
    e = E.Engine(sc.config(device=0))
    yield e
    e.close()


def check_against_host(dev, host, twin):
    """The probe's records against the host emitter's: the bit-exact fields exactly, oldest first; positions within B of the twin."""
    d, h, t = dev.particles(), host.particles(), twin.particles()
    assert len(d) == len(h) == twin.count
    for f in ("lifetime", "rotation", "size", "startLifetime"):
        assert d[f].tobytes() == h[f].tobytes(), f
    assert np.all(np.diff(d["lifetime"]) >= 0)                                   # the oldest first
    for f in ("velocity", "color", "randomSeed", "angularVelocity"):
        assert not d[f].any()                                                    # the rest of a record is zeroed
    if len(d) == 0:
        return 0.0
    err = np.abs(d["position"].astype(np.float64) - t["position"]) / t["bound"][:, None]
    assert err.max() <= 1.0, float(err.max())
    return float(err.max())


def mixed_dts(steps, base, seed):
    """The run's own dt with zeros, 0.1 s steps and random ones in between, and ONE step longer than every lifetime in the middle."""
    rng = np.random.default_rng(seed)
    dts = np.full(steps, base, dtype=np.float32)
    dts[3::10] = 0.0
    dts[7::10] = 0.1
    dts[5::17] = rng.uniform(0.0, 2.0 * base, size=len(dts[5::17]))
    dts[steps // 2] = 7.0
    return dts


@pytest.mark.parametrize("run", T.RUNS, ids=lambda r: f"rate{r[0]:g}_life{r[1]:g}_max{r[2]}")
def test_device_emitter_follows_the_host_emitter_step_by_step(eng, run):
    rate, lifetime, cap, steps, dt = run
    steps = max(steps, 320)
    kw = dict(rate=rate, lifetime=lifetime, max_particles=cap)
    host, dev = S.DemoEmitter(seed=7, **kw), S.DeviceEmitter(eng, seed=7, **kw)
    twin = T.EmitterTwin(dev.cfg)
    dts = mixed_dts(steps, dt, seed=cap)
    assert (dts == 0).any() and (dts > lifetime).sum() == 1
    worst, peak = 0.0, 0
    for i, step in enumerate(dts):
        n = host.step(step)
        assert dev.step(step) == n == twin.step(step) == dev.count(), i
        peak = max(peak, n)
        if i % 25 == 24 or i == steps - 1:
            worst = max(worst, check_against_host(dev, host, twin))
    print(f"device emitter vs twin: worst position error {worst:.3f} B; births {twin.next}, peak count {peak} of {cap}")
    assert twin.next > 2 * cap                                                   # the ring wrapped at least twice
    if cap == 100:
        assert peak == cap                                                       # this run saturates the cap
    dev.close(); host.close()


def test_generator_by_index_over_one_step_of_100000_births(eng):
    """Thread i of the step jumps the generator ahead by 3i: across wave and block boundaries, distances up to 3e5."""
    kw = dict(rate=3.0e6, lifetime=6.0, max_particles=1 << 17)
    host, dev = S.DemoEmitter(seed=123, **kw), S.DeviceEmitter(eng, seed=123, **kw)
    twin = T.EmitterTwin(dev.cfg)
    assert host.step(1 / 30) == dev.step(1 / 30) == twin.step(1 / 30) == 100000
    worst = check_against_host(dev, host, twin)
    print(f"100000 births in one step: worst position error {worst:.3f} B")
    d = dev.particles()
    assert len(np.unique(d["rotation"])) > 99000                                 # (and they are 100000 different draws)
    dev.close(); host.close()


def test_prewarm_gives_the_host_emitters_prewarmed_cloud(eng):
    host = S.DemoEmitter(seed=21, reserved=(C.c_int32 * 6)(1, 0, 0, 0, 0, 0))
    dev = S.DeviceEmitter(eng, seed=21, prewarm=True)
    twin = T.EmitterTwin(dev.cfg)
    assert dev.cfg.reserved[0] == 1 and 55 <= dev.count() <= 60
    assert dev.count() == E.lib().vp_emitter_count(host.h)
    check_against_host(dev, host, twin)
    for _ in range(5):                                                           # and it goes on from there like the host's
        assert dev.step(1 / 30) == host.step(1 / 30) == twin.step(1 / 30)
    check_against_host(dev, host, twin)
    dev.close(); host.close()


# ---- 6. whole frames without a host round trip ---------------------------------------------------------------------------------------------
def test_frames_fed_by_the_device_emitter_equal_frames_fed_through_the_host():
    sc, _, _ = S.make_demo_scene(width=160, height=120)
    dev, host = E.Engine(sc.config(device=0)), E.Engine(sc.config(device=0))
    em = S.DeviceEmitter(dev, seed=7, prewarm=True)
    for e in (dev, host):
        e.set_frame(sc.light_to_world, sc.grid_center)
    for _ in range(3):
        n = em.step(1 / 30)
        dev.upload_particles_from_emitter(em, sc.psys_local_to_world)
        img_d = frame(dev, sc)
        records = em.particles()
        assert len(records) == n and 55 <= n <= 60
        host.upload_particles(records, em.layout, sc.psys_local_to_world)
        img_h = frame(host, sc)
        occupied = assert_same_volume(dev, host, img_d, img_h)
        assert occupied >= 8 and dev.stats()["occupied_mv"] == occupied and dev.stats()["particles"] == n
        assert (img_d[..., 3] > 0.01).any()
    em.close(); dev.close(); host.close()


# ---- 7. ownership --------------------------------------------------------------------------------------------------------------------------
def test_emitters_belong_to_their_context():
    L = E.lib()
    sc = S.make_scene("T0")
    a, b = E.Engine(sc.config(device=0)), E.Engine(sc.config(device=0))
    e1, e2 = S.DeviceEmitter(a, seed=1, rate=100.0), S.DeviceEmitter(a, seed=2, rate=100.0)
    h1, h2 = S.DemoEmitter(seed=1, rate=100.0), S.DemoEmitter(seed=2, rate=100.0)
    for i in range(40):                                                          # two emitters of one context step independently
        assert e1.step(1 / 30) == h1.step(1 / 30)
        if i % 3 == 0:
            assert e2.step(0.1) == h2.step(0.1)
    p1, p2 = e1.particles(), e2.particles()
    assert p1["rotation"].tobytes() == h1.particles()["rotation"].tobytes() and p2["rotation"].tobytes() == h2.particles()["rotation"].tobytes()
    assert p1["lifetime"].tobytes() == h1.particles()["lifetime"].tobytes() and p1["rotation"].tobytes() != p2["rotation"].tobytes()
    # bad dt: refused, nothing changes
    for bad in (-0.1, float("nan"), float("inf")):
        assert L.vp_device_emitter_step(e1.h, C.c_float(bad)) == abi.VP_ERR_BAD_ARG
    assert e1.count() == len(p1) and e1.particles().tobytes() == p1.tobytes()
    # an emitter of context A is not context B's
    with pytest.raises(E.VpfxError) as ei:
        b.upload_particles_from_emitter(e1, sc.psys_local_to_world)
    assert ei.value.code == abi.VP_ERR_BAD_ARG
    a.upload_particles_from_emitter(e1, sc.psys_local_to_world)
    e2.close()                                                                   # one emitter destroyed before its context, one after
    a.close()
    buf = np.zeros(4, dtype=S.PARTICLE_DTYPE)
    lay = S.particle_layout()
    m = np.ascontiguousarray(sc.psys_local_to_world, dtype=np.float32)
    assert L.vp_device_emitter_step(e1.h, C.c_float(0.1)) == abi.VP_ERR_STATE
    assert L.vp_device_emitter_count(e1.h) == abi.VP_ERR_STATE
    assert L.vp_device_emitter_read_particles(e1.h, buf.ctypes.data_as(C.c_void_p), 4, C.byref(lay)) == abi.VP_ERR_STATE
    assert L.vp_upload_particles_from_emitter(b.h, e1.h, m.ctypes.data_as(C.c_void_p)) == abi.VP_ERR_STATE
    e1.close()                                                                   # frees the host part only; returns normally
    L.vp_device_emitter_destroy(None)
    b.close()
