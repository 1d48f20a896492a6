"""CPU: the host-only half of the particle queries -- `vp_fit_grid` against its float64 twin (tests/bounds_twin.py) and against the CPU
oracle's binning (a fitted grid loses no particle where the reference's own binning can keep them all), the layouts of the three result
records against a C99 program, and the resource budget of the kernels of csrc/particle_bounds.hip."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import bounds_twin as B
from oracle.oracle import Oracle
from vpfx_amd import abi, engine as E, scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "volumetric-particles-for-unity_amd", "csrc", "particle_bounds.hip")
FIT = E.lib().vp_fit_grid          # (a library without the particle queries has no such symbol: nothing here applies to it)
F = np.float32
S_MV = 3.0

LIGHTS = {
    "scene": S.to_colmajor16(S.trs((0.0, 0.0, -44.34), S.quat_to_matrix((0.185593992, 0.0, 0.0, 0.982626557)))),
    "identity": S.to_colmajor16(np.eye(4)),
    "tilted": S.to_colmajor16(S.trs((3.5, -12.25, 20.0), S.quat_to_matrix(np.array([0.3, -0.5, 0.2, 0.79]) / np.linalg.norm([0.3, -0.5, 0.2, 0.79])))),
}
BOXES = [((-4.0, -3.5, -2.25), (5.0, 1.5, 7.75)), ((17.3, -41.1, 5.9), (19.9, -35.2, 6.0)), ((-100.5, 80.25, -7.0), (-100.5, 80.25, -7.0))]


def raw_fit(l2w, lo, hi, n, s, snap, out=None):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
    l2w, lo, hi, n = arr(l2w, F), arr(lo, F), arr(hi, F), arr(n, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    fit = abi.vp_grid_fit() if out is None else out
    rc = FIT(p(l2w), p(lo), p(hi), p(n), C.c_float(s), C.c_float(snap), C.byref(fit) if fit is not False else None)
    return rc, fit


@pytest.mark.parametrize("N", [(1, 1, 1), (5, 5, 5), (6, 6, 6), (4, 5, 7)], ids=str)
@pytest.mark.parametrize("snap", [0.0, S_MV / 14.0], ids=["nosnap", "snap_s14"])
def test_fit_grid_equals_the_float64_twin(N, snap):
    for name, l2w in LIGHTS.items():
        for lo, hi in BOXES:
            got = E.fit_grid(l2w, lo, hi, N, S_MV, snap)
            want = B.fit(l2w, lo, hi, N, S_MV, snap)
            if snap > 0:                                   # the inputs keep the snapped quotient away from a tie
                sn = float(F(snap))
                q = ((np.asarray(lo, F).astype(float) + np.asarray(hi, F).astype(float)) / 2 + np.where(np.array(N) % 2 == 0, S_MV / 2, 0.0)) / sn
                assert np.all(np.abs(q - np.floor(q) - 0.5) > 1e-6), (name, lo, hi)
                assert np.all(np.abs(want["ls_center"] / sn - np.rint(want["ls_center"] / sn)) < 1e-9)       # on the lattice
            # computed in double and rounded once: equal to, or adjacent to, the float32 rounding of the twin
            for k in ("grid_center", "ls_center", "box_min", "box_max", "min_mv_scale"):
                assert B.within_one_ulp(got[k], want[k]), (name, lo, hi, k, got[k], want[k])
            assert (got["fits"], got["clipped"]) == (want["fits"], want["clipped"])
            # box_max - box_min = N s, up to the two roundings of the outputs (half an ulp of each bound)
            span = got["box_max"].astype(np.float64) - got["box_min"].astype(np.float64)
            slack = 0.5 * (np.spacing(np.abs(got["box_max"])) + np.spacing(np.abs(got["box_min"]))).astype(np.float64)
            assert np.all(np.abs(span - np.array(N) * S_MV) <= slack), (span, slack)
            # the centre sits where the integer N/2 origin puts it: box_min + (N/2 + 0.5) s
            assert np.allclose(want["ls_center"], want["box_min"] + (np.array(N) // 2 + 0.5) * S_MV, rtol=0, atol=1e-9)


def test_fit_grid_reports_what_sticks_out():
    l2w, N = LIGHTS["scene"], (4, 5, 6)
    # a box that fits exactly: N s wide on every axis
    lo = np.array([-1.0, 2.0, 10.0], dtype=F)
    hi = lo + np.array(N, dtype=F) * F(S_MV)
    fit = E.fit_grid(l2w, lo, hi, N, S_MV, 0.0)
    assert fit["fits"] == 1 and fit["clipped"] == 0 and fit["min_mv_scale"] == F(S_MV)
    assert np.array_equal(fit["box_min"], lo) and np.array_equal(fit["box_max"], hi)
    # one voxel wider than the grid on axis k: both sides stick out (the centre stays in the middle)
    for k in range(3):
        wide_hi = hi.copy()
        wide_hi[k] += F(1.0)
        fit = E.fit_grid(l2w, lo, wide_hi, N, S_MV, 0.0)
        assert fit["fits"] == 0 and fit["clipped"] == (1 << k) | (1 << (3 + k))
        assert fit["min_mv_scale"] > F(S_MV)
    # snapping moves the grid off the middle: a box that fitted exactly now sticks out of ONE chosen side.  Axis 0 (N = 4, even): the
    # unsnapped centre is lo + 2 s + s/2 = 6.5; snap 4 -> rint(1.625) * 4 = 8: the grid moved up, the low side sticks out.
    # Axis 1 (N = 5, odd): centre 2 + 7.5 = 9.5; snap 4 -> rint(2.375) * 4 = 8: the grid moved down, the high side sticks out.
    fit = E.fit_grid(l2w, lo, hi, N, S_MV, 4.0)
    want = B.fit(l2w, lo, hi, N, S_MV, 4.0)
    assert fit["ls_center"][0] == 8.0 and fit["ls_center"][1] == 8.0
    assert fit["clipped"] & 0b001001 == 0b000001 and fit["clipped"] & 0b010010 == 0b010000
    assert (fit["fits"], fit["clipped"]) == (want["fits"], want["clipped"]) and fit["fits"] == 0
    # min_mv_scale leaves room for the snap: (hi - lo + snap) / N
    assert B.within_one_ulp(fit["min_mv_scale"], max((float(hi[k] - lo[k]) + 4.0) / N[k] for k in range(3)))


def test_fit_grid_refusals():
    l2w, lo, hi, N = LIGHTS["scene"], (-1.0, -2.0, -3.0), (1.0, 2.0, 3.0), (5, 5, 5)
    assert raw_fit(l2w, lo, hi, N, S_MV, 0.0)[0] == 0
    untouched = abi.vp_grid_fit()
    untouched.fits = 77

    def refused(*args):
        rc, _ = raw_fit(*args, out=untouched)
        return rc == abi.VP_ERR_BAD_ARG and untouched.fits == 77          # a refused call writes nothing

    scaled = np.array(l2w, dtype=F); scaled[0:3] *= F(1.01)               # first column scaled by 1 %: rows off by > 1e-3
    sheared = np.array(l2w, dtype=F); sheared[4] += F(0.01)               # M(0, 1) += 0.01
    nan = np.array(l2w, dtype=F); nan[13] = np.nan
    inf = np.array(l2w, dtype=F); inf[5] = np.inf
    proj = np.array(l2w, dtype=F); proj[3] = F(0.5)                       # last row is not 0 0 0 1
    w2 = np.array(l2w, dtype=F); w2[15] = F(2.0)
    for bad in (scaled, sheared, nan, inf, proj, w2):
        assert refused(bad, lo, hi, N, S_MV, 0.0)
    nearly = np.array(l2w, dtype=F); nearly[0:3] *= F(1.0002)            # within the 1e-3 tolerance: accepted
    assert raw_fit(nearly, lo, hi, N, S_MV, 0.0)[0] == 0
    assert refused(l2w, (2.0, -2.0, -3.0), hi, N, S_MV, 0.0)              # lo > hi
    assert refused(l2w, (np.nan, -2.0, -3.0), hi, N, S_MV, 0.0)
    assert refused(l2w, lo, (1.0, np.inf, 3.0), N, S_MV, 0.0)
    assert refused(l2w, (-np.inf, -2.0, -3.0), hi, N, S_MV, 0.0)
    assert refused(l2w, lo, hi, (5, 0, 5), S_MV, 0.0) and refused(l2w, lo, hi, (5, 5, -1), S_MV, 0.0)
    for bad_s in (0.0, -3.0, np.nan, np.inf):
        assert refused(l2w, lo, hi, N, bad_s, 0.0)
    for bad_snap in (-0.1, np.nan, np.inf):
        assert refused(l2w, lo, hi, N, S_MV, bad_snap)
    for i in range(4):                                                    # null pointers
        args = [l2w, lo, hi, N]
        args[i] = None
        assert refused(*args, S_MV, 0.0)
    assert raw_fit(l2w, lo, hi, N, S_MV, 0.0, out=False)[0] == abi.VP_ERR_BAD_ARG
    assert b"vp_fit_grid" in E.lib().vp_last_error(None)


# ---- the fit rule against the CPU oracle's binning -----------------------------------------------------------------------------------------
def drifted_scene(N, size_range):
    sc = S.make_scene(dims=(N, 16, 600, 64, 64), size_range=size_range)
    sc.particles["position"] = (sc.particles["position"].astype(np.float64) * 0.9 + np.array([7.3, -4.1, 5.9])).astype(F)
    return sc


def light_space_box64(sc):
    """The spheres' box in the light's local space, in float64, rounded OUTWARD to float32."""
    L = B.rows_of(sc.light_to_world).astype(np.float64)
    inv = np.linalg.inv(L)
    pos = sc.particles["position"].astype(np.float64)                      # the system's localToWorld is the identity
    ls = pos @ inv[:3, :3].T + inv[:3, 3]
    h = sc.particles["size"].astype(np.float64)[:, None] / 2.0
    lo, hi = (ls - h).min(axis=0), (ls + h).max(axis=0)
    lo32, hi32 = lo.astype(F), hi.astype(F)
    lo32 = np.where(lo32 > lo, np.nextafter(lo32, F(-np.inf)), lo32)
    hi32 = np.where(hi32 < hi, np.nextafter(hi32, F(np.inf)), hi32)
    return lo32, hi32


def oracle_uncovered(sc, grid_center):
    orc = Oracle(sc.config())
    orc.set_frame(sc.light_to_world, grid_center)
    orc.bin(sc.particles, sc.layout, sc.psys_local_to_world)
    lists, _ = B.lists_of(orc)
    cov, _ = B.coverage(len(sc.particles), lists, np.ones(len(sc.particles), dtype=bool))
    orc.close()
    return cov["uncovered"]


@pytest.mark.parametrize("snap", [0.0, S_MV / 14.0], ids=["nosnap", "snap_s14"])
@pytest.mark.parametrize("N,size_range", [(5, (1.2, 1.4)), (5, (0.6, 1.4)), (5, (0.1, 0.3)), (6, (1.2, 1.4))], ids=str)
def test_a_fitted_grid_loses_no_particle_in_the_oracles_binning(N, size_range, snap):
    sc = drifted_scene(N, size_range)
    lo, hi = light_space_box64(sc)
    fit = E.fit_grid(sc.light_to_world, lo, hi, sc.N, sc.mv_scale, snap)
    assert fit["fits"] == 1 and fit["clipped"] == 0
    left_at_origin = oracle_uncovered(sc, np.zeros(3, dtype=F))
    fitted = oracle_uncovered(sc, fit["grid_center"])
    print(f"N = {N}, sizes {size_range} s, snap {snap:.4f}: uncovered {left_at_origin} of 600 with the grid at the origin, {fitted} fitted")
    assert left_at_origin > 100
    assert fitted == 0


@pytest.mark.parametrize("snap", [0.0, S_MV / 14.0], ids=["nosnap", "snap_s14"])
def test_even_grids_still_drop_small_particles_q1_q2(snap):
    """Reference quirks Q1 / Q2 (integer N/2 origin against float binning, VPR.cs:388 / 422-438): with an even metavoxel count a particle
    smaller than half a metavoxel is looked up in ONE candidate cell and is lost in the upper half of it.  The fit cannot help (the box
    fits); this is why coverage is a call of its own."""
    sc = drifted_scene(6, (0.1, 0.3))
    lo, hi = light_space_box64(sc)
    fit = E.fit_grid(sc.light_to_world, lo, hi, sc.N, sc.mv_scale, snap)
    assert fit["fits"] == 1
    dropped = oracle_uncovered(sc, fit["grid_center"])
    print(f"N = 6, sizes (0.1, 0.3) s, snap {snap:.4f}: the oracle drops {dropped} of 600 on a grid that contains them")
    assert dropped > 0


# ---- layouts and budget -------------------------------------------------------------------------------------------------------------------
def test_result_record_layouts_match_a_c99_program():
    fields = {"vp_particle_bounds": ("struct vp_particle_bounds", abi.vp_particle_bounds),
              "vp_particle_coverage": ("struct vp_particle_coverage", abi.vp_particle_coverage),
              "vp_grid_fit": ("vp_grid_fit", abi.vp_grid_fit)}
    lines, mirror = [], []
    for name, (ctype, mir) in fields.items():
        lines.append(f'printf("%zu\\n", sizeof({ctype}));')
        mirror.append(C.sizeof(mir))
        for f, _ in mir._fields_:
            lines.append(f'printf("%zu\\n", offsetof({ctype}, {f}));')
            mirror.append(getattr(mir, f).offset)
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "vpfx.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out == mirror
    assert (C.sizeof(abi.vp_particle_bounds), C.sizeof(abi.vp_particle_coverage), C.sizeof(abi.vp_grid_fit)) == (64, 32, 64)


def test_particle_query_kernels_fit_the_budget():
    """No scratch, VGPR + AGPR <= 64 (the device emitter's standard), read the way tests/test_device_emitter_cpu.py reads it."""
    flags = open(os.path.join(os.path.dirname(SRC), "Makefile")).read()
    assert "particle_bounds.o" in flags
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", flags, flags=re.M).group(1).replace("--offload-arch=$(ARCH)", "--offload-arch=gfx950").replace("$(EXTRA)", "").split()
    assert "-ffp-contract=off" in flags and "-O3" in flags
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-c", SRC, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    names = [b.split()[0] for b in blocks]
    for k in ("k_bounds_init", "k_bounds", "k_cover_count", "k_cover_reduce"):
        assert any(k in n for n in names), (k, names)
    for b in blocks:
        vgpr = int(re.search(r"VGPRs: (\d+)", b).group(1))
        agpr = int(re.search(r"AGPRs: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        print(b.split()[0], "VGPRs", vgpr, "AGPRs", agpr, "scratch", scratch)
        assert scratch == 0 and vgpr + agpr <= 64, (b.split()[0], vgpr, agpr, scratch)
    assert "fmaf" not in re.sub(r"//[^\n]*", "", open(SRC).read())        # -ffp-contract=off and no written FMA: the twin's operations
