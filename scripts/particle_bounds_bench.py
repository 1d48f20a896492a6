#!/usr/bin/env python3
"""What it costs per frame to know where a device-resident cloud is, on one GPU, at 100 000 and 1 000 000 device-emitter particles:

    bounds        vp_particle_bounds in the light's frame (one reduction kernel + one wait on the stream; 64 bytes come back)
    readback      what a host had to do before: vp_device_emitter_read_particles (pack, copy every record, rewrite them in the caller's
                  layout) followed by the numpy minimum / maximum of the spheres -- timed together and apart
    fit           vp_fit_grid on the box (host only)
    coverage      vp_particle_coverage after a bin of benchmark configuration C3 (100 000 particles, 32^3 metavoxels), with and without the
                  per-particle array

Every timed call starts after a vp_sync; the figures are medians over --steps calls after --warmup calls, in milliseconds.  Prints one
JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(eng, fn, warmup, steps):
    out = []
    for i in range(warmup + steps):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            out.append(t1 - t0)
    return round(float(np.median(out)) * 1e3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--counts", type=int, nargs="+", default=[100_000, 1_000_000])
    args = ap.parse_args()
    import __graft_entry__ as G
    G.load_package()
    from vpfx_amd import engine as E, scene as S
    import torch
    assert torch.cuda.is_available(), "the benchmark needs a GPU (there is no CPU fallback)"
    sc = S.make_scene("T0")                    # the grid plays no part in the bounds
    lifetime = 6.0
    light_frame = E.rigid_inverse(sc.light_to_world)
    out = {"steps": args.steps, "warmup": args.warmup, "results": {}}
    for count in args.counts:
        eng = E.Engine(sc.config(device=0))
        em = S.DeviceEmitter(eng, seed=7, prewarm=True, rate=1.05 * count / lifetime, lifetime=lifetime, max_particles=count)
        n = em.step(1.0 / 30.0)
        assert 0.99 * count <= n <= count, (n, count)
        eng.upload_particles_from_emitter(em, sc.psys_local_to_world)
        res = {"live": n}
        box = {}

        def bounds():
            box["b"] = eng.particle_bounds(light_frame)

        def readback():
            t0 = time.perf_counter()
            p = em.particles()
            t1 = time.perf_counter()
            h = np.abs(p["size"]) * np.float32(0.5)
            box["h"] = ((p["position"] - h[:, None]).min(axis=0), (p["position"] + h[:, None]).max(axis=0))
            box["split"] = (t1 - t0, time.perf_counter() - t1)

        res["bounds_ms"] = timed(eng, bounds, args.warmup, args.steps)
        splits = []

        def readback_split():
            readback()
            splits.append(box["split"])
        res["readback_ms"] = timed(eng, readback_split, args.warmup, args.steps)
        res["readback_copy_ms"] = round(float(np.median([s[0] for s in splits[args.warmup:]])) * 1e3, 4)
        res["readback_minmax_ms"] = round(float(np.median([s[1] for s in splits[args.warmup:]])) * 1e3, 4)
        b = box["b"]
        assert b["counted"] == n
        res["fit_ms"] = timed(eng, lambda: E.fit_grid(sc.light_to_world, b["sphere_min"], b["sphere_max"], (32, 32, 32), 3.0, 3.0 / 30.0),
                              args.warmup, args.steps)
        res["bytes_read_by_the_kernel"] = 16 * n
        em.close()
        eng.close()
        out["results"][str(count)] = res
    c3 = S.make_scene("C3")
    eng = E.Engine(c3.config(device=0))
    eng.set_frame(c3.light_to_world, c3.grid_center)
    eng.bin(c3.particles, c3.layout, c3.psys_local_to_world)
    cov = eng.particle_coverage()
    out["coverage_C3"] = {"ms": timed(eng, eng.particle_coverage, args.warmup, args.steps),
                          "with_per_particle_array_ms": timed(eng, lambda: eng.particle_coverage(per_particle=True), args.warmup, args.steps),
                          "bounds_ms": timed(eng, eng.particle_bounds, args.warmup, args.steps), **cov}
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
