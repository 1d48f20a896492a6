#!/usr/bin/env python3
"""Mesh-occluder timings on the GPU: the light depth map at C3's size (32 x 32 metavoxels x 32 voxels = 1024^2 texels) and the eye depth map at
1920 x 1080, rendered from
    demo_solids    the DEMO scene's 8 occluders as analytic solids (4 boxes, 4 capped cylinders)            -- the path without meshes
    demo_meshes    the same 8 as triangle meshes (Unity's Cube: 12 triangles, Cylinder: 20-sided prism, 80)
    tris_10k       8 icospheres of 1 280 triangles (10 240 instanced triangles)
    tris_1M        50 icospheres of 20 480 triangles (1 024 000 instanced triangles)
    no_occluders   nothing: what the two calls cost without any occluder (render of a cleared map + read-back)
Each number is the mean wall time of vp_render_light_depth / vp_render_scene_depth after a warm-up: the render plus the read-back of the map
(4 MiB / 8 MiB) and, for meshes, the one host wait of the binning.  The per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script.  Prints one JSON line per case.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    import __graft_entry__ as G
    G.load_package()
    from vpfx_amd import abi, engine as E, scene as S
    import torch
    assert torch.cuda.is_available(), "the benchmark needs a GPU (there is no CPU fallback)"
    reps = int(os.environ.get("MESH_BENCH_REPS", "20"))
    sc = S.make_scene("mesh_bench", dims=(32, 32, 10, 1920, 1080))
    _, _, demo = S.make_demo_scene(width=64, height=48)
    cube, prism = S.unity_cube_mesh(), S.prism_mesh(20)
    demo_inst = []
    for s in demo:
        A = np.asarray(list(s.axes), dtype=np.float64).reshape(3, 3)
        h = np.asarray(list(s.half_extent), dtype=np.float64)
        if s.type == abi.VP_OCC_BOX:
            demo_inst.append(S.make_instance(0, S.box_instance_matrix(s)))
        else:                                                   # prism of radius 0.5, half height 1: scale (2 hx, hy, 2 hz)
            demo_inst.append(S.make_instance(1, S.trs(list(s.center), np.linalg.inv(A), (2 * h[0], h[1], 2 * h[2]))))
    rng = np.random.default_rng(9)
    D = sc.N[0] * sc.mv_scale

    def spheres(n, sub):
        return [S.icosphere_mesh(sub)], [S.make_instance(0, S.trs(rng.uniform(-0.3 * D, 0.3 * D, 3), np.eye(3), rng.uniform(2.0, 8.0, 3)))
                                         for _ in range(n)]
    cases = [("no_occluders", None, []), ("demo_solids", None, None), ("demo_meshes", [cube, prism], demo_inst), ("tris_10k",) + spheres(8, 3), ("tris_1M",) + spheres(50, 5)]
    cam = sc.camera()
    for name, meshes, inst in cases:
        e = E.Engine(sc.config())
        e.set_frame(sc.light_to_world, sc.grid_center)
        ntri = 0
        if meshes is None and inst is None:
            e.set_occluders(demo)
        elif meshes is None:
            pass                                                # the render + read-back floor
        else:
            e.set_occluder_meshes(meshes)
            e.set_occluder_instances(inst)
            ntri = sum(len(meshes[i.mesh][1]) for i in inst)
        out = {"case": name, "instanced_triangles": ntri}
        for view, fn in (("light_1024sq", lambda: e.render_light_depth()), ("eye_1080p", lambda: e.render_scene_depth(cam))):
            for _ in range(3):
                m = fn()
            t0 = time.perf_counter()
            for _ in range(reps):
                m = fn()
            out[view + "_ms"] = round((time.perf_counter() - t0) / reps * 1e3, 4)
            out[view + "_covered"] = round(float((m < (1.0 if view.startswith("light") else 1e30)).mean()), 4)
        print(json.dumps(out), flush=True)
        e.close()


if __name__ == "__main__":
    main()
