"""Float64 reference ray caster for the mesh occluders (test infrastructure).

Same rays as the library's depth maps (occluders.hip / occluder_mesh.hip): pixel-centre rays of the ortho light camera (VPR.cs:338-342, 365) and
of the main camera, same depth definitions, same culling (light: faces turned away from the light, Cull Front; eye: faces turned towards the
camera, Cull Back; outward normal = sign(det M) * Cross(b - a, c - a)).  Besides the depth it reports, per pixel, how close (in pixels) the
centre lies to a projected triangle edge -- where fp32 and fp64 may disagree about a hit -- both for any edge and for silhouette edges only.
"""
import math

import numpy as np


def world_triangles(meshes, instances):
    """[(a, b, c, edge keys)] in world space (float64), mirrored instances rewound so that Cross(b - a, c - a) points outward."""
    out = []
    for ii, inst in enumerate(instances):
        m = np.asarray(list(inst.object_to_world), dtype=np.float64).reshape(4, 4).T      # column-major -> row-major
        pos, tri = meshes[inst.mesh]
        det = np.linalg.det(m[:3, :3])
        if det == 0.0:
            continue
        w = np.asarray(pos, dtype=np.float64) @ m[:3, :3].T + m[:3, 3]
        tri = np.asarray(tri, dtype=np.int64)
        if det < 0:
            tri = tri[:, [0, 2, 1]]
        out.append((w, tri, ii))
    return out


class View:
    """Pixel-centre rays of one map.  kind = 'light' (ortho) or 'eye' (perspective)."""

    @staticmethod
    def light(sc, near=0.3, far=1000.0, cam_distance=200.0):
        v = View()
        v.kind = "light"
        L = np.asarray(sc.light_to_world, dtype=np.float64).reshape(4, 4).T
        R = L[:3, :3]
        f = R[:, 2] / np.linalg.norm(R[:, 2])
        v.W, v.H = sc.N[0] * sc.nv, sc.N[1] * sc.nv
        r, t = sc.N[0] * sc.mv_scale * 0.5, sc.N[1] * sc.mv_scale * 0.5
        X, Y = np.meshgrid(np.arange(v.W), np.arange(v.H))
        lx = -r + (X + 0.5) / v.W * (2 * r)
        ly = -t + (Y + 0.5) / v.H * (2 * t)
        c = np.asarray(sc.grid_center, dtype=np.float64) - f * cam_distance
        v.o = c + lx[..., None] * R[:, 0] + ly[..., None] * R[:, 1]
        v.d = np.broadcast_to(f, v.o.shape)
        v.near, v.far = near, far
        inv = np.linalg.inv(np.stack([R[:, 0], R[:, 1], f], 1))
        v.project = lambda p: np.stack([((inv[0] @ (p - c).T) + r) / (2 * r) * v.W - 0.5, ((inv[1] @ (p - c).T) + t) / (2 * t) * v.H - 0.5], -1)
        v.facing = lambda a, n: n @ f > 0                      # back faces only (Cull Front)
        v.depth = lambda tt: (tt - near) / (far - near)
        v.clear = 1.0
        return v

    @staticmethod
    def eye(sc, cam):
        v = View()
        v.kind = "eye"
        v.W, v.H = sc.width, sc.height
        m = np.asarray(list(cam.camera_to_world), dtype=np.float64).reshape(4, 4).T
        C3, o = m[:3, :3], m[:3, 3]
        aspect, nit = v.W / v.H, -1.0 / math.tan(float(cam.fov_y) * 0.5)
        X, Y = np.meshgrid(np.arange(v.W), np.arange(v.H))
        e = np.stack([(2 * (X + 0.5) / v.W - 1) * aspect, 2 * (Y + 0.5) / v.H - 1, np.full(X.shape, nit)], -1)
        v.d = e @ C3.T
        v.o = np.broadcast_to(o, v.d.shape)
        v.near = float(cam.near_clip)
        v.far = float(cam.far_clip) if cam.far_clip > 0 else 3e38
        inv = np.linalg.inv(C3)

        def project(p):
            q = (p - o) @ inv.T
            dep = -q[:, 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                ex, ey = q[:, 0] * (-nit) / dep, q[:, 1] * (-nit) / dep
            xy = np.stack([(ex / aspect + 1) * v.W * 0.5 - 0.5, (ey + 1) * v.H * 0.5 - 0.5], -1)
            xy[dep <= 0] = np.nan
            return xy
        v.project = project
        v.facing = lambda a, n: np.einsum("ij,ij->i", n, a - o) < 0      # front faces only (Cull Back)
        v.depth = lambda tt: tt * (-nit)
        v.clear = np.float32(3e38)
        v.nit = nit
        return v


def _seg_dist(px, py, x0, y0, x1, y1):
    dx, dy = x1 - x0, y1 - y0
    L2 = dx * dx + dy * dy
    s = np.clip(((px - x0) * dx + (py - y0) * dy) / np.where(L2 > 0, L2, 1), 0, 1)
    return np.hypot(px - (x0 + s * dx), py - (y0 + s * dy))


def render(view, meshes, instances, edge_tol=1e-3):
    """-> (depth [H, W] float64 in the map's encoding, near_any_edge [H, W] bool, near_silhouette [H, W] bool)."""
    with np.errstate(all="ignore"):                          # rays parallel to a triangle: t = inf / nan, rejected by the tests below
        return _render(view, meshes, instances, edge_tol)


def _render(view, meshes, instances, edge_tol):
    H, W = view.H, view.W
    best_t = np.full((H, W), np.inf)
    near_any = np.zeros((H, W), bool)
    near_sil = np.zeros((H, W), bool)
    for w, tri, _ in world_triangles(meshes, instances):
        a, b, c = w[tri[:, 0]], w[tri[:, 1]], w[tri[:, 2]]
        n = np.cross(b - a, c - a)
        keep = view.facing(a, n)
        # silhouette edges: used by exactly one kept triangle of this instance
        edges = {}
        for k, (i0, i1, i2) in enumerate(tri):
            if not keep[k]:
                continue
            for e in ((i0, i1), (i1, i2), (i2, i0)):
                key = (min(e), max(e))
                edges[key] = edges.get(key, 0) + 1
        pxy = view.project(w)
        for k in np.nonzero(keep)[0]:
            ids = tri[k]
            P = pxy[ids]
            if np.isnan(P).any():
                x0, x1, y0, y1 = 0, W - 1, 0, H - 1
            else:
                x0, x1 = max(0, int(math.floor(P[:, 0].min())) - 1), min(W - 1, int(math.ceil(P[:, 0].max())) + 1)
                y0, y1 = max(0, int(math.floor(P[:, 1].min())) - 1), min(H - 1, int(math.ceil(P[:, 1].max())) + 1)
            if x0 > x1 or y0 > y1:
                continue
            o = view.o[y0:y1 + 1, x0:x1 + 1].reshape(-1, 3)
            d = view.d[y0:y1 + 1, x0:x1 + 1].reshape(-1, 3)
            A, B, Cc, N = a[k], b[k], c[k], n[k]
            nd = d @ N
            with np.errstate(divide="ignore", invalid="ignore"):
                t = ((A - o) @ N) / nd
            p = o + t[:, None] * d
            inside = (np.cross(B - A, p - A) @ N >= 0) & (np.cross(Cc - B, p - B) @ N >= 0) & (np.cross(A - Cc, p - Cc) @ N >= 0) & (nd != 0)
            if view.kind == "light":
                ok = inside & (t >= view.near) & (t <= view.far)
            else:
                dep = t * (-view.nit)
                ok = inside & (t > 0) & (dep >= view.near) & (dep <= view.far)
            sub = best_t[y0:y1 + 1, x0:x1 + 1].reshape(-1)
            sub[ok] = np.minimum(sub[ok], t[ok])
            best_t[y0:y1 + 1, x0:x1 + 1] = sub.reshape(y1 - y0 + 1, x1 - x0 + 1)
            if np.isnan(P).any():
                continue
            X, Y = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1))
            for e0, e1 in ((0, 1), (1, 2), (2, 0)):
                dist = _seg_dist(X, Y, P[e0, 0], P[e0, 1], P[e1, 0], P[e1, 1]) <= edge_tol
                near_any[y0:y1 + 1, x0:x1 + 1] |= dist
                if edges[(min(ids[e0], ids[e1]), max(ids[e0], ids[e1]))] == 1:
                    near_sil[y0:y1 + 1, x0:x1 + 1] |= dist
    depth = np.where(np.isfinite(best_t), view.depth(np.where(np.isfinite(best_t), best_t, 0.0)), view.clear)
    return depth, near_any, near_sil


def sample(view, meshes, instances, pixels, edge_tol=1e-3):
    """The reference at a few pixels only ([(X, Y)]), vectorised over every triangle: -> (depth [n], near_any_edge [n])."""
    with np.errstate(all="ignore"):
        return _sample(view, meshes, instances, pixels, edge_tol)


def _sample(view, meshes, instances, pixels, edge_tol):
    tris = [(w[t[:, 0]], w[t[:, 1]], w[t[:, 2]]) for w, t, _ in world_triangles(meshes, instances)]
    a = np.concatenate([x[0] for x in tris]); b = np.concatenate([x[1] for x in tris]); c = np.concatenate([x[2] for x in tris])
    n = np.cross(b - a, c - a)
    keep = view.facing(a, n)
    a, b, c, n = a[keep], b[keep], c[keep], n[keep]
    pa, pb, pc = view.project(a), view.project(b), view.project(c)
    out, near = [], []
    for X, Y in pixels:
        o, d = view.o[Y, X], view.d[Y, X]
        nd = n @ d
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.einsum("ij,ij->i", a - o, n) / nd
        p = o + t[:, None] * d
        inside = ((np.einsum("ij,ij->i", np.cross(b - a, p - a), n) >= 0) & (np.einsum("ij,ij->i", np.cross(c - b, p - b), n) >= 0)
                  & (np.einsum("ij,ij->i", np.cross(a - c, p - c), n) >= 0) & (nd != 0))
        if view.kind == "light":
            ok = inside & (t >= view.near) & (t <= view.far)
        else:
            ok = inside & (t > 0) & (t * (-view.nit) >= view.near) & (t * (-view.nit) <= view.far)
        out.append(view.depth(t[ok].min()) if ok.any() else view.clear)
        dist = np.minimum(np.minimum(_seg_dist(X, Y, pa[:, 0], pa[:, 1], pb[:, 0], pb[:, 1]), _seg_dist(X, Y, pb[:, 0], pb[:, 1], pc[:, 0], pc[:, 1])),
                          _seg_dist(X, Y, pc[:, 0], pc[:, 1], pa[:, 0], pa[:, 1]))
        near.append(bool((dist <= edge_tol).any()))
    return np.asarray(out, dtype=np.float64), np.asarray(near)
