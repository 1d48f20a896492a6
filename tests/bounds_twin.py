"""Test infrastructure: numpy restatements of the particle queries (include/vpfx.h "where the resident particles are").

  world_particles  what the upload's extract leaves on the device: world position (float32, the association of k_extract) + size
  bounds           vp_particle_bounds: float32, f_r = ((M(r,0) x + M(r,1) y) + M(r,2) z) + M(r,3), h = |size| * 0.5, exact min / max
  coverage         vp_particle_coverage rebuilt from bin lists
  fit              vp_fit_grid in float64

numpy multiplies and adds float32 arrays in float32 without contraction, so `bounds` is the library's result bit for bit (up to the sign of
a zero, which `==` does not see)."""
import numpy as np

F = np.float32


def rows_of(m16):
    """Column-major 16 floats -> (row, col) float32 matrix."""
    return np.ascontiguousarray(m16, dtype=F).reshape(4, 4).T


def transform32(m16, xyz):
    """MultiplyPoint3x4 in float32: ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 for r = 0..2."""
    m = rows_of(m16)
    x, y, z = (np.ascontiguousarray(xyz[:, k], dtype=F) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):                  # non-finite inputs are the caller's business
        return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1)


def world_particles(position, size, psys_local_to_world):
    """[P, 4] float32: (world xyz, size) as the extract kernel writes them."""
    ws = np.empty((len(position), 4), dtype=F)
    ws[:, :3] = transform32(psys_local_to_world, np.asarray(position, dtype=F))
    ws[:, 3] = np.asarray(size, dtype=F)
    return ws


IDENTITY = np.eye(4, dtype=F).reshape(16)


def bounds(ws, world_to_frame=None):
    ws = np.asarray(ws, dtype=F).reshape(-1, 4)
    finite = np.isfinite(ws).all(axis=1)
    w = ws[finite]
    out = dict(counted=int(finite.sum()), skipped=int((~finite).sum()), max_radius=F(0.0))
    inf = np.full(3, np.inf, dtype=F)
    out.update(center_min=inf.copy(), center_max=-inf, sphere_min=inf.copy(), sphere_max=-inf.copy())
    if len(w):
        f = transform32(IDENTITY if world_to_frame is None else world_to_frame, w[:, :3])
        h = np.abs(w[:, 3]) * F(0.5)
        assert f.dtype == F and h.dtype == F
        out.update(center_min=f.min(axis=0), center_max=f.max(axis=0), sphere_min=(f - h[:, None]).min(axis=0),
                   sphere_max=(f + h[:, None]).max(axis=0), max_radius=h.max())
    return out


def assert_bounds_equal(got, want):
    """All 13 floats with ==, both counters equal."""
    for k in ("center_min", "center_max", "sphere_min", "sphere_max"):
        assert np.asarray(got[k]).dtype == F
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert F(got["max_radius"]) == want["max_radius"], (got["max_radius"], want["max_radius"])
    assert (got["counted"], got["skipped"]) == (want["counted"], want["skipped"])


def lists_of(eng):
    """{(xx, yy, zz): ids} of every non-empty metavoxel list, through the bin's own probes (engine or oracle)."""
    counts = eng.bin_counts()
    return {(int(xx), int(yy), int(zz)): eng.bin_list(xx, yy, zz) for zz, yy, xx in np.argwhere(counts > 0)}, counts


def coverage(n_particles, lists, finite):
    per = np.zeros(n_particles, dtype=np.int32)
    for ids in lists.values():
        assert len(np.unique(ids)) == len(ids)
        per[ids] += 1
    finite = np.asarray(finite, dtype=bool)
    assert not per[~finite].any()
    return dict(particles=n_particles, covered=int((per > 0).sum()), uncovered=int(((per == 0) & finite).sum()), skipped=int((~finite).sum()),
                pairs=int(per.sum()), max_mv_per_particle=int(per.max()) if n_particles else 0), per


def fit(light_to_world, lo, hi, num_mv, s, snap):
    """vp_fit_grid in float64.  Metavoxel xx is centred at lsO + (xx - N/2) s with integer N/2 (VPR.cs:370-394)."""
    L = rows_of(light_to_world).astype(np.float64)
    lo, hi = np.asarray(lo, dtype=F).astype(np.float64), np.asarray(hi, dtype=F).astype(np.float64)
    s, snap = float(F(s)), float(F(snap))
    c, bmin, bmax, clipped, need = np.zeros(3), np.zeros(3), np.zeros(3), 0, 0.0
    for k in range(3):
        n = int(num_mv[k])
        c[k] = (lo[k] + hi[k]) / 2.0 + (s / 2.0 if n % 2 == 0 else 0.0)
        if snap > 0.0:
            c[k] = np.rint(c[k] / snap) * snap
        bmin[k] = c[k] - (n // 2 + 0.5) * s
        bmax[k] = bmin[k] + n * s
        clipped |= (1 << k) if lo[k] < bmin[k] else 0
        clipped |= (1 << (3 + k)) if hi[k] > bmax[k] else 0
        need = max(need, (hi[k] - lo[k] + snap) / n)
    gc = np.array([((L[r, 0] * c[0] + L[r, 1] * c[1]) + L[r, 2] * c[2]) + L[r, 3] for r in range(3)])
    return dict(grid_center=gc, ls_center=c, box_min=bmin, box_max=bmax, min_mv_scale=need, fits=int(clipped == 0), clipped=clipped)


def within_one_ulp(got32, want64):
    """got32 equals the float32 rounding of want64 or one of its two float32 neighbours."""
    got32, r = np.asarray(got32, dtype=F), np.asarray(want64, dtype=np.float64).astype(F)
    return bool(np.all((got32 == r) | (got32 == np.nextafter(r, F(np.inf))) | (got32 == np.nextafter(r, F(-np.inf)))))
