"""column_tri and cd_points_inside restated in numpy (csrc/cd_math.h, csrc/cd_inside.h): FP64, the operation order
of the device function, every difference, product and sum a numpy operation of its own (no contraction).  The per-point sums are brute
force over all faces."""
import numpy as np


def _edge(la, lb, ha, hb, pa, pb):
    """The directed edge l -> h: (E, sign).  sign: that of E where E != 0, else of l_b - h_b, else of h_a - l_a, else 0; a NaN E: 0."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        E = (la - pa) * (hb - pb) - (lb - pb) * (ha - pa)
        tie = np.where(lb > hb, 1, np.where(lb < hb, -1, np.where(ha > la, 1, np.where(ha < la, -1, 0))))
        s = np.where(E > 0, 1, np.where(E < 0, -1, np.where(E == 0, tie, 0)))
    return E, s


def column_tri(p, tri, axis):
    """p [..., 3] against tri [..., 3, 3] (broadcast together) -> dict(cover int8, counted, above bool, E [..., 3], zc, S)."""
    p = np.asarray(p, dtype=np.float64)
    t = np.asarray(tri, dtype=np.float64)
    c, a, b = axis, (axis + 1) % 3, (axis + 2) % 3
    pa, pb, pc = p[..., a], p[..., b], p[..., c]
    va, vb, vc = t[..., a], t[..., b], t[..., c]                               # [..., 3]: the three vertices
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        gate = ((va <= pa[..., None]).any(-1) & (va >= pa[..., None]).any(-1) & (vb <= pb[..., None]).any(-1) & (vb >= pb[..., None]).any(-1))
        E0, s0 = _edge(va[..., 1], vb[..., 1], va[..., 2], vb[..., 2], pa, pb)
        E1, s1 = _edge(va[..., 2], vb[..., 2], va[..., 0], vb[..., 0], pa, pb)
        E2, s2 = _edge(va[..., 0], vb[..., 0], va[..., 1], vb[..., 1], pa, pb)
        z0, z1, z2 = vc[..., 0] - pc, vc[..., 1] - pc, vc[..., 2] - pc
        S = (E0 + E1) + E2
        zc = (E0 * z0 + E1 * z1) + E2 * z2
        o = np.where((s0 > 0) & (s1 > 0) & (s2 > 0), 1, np.where((s0 < 0) & (s1 < 0) & (s2 < 0), -1, 0))
        o = np.where(gate, o, 0).astype(np.int8)
        counted = (o != 0) & ((S > 0) | (S < 0)) & (zc == zc)
        above = counted & (((zc > 0) & (S > 0)) | ((zc < 0) & (S < 0)))
    return dict(cover=o, counted=counted, above=above, E=np.stack([E0, E1, E2], axis=-1), zc=zc, S=S)


def points_inside(points, verts, faces, axis, parity=False, chunk=256):
    """-> (inside bool, n_above u32, n_below u32, w_above i32, w_below i32) over ALL faces for every point."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(verts, dtype=np.float64)[np.asarray(faces).astype(np.int64)]   # [nf, 3, 3]
    n = p.shape[0]
    na, nb = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    wa, wb = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for s in range(0, n, chunk):
        r = column_tri(p[s:s + chunk, None, :], t[None, :, :, :], axis)
        up, dn, o = r["above"], r["counted"] & ~r["above"], r["cover"].astype(np.int32)
        na[s:s + chunk] = up.sum(axis=1)
        nb[s:s + chunk] = dn.sum(axis=1)
        wa[s:s + chunk] = (o * up).sum(axis=1)
        wb[s:s + chunk] = (o * dn).sum(axis=1)
    inside = (na & 1) != 0 if parity else wa != 0
    return inside, na, nb, wa, wb
