"""Closed, welded, outward-oriented meshes for the inside / outside queries (cd_points_inside), and what the tests derive from them.
Every generator returns (verts float64 [nv, 3], faces uint32 [nf, 3]); a face is counter-clockwise seen from outside."""
import numpy as np


def box_grid(m: int = 4, lo=0.0, hi=1.0):
    """The surface of the cube [lo, hi]^3 with m x m quads a side, two triangles a quad, welded: 6 m^2 + 2 vertices, 12 m^2 faces.
    With lo = 0, hi = 1 and m a power of two every coordinate is i / m, exact."""
    index = {}
    verts = []

    def vid(ijk):
        if ijk not in index:
            index[ijk] = len(verts)
            verts.append([lo + (hi - lo) * (t / m) for t in ijk])
        return index[ijk]

    faces = []
    for c in range(3):
        a, b = (c + 1) % 3, (c + 2) % 3
        for side in (0, 1):
            for u in range(m):
                for v in range(m):
                    quad = []
                    for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):          # counter-clockwise seen from +c
                        ijk = [0, 0, 0]
                        ijk[a], ijk[b], ijk[c] = u + du, v + dv, side * m
                        quad.append(vid(tuple(ijk)))
                    if side == 0:
                        quad.reverse()
                    faces.append([quad[0], quad[1], quad[2]])
                    faces.append([quad[0], quad[2], quad[3]])
    return np.array(verts, dtype=np.float64), np.array(faces, dtype=np.uint32)


def torus(nu: int = 24, nv: int = 12, R: float = 1.0, r: float = 0.375):
    """A torus around the z axis, nu quads around the axis and nv around the tube: nu nv vertices, 2 nu nv faces."""
    u = 2.0 * np.pi * np.arange(nu) / nu
    v = 2.0 * np.pi * np.arange(nv) / nv
    uu, vv = np.meshgrid(u, v, indexing="ij")
    rho = R + r * np.cos(vv)
    verts = np.stack([rho * np.cos(uu), rho * np.sin(uu), r * np.sin(vv)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    p00, p10, p11, p01 = i * nv + j, i1 * nv + j, i1 * nv + j1, i * nv + j1
    faces = np.concatenate([np.stack([p00, p10, p11], axis=-1).reshape(-1, 3), np.stack([p00, p11, p01], axis=-1).reshape(-1, 3)])
    return np.ascontiguousarray(verts), faces.astype(np.uint32)


def torus_distance(points, R: float = 1.0, r: float = 0.375):
    """The signed distance to the smooth torus: negative inside the tube."""
    p = np.asarray(points, dtype=np.float64)
    return np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R) ** 2 + p[:, 2] ** 2) - r


def inverted(faces):
    """The same surface seen from the other side: every face reversed."""
    return np.ascontiguousarray(np.asarray(faces)[:, ::-1])


def nested_boxes(m: int = 4, invert_inner: bool = True):
    """The box [0, 1]^3 with the box [1/4, 3/4]^3 inside it, as ONE mesh; the inner shell inverted (a cavity) or not."""
    v0, f0 = box_grid(m)
    v1, f1 = box_grid(m, 0.25, 0.75)
    if invert_inner:
        f1 = inverted(f1)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + np.uint32(v0.shape[0])]).astype(np.uint32)


def open_box(m: int = 4):
    """box_grid(m) without its top (the side z = 1): an open mesh.  -> (verts, faces, removed faces)"""
    verts, faces = box_grid(m)
    top = (verts[faces][:, :, 2] == 1.0).all(axis=1)
    return verts, np.ascontiguousarray(faces[~top]), np.ascontiguousarray(faces[top])


def rotated(verts, shift=2.0 ** 20 + 0.37):
    """verts turned about a skew axis (no face stays axis-parallel) and moved by `shift` on every axis: inexact arithmetic."""
    ax = np.array([0.3, -0.5, 0.81])
    ax /= np.linalg.norm(ax)
    th = 0.7
    K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    Rm = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    return np.ascontiguousarray(np.asarray(verts) @ Rm.T + shift)


def signed_volume(verts, faces):
    """> 0 for an outward-oriented closed mesh."""
    t = np.asarray(verts)[np.asarray(faces)]
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def lattice(axis: int):
    """The 11^3 points {-1/8, ..., 9/8}^3 with the `axis` coordinate moved by 1/16: on the other two axes the points lie exactly under
    the m = 4 box's vertices, on its edges' projections and in the planes of its axis-parallel sides."""
    g = np.arange(-1, 10) / 8.0
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    p[:, axis] += 1.0 / 16.0
    return np.ascontiguousarray(p)


def lattice_inside(points, axis: int):
    """What the moved point (eps, eps^2 in (a, b)) says for the unit box: half-open on a and b, open on the column axis."""
    a, b = (axis + 1) % 3, (axis + 2) % 3
    p = points
    return (0 <= p[:, a]) & (p[:, a] < 1) & (0 <= p[:, b]) & (p[:, b] < 1) & (0 < p[:, axis]) & (p[:, axis] < 1)


def torus_points(n: int = 4000, seed: int = 11, margin: float = 0.05):
    """Uniform points in [-1.5, 1.5]^2 x [-0.6, 0.6], those kept whose distance to the smooth torus exceeds `margin` (the faceting
    error of the 24 x 12 torus is below 0.013).  -> (points, inside)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform([-1.5, -1.5, -0.6], [1.5, 1.5, 0.6], size=(n, 3))
    d = torus_distance(p)
    keep = np.abs(d) > margin
    return np.ascontiguousarray(p[keep]), d[keep] < 0
