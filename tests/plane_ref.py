"""The plane queries restated on the CPU (no test in here): plane_tri (csrc/cd_math.h) in numpy with the same operation order, bit for
bit in every output; cd_planes_cut_all and cd_planes_count by brute force -- every plane against EVERY triangle, no box of any kind --
what the segments of a plane add up to (loops, enclosed area), and the planes and meshes the CPU and GPU tests share.

A plane is four doubles {nx, ny, nz, d}: n . x = d.  A row set is sorted by (plane, face), the order the comparisons use (the device's
order is free)."""
from __future__ import annotations

import collections
import functools

import numpy as np

import closed_meshes as cm
import scale_inputs as si
import within_ref as wr

ABOVE, BELOW, CUT = 0, 1, 2
PlaneRows = collections.namedtuple("PlaneRows", "rows ids seg edge t on")


# ---------------------------------------------------------------- the predicate
def side(pl, p):
    """The vertex value s = ((nx x + ny y) + nz z) - d on broadcastable operands; the vertex is below iff s < 0."""
    with np.errstate(all="ignore"):
        return ((pl[0] * p[0] + pl[1] * p[1]) + pl[2] * p[2]) - pl[3]


def _edge_point(L, sl, U, su):
    """The point of an edge whose ends differ in "below" (L the below end): U itself and t = 1 where s_U == 0, else L + t (U - L)."""
    with np.errstate(all="ignore"):
        t = sl / (sl - su)
        pt = tuple(L[a] + t * (U[a] - L[a]) for a in range(3))
    at_u = su == 0.0
    return tuple(np.where(at_u, U[a], pt[a]) for a in range(3)), np.where(at_u, 1.0, t)


def _core(pl, P):
    """plane_tri on broadcastable operands.  pl: (nx, ny, nz, d); P: three vertices, each (x, y, z).
    -> cls, a (x, y, z), b (x, y, z), edge_a, edge_b, t_a, t_b, on"""
    s = [side(pl, p) for p in P]
    below = [x < 0.0 for x in s]
    shape = np.broadcast(*s).shape
    on = np.zeros(shape, dtype=np.uint8)
    for i in range(3):
        on |= ((s[i] == 0.0).astype(np.uint8) << i).astype(np.uint8)
    nb = below[0].astype(np.int8) + below[1] + below[2]
    cls = np.where(nb == 3, BELOW, np.where(nb == 0, ABOVE, CUT)).astype(np.uint8)
    a = [np.zeros(shape) for _ in range(3)]
    b = [np.zeros(shape) for _ in range(3)]
    ea, eb = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    ta, tb = np.zeros(shape), np.zeros(shape)
    for e in range(3):
        j = (e + 1) % 3
        leaves = ~below[e] & below[j]                                        # the boundary leaves "not below" through edge e: L = p_j
        pt, t = _edge_point(P[j], s[j], P[e], s[e])
        for x in range(3):
            np.copyto(a[x], np.broadcast_to(pt[x], shape), where=leaves)
        np.copyto(ta, np.broadcast_to(t, shape), where=leaves)
        np.copyto(ea, np.uint8(e), where=leaves)
        back = below[e] & ~below[j]                                          # ... and comes back through edge e: L = p_e
        pt, t = _edge_point(P[e], s[e], P[j], s[j])
        for x in range(3):
            np.copyto(b[x], np.broadcast_to(pt[x], shape), where=back)
        np.copyto(tb, np.broadcast_to(t, shape), where=back)
        np.copyto(eb, np.uint8(e), where=back)
    return cls, tuple(a), tuple(b), ea, eb, ta, tb, on


def plane_tri_np(planes, tris):
    """planes [n, 4], tris [n, 3, 3] -> cls[n] (uint8), seg[n, 2, 3] (a, b), edge[n, 2] (uint8), t[n, 2], on[n] (uint8)."""
    pl = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    cls, a, b, ea, eb, ta, tb, on = _core(tuple(pl[:, k] for k in range(4)), tuple(tuple(t[:, i, x] for x in range(3)) for i in range(3)))
    seg = np.stack([np.stack(a, axis=-1), np.stack(b, axis=-1)], axis=1).reshape(-1, 2, 3)
    return cls, seg, np.stack([ea, eb], axis=-1).reshape(-1, 2), np.stack([ta, tb], axis=-1).reshape(-1, 2), on


# ---------------------------------------------------------------- the two calls, all pairs
def classes_ref(verts, vidx, planes, pairs_per_chunk=1 << 22, threads=8):
    """The class of EVERY (plane, face) from the vertex values of every (plane, face, vertex): uint8 [n, T]."""
    p, _ = wr._mesh(verts, vidx, None)
    pl = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    n, nt = pl.shape[0], p.shape[0]
    P = tuple(np.ascontiguousarray(p[:, :, x].reshape(-1))[None, :] for x in range(3))       # every face's every vertex
    step = max(1, pairs_per_chunk // max(nt, 1))

    def work(a):
        e = min(n, a + step)
        nb = (side(tuple(pl[a:e, k][:, None] for k in range(4)), P) < 0.0).reshape(e - a, nt, 3).sum(axis=2)
        return np.where(nb == 3, BELOW, np.where(nb == 0, ABOVE, CUT)).astype(np.uint8)

    parts = wr._chunks(work, n, step, threads)
    return np.concatenate(parts) if parts else np.zeros((0, nt), dtype=np.uint8)


def rows_of(verts, vidx, ids, planes, cls) -> PlaneRows:
    p, ids = wr._mesh(verts, vidx, ids)
    pl = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    k, f = np.nonzero(cls == CUT)                                            # row-major: sorted by (plane, face)
    c, seg, edge, t, on = plane_tri_np(pl[k], p[f])
    assert (c == CUT).all()
    return PlaneRows(np.stack([k, f], axis=1).astype(np.uint32).reshape(-1, 2), ids[f], seg, edge, t, on)


def counts_of_classes(cls):
    """n_cut, n_below, n_above per plane."""
    return tuple((cls == c).sum(axis=1).astype(np.uint32) for c in (CUT, BELOW, ABOVE))


def planes_cut_all_ref(verts, vidx, ids, planes) -> PlaneRows:
    return rows_of(verts, vidx, ids, planes, classes_ref(verts, vidx, planes))


def planes_count_ref(verts, vidx, planes):
    return counts_of_classes(classes_ref(verts, vidx, planes))


def take_items(w: PlaneRows, m) -> PlaneRows:
    """The rows of the first m planes."""
    keep = w.rows[:, 0] < m
    return PlaneRows(*(a[keep] for a in w))


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def same_rows(got, want: PlaneRows, what=""):
    """got: a call's (rows, values ...) in any order.  The same set of (plane, face), each once, and every value bit for bit."""
    g = wr.sort_rows(*got[:len(want)])
    assert g[0].shape == want.rows.shape and np.array_equal(g[0], want.rows), (what, g[0].shape, want.rows.shape)
    n = want.rows.shape[0]
    for name, a, b in zip(want._fields[1:], g[1:], want[1:]):
        a, b = np.asarray(a), np.asarray(b)
        if b.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        bad = np.nonzero((a.reshape(n, -1) != b.reshape(n, -1)).any(axis=1))[0] if n else np.zeros(0, dtype=np.int64)
        assert bad.size == 0, (what, name, bad.size, g[0][bad[:4]])


# ---------------------------------------------------------------- what the segments of one plane add up to
def _point_keys(pts):
    """One integer per distinct point (bit for bit, -0.0 and 0.0 apart)."""
    b = _bits(np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    _, inv = np.unique(b, axis=0, return_inverse=True)
    return inv.reshape(-1)


def loops_closed(seg):
    """The multiset of a equals the multiset of b, bit for bit."""
    s = np.asarray(seg, dtype=np.float64).reshape(-1, 2, 3)
    a, b = _bits(s[:, 0]), _bits(s[:, 1])
    order = lambda x: x[np.lexsort((x[:, 2], x[:, 1], x[:, 0]))]
    return np.array_equal(order(a), order(b))


def area(seg, normal):
    """sum n . (a x b) / (2 |n|): the area the loops enclose (counter-clockwise seen from the tip of n counts positive)."""
    s = np.asarray(seg, dtype=np.float64).reshape(-1, 2, 3)
    n = np.asarray(normal, dtype=np.float64)
    return float((np.cross(s[:, 0], s[:, 1]) @ n).sum() / (2.0 * np.sqrt(n @ n)))


def n_loops(seg):
    """The connected components of the segments with a != b (a face that touches the plane with one vertex is no part of a loop)."""
    s = np.asarray(seg, dtype=np.float64).reshape(-1, 2, 3)
    key = _point_keys(s).reshape(-1, 2)
    key = key[key[:, 0] != key[:, 1]]
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in key.tolist():
        parent[find(u)] = find(v)
    return len({find(x) for x in list(parent)})


# ---------------------------------------------------------------- the families of single pairs (tests/test_plane_ref.py checks them against exact arithmetic)
N = 4000


@functools.lru_cache(maxsize=None)
def integer_family(n=N, seed=1):
    """Vertices in {-4 .. 4}^3, normals in {-3 .. 3}^3 \\ 0, d in {-6 .. 6}: every operation up to the quotient is exact.  Vertices on
    the plane, edges in it and whole faces in it all occur; a sixth of the zeros among the coordinates, normals and d are -0.0."""
    g = np.random.default_rng(seed)
    tris = g.integers(-4, 5, (n, 3, 3)).astype(np.float64)
    nrm = g.integers(-3, 4, (n, 3)).astype(np.float64)
    nrm[(nrm == 0).all(axis=1), 2] = 1.0
    d = g.integers(-6, 7, (n, 1)).astype(np.float64)
    planes = np.concatenate([nrm, d], axis=1)
    for arr in (tris, planes):
        flip = (arr == 0.0) & (g.random(arr.shape) < 1.0 / 6.0)
        arr[flip] = -0.0
    return np.ascontiguousarray(planes), np.ascontiguousarray(tris)


@functools.lru_cache(maxsize=None)
def constructed_family(n=N, seed=2):
    """Dyadic triangles (coordinates i / 16 in [-2, 2]) against axis-parallel planes through one of their vertices' coordinates, and
    against the planes x + y = d, x - z = d through a vertex (exact sums): one vertex, an edge (two vertices share the coordinate in a
    third of the cases) or the whole face (all three share it in a ninth) lie in the plane exactly."""
    g = np.random.default_rng(seed)
    tris = g.integers(-32, 33, (n, 3, 3)).astype(np.float64) / 16.0
    kind = g.integers(0, 5, n)
    share = g.integers(0, 3, n)                                              # 1: p1 shares p0's coordinate; 2: p1 and p2 do
    planes = np.zeros((n, 4))
    for i in range(n):
        ax = int(kind[i]) % 3
        if kind[i] < 3:
            for j in range(1, 1 + int(share[i])):
                tris[i, j, ax] = tris[i, 0, ax]
            sign = 1.0 if g.random() < 0.5 else -1.0
            planes[i, ax] = sign
            planes[i, 3] = sign * tris[i, 0, ax]
        elif kind[i] == 3:
            planes[i] = (1.0, 1.0, 0.0, tris[i, 0, 0] + tris[i, 0, 1])
        else:
            planes[i] = (1.0, 0.0, -1.0, tris[i, 0, 0] - tris[i, 0, 2])
    return np.ascontiguousarray(planes), np.ascontiguousarray(tris)


@functools.lru_cache(maxsize=None)
def random_family(offset=0.0, n=100_000, seed=3):
    """Triangles (a vertex and two more within 0.3 of it) in the unit cube moved by `offset`, and planes with a normal uniform in
    [-1, 1]^3 times 1 or 37.5 through a point within 0.3 of the first vertex: about half are cut."""
    g = np.random.default_rng(seed)
    p0 = g.random((n, 1, 3))
    tris = np.concatenate([p0, np.clip(p0 + 0.6 * (g.random((n, 2, 3)) - 0.5), 0.0, 1.0)], axis=1) + offset
    nrm = g.uniform(-1.0, 1.0, (n, 3)) * np.where(g.random((n, 1)) < 0.5, 1.0, 37.5)
    through = tris[:, 0] + 0.6 * (g.random((n, 3)) - 0.5)
    d = (nrm * through).sum(axis=1)
    return np.ascontiguousarray(np.concatenate([nrm, d[:, None]], axis=1)), np.ascontiguousarray(tris)


OFFSET = 2.0 ** 20 + 0.37


# ---------------------------------------------------------------- the meshes and planes of the tests
L = 256                                                                      # CD_PLANE_SLAB (tests/test_planes_abi.py compares it with the header's)
SOUP_SIZES = (1, 2, L - 1, L, L + 1, 2 * L + 1, 64 * L + 1)                  # the last: one plane has 65 slabs, two waves


def _soup(n):
    v, i = si.box_soup(n, 0.02 if n > 4 * L else 0.2, 0.0, 1.0, 100 + (n % 97))
    return v, i, None, 0.02 if n > 4 * L else 0.2


@functools.lru_cache(maxsize=None)
def mesh(name):
    """name -> (verts, vidx, ids, edge): the meshes of tests/box_ref.py, the closed meshes, and soups of exactly n faces ("soup<n>")."""
    if name in wr.MESHES:
        return wr.MESHES[name]
    if name.startswith("soup") and name[4:].isdigit() and name not in wr.MESHES:
        return _soup(int(name[4:]))
    v, f = {"torus": cm.torus, "box_grid": cm.box_grid, "nested_boxes": cm.nested_boxes}[name.replace("_rotated", "")]()
    if name.endswith("_rotated"):
        v = cm.rotated(v)
    return v, f, None, 0.25


NAMES = ["n1", "n2", "n3", "n63", "n64", "n65", "duplicates", "custom_ids", "comb", "soup10k", "cloth100"]     # box_ref.NAMES
SOUPS = [f"soup{n}" for n in SOUP_SIZES]
CLOSED = ["torus", "box_grid", "nested_boxes", "box_grid_rotated"]
COUNTS = (1, 63, 64, 65, 1000)
SEED = 29
KINDS = ("random", "axis", "vertex", "axis_vertex", "miss", "scaled", "random", "axis_neg")   # plane i is of kind KINDS[i % 8]
SIDES_AT = 8                                                                 # planes SIDES_AT .. SIDES_AT + 5: the six sides of the root box


def make_planes(verts, vidx, n, seed=SEED):
    """n planes [n, 4] for a mesh, by index modulo 8: a RANDOM normal through a random point of the root box; AXIS-parallel (+e_a)
    through a random coordinate; a random normal through a mesh VERTEX (d computed in plane_tri's own order, so that vertex has s == 0
    exactly); axis-parallel through a vertex's coordinate (every vertex that shares it lies in the plane); a plane that MISSES the mesh
    (all of it on one side); a random normal SCALED by 37.5 (not a unit vector); -e_a through a random coordinate.  Planes SIDES_AT ..
    SIDES_AT + 5 are the six sides of the mesh's root box with the normal pointing out of it -- for box_grid they contain a whole side
    of the mesh.  (The first plane is of kind `random`, so one plane alone is an ordinary one.)"""
    v = np.asarray(verts, dtype=np.float64)
    used = v[np.asarray(vidx).astype(np.int64)].reshape(-1, 3)
    lo, hi = used.min(axis=0), used.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3)
    g = np.random.default_rng(seed)
    out = np.zeros((n, 4))
    for i in range(n):
        kind = KINDS[i % 8]
        nrm = g.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        at = used[g.integers(0, used.shape[0])]
        ax = int(g.integers(0, 3))
        through = lo + g.random(3) * (hi - lo)
        if kind in ("axis", "axis_neg", "axis_vertex"):
            sign = -1.0 if kind == "axis_neg" else 1.0
            nrm = np.zeros(3)
            nrm[ax] = sign
            c = at[ax] if kind == "axis_vertex" else through[ax]
            out[i] = (*nrm, sign * c)
        elif kind == "vertex":
            out[i] = (*nrm, (nrm[0] * at[0] + nrm[1] * at[1]) + nrm[2] * at[2])
        elif kind == "miss":
            far = (hi + ext) if i % 16 < 8 else (lo - ext)                  # wholly below, or wholly above, in turn
            nrm = np.abs(nrm) + 0.1
            out[i] = (*nrm, float(nrm @ far))
        else:
            if kind == "scaled":
                nrm = nrm * 37.5
            out[i] = (*nrm, float(nrm @ through))
    for s in range(6):
        if SIDES_AT + s < n:
            ax, up = s // 2, s % 2
            nrm = np.zeros(3)
            nrm[ax] = 1.0 if up else -1.0
            out[SIDES_AT + s] = (*nrm, hi[ax] if up else -lo[ax])
    return np.ascontiguousarray(out)


# closed meshes and planes whose sections the CPU test and the GPU test both check: loops closed bit for bit, and where stated the
# enclosed area (exact) and the number of loops
CLOSED_CASES = [
    # mesh, normal, d, area (None: not stated), loops (None: not stated)
    ("box_grid", (0.0, 0.0, 1.0), 0.25, 1.0, 1),                             # through vertices
    ("box_grid", (0.0, 0.0, 2.0), 0.75, 1.0, 1),                             # between them, |n| = 2
    ("box_grid", (0.0, 0.0, 1.0), 1.0, 1.0, 1),                              # along the whole top side: its faces are ABOVE, the walls report the edges
    ("box_grid", (0.0, 0.0, 1.0), 0.0, None, 0),                             # along the bottom: nothing is below
    ("box_grid", (1.0, 0.0, 0.0), 0.5, 1.0, 1),
    ("box_grid", (0.3, -0.5, 0.81), 0.2, None, 1),
    ("torus", (1.0, 0.0, 0.0), 0.0, 0.84375, 2),
    ("torus", (0.0, 0.0, 1.0), 0.0, None, 2),
    ("torus", (0.3, -0.5, 0.81), 0.1, None, None),
    ("nested_boxes", (0.0, 0.0, 1.0), 0.5, 0.75, 2),                         # the cavity's loop runs the other way: 1 - 1/4
    ("nested_boxes", (0.0, 0.0, 1.0), 0.25, None, None),                     # along the cavity's whole bottom side
    ("nested_boxes", (0.0, 1.0, 0.0), 0.75, None, None),
    ("box_grid_rotated", (0.0, 0.0, 1.0), 2.0 ** 20 + 0.9, None, 1),
    ("box_grid_rotated", (0.3, -0.5, 0.81), 0.61 * (2.0 ** 20 + 0.37) + 0.4, None, None),
    ("nested_boxes_rotated", (1.0, 2.0, -0.5), 2.5 * (2.0 ** 20 + 0.37) + 0.6, None, None),
    ("torus_rotated", (0.0, 1.0, 0.0), 2.0 ** 20 + 0.37, None, None),
]


@functools.lru_cache(maxsize=None)
def planes(name, n=1000):
    v, i, ids, edge = mesh(name)
    return make_planes(v, i, n)


@functools.lru_cache(maxsize=None)
def want_classes(name, n=1000):
    v, i, ids, edge = mesh(name)
    return classes_ref(v, i, planes(name, n))


@functools.lru_cache(maxsize=None)
def want_rows(name, n=1000) -> PlaneRows:
    v, i, ids, edge = mesh(name)
    return rows_of(v, i, ids, planes(name, n), want_classes(name, n))


def input_conditions(name):
    """What the GPU test needs of its planes, per mesh: planes with no row (the miss planes, n / 8 less the one a side of the root box replaces) on both sides, and on a mesh of
    more than three faces planes with several rows, faces below and faces above for the same plane, and rows whose `on` is set."""
    n, nt = 1000, mesh(name)[1].shape[0]
    n_cut, n_below, n_above = counts_of_classes(want_classes(name))
    w = want_rows(name)
    print(name, "planes without a row", int((n_cut == 0).sum()), "with several", int((n_cut >= 2).sum()), "rows", w.rows.shape[0], "with a vertex in the plane", int((w.on != 0).sum()))
    assert (n_cut == 0).sum() >= n // 10 and (n_below == nt).sum() >= n // 20 and (n_above == nt).sum() >= n // 20
    assert ((n_cut + n_below + n_above) == nt).all()
    if nt > 3:
        assert (n_cut >= 2).sum() >= n // 8 and ((n_below > 0) & (n_above > 0)).sum() >= n // 8 and (w.on != 0).any()
