"""Meshes whose colliding pairs are known BY CONSTRUCTION, for the device pair-list sort and ID set (cd_sorted_pairs,
cd_collision_triangles: csrc/cd_post.h, pp_sort / pp_reserve in csrc/mi355cd.hip, k_scan_exclusive in csrc/cd_sort.h).

crosses(K, fans, live) puts isolated cells on a g x g x g grid in the unit cube, g = ceil(cbrt(cells)), pitch 1 / g, triangle scale
0.4 / g; vertices are rounded to fp32 and never shared.  A cell holds one flat triangle (0,0,.5) (1,0,.5) (0,1,.5) and j thin blades
(u,v,.2) (u+w,v,.8) (u,v+w,.8) that pierce it, laid on a triangular lattice inside it (footprints a lattice step apart, 0.4 of a step
wide: their boxes are disjoint, so blades never meet each other).  A cross cell has j = 1, a fan cell the j asked for: exactly j pairs,
all of them holding the flat triangle (the hub).  Cells are 0.6 pitches apart, so nothing else touches.  A blade whose `live` entry is
False is lifted by half a pitch in z, clear of its flat triangle and still inside its cell: same topology, fewer pairs.

Faces: cross c is faces 2c (flat) and 2c + 1 (blade); then every fan as its hub followed by its blades.  Row i of `pairs` is blade
i's pair (flat face, blade face), in face order -- never taken from the device or the oracle; tests/test_post_inputs.py checks it
against oracle.pipeline.  The unit cube is not the reference's Morton frame: contexts and the oracle take FRAME_OFF / FRAME_SPAN as a
custom frame (the pair set does not depend on the frame).

ID maps (ids[face], each a bijection into uint32): see ID_MAPS.  The ABI reserves no triangle ID -- cd_create takes any uint32, the
ID rule of the kernels is a plain a < b, and 0xFFFFFFFF as a "none" value exists only in the outputs of cd_cast_rays /
cd_closest_points -- so the random map includes both 0 and 0xFFFFFFFF.

The comparison helpers at the end are the ones tests/test_post_gpu.py uses; tests/test_post_inputs.py shows on the CPU that each of
them fails on a wrong result."""
from __future__ import annotations

import numpy as np

FRAME_OFF = np.zeros(3, dtype=np.float64)
FRAME_SPAN = np.ones(3, dtype=np.float64)
CD_OK, CD_OVERFLOW = 0, 1


class Mesh:
    """verts f64[V, 3], vidx u32[nt, 3], pairs u32[m, 2] (face indices of the LIVE blades' pairs, in blade order), all_pairs (every
    blade's pair, live or not), fans: [(hub face, first blade face, j)], n_cross: the number of cross cells in front."""

    def __init__(self, verts, vidx, all_pairs, live, fans, n_cross):
        self.verts, self.vidx, self.all_pairs, self.live, self.fans, self.n_cross = verts, vidx, all_pairs, live, fans, n_cross
        self.pairs = np.ascontiguousarray(all_pairs[live])
        self.nt = vidx.shape[0]


def _lattice(j: int):
    """j lattice points (u, v) and the blade width w inside the unit right triangle: rows a + b <= n - 1 of step d = 1 / (n + 2)."""
    n = 1
    while n * (n + 1) // 2 < j:
        n += 1
    d = 1.0 / (n + 2)
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = (a + b) <= n - 1
    a, b = a[keep][:j], b[keep][:j]
    return (a + 0.6) * d, (b + 0.6) * d, 0.4 * d


def crosses(K: int, fans=(), live=None) -> Mesh:
    fans = tuple(int(j) for j in fans)
    blades_of = np.array([1] * K + list(fans), dtype=np.int64)             # blades per cell
    cells = blades_of.shape[0]
    g = 1
    while g * g * g < cells:
        g += 1
    pitch, s = 1.0 / g, 0.4 / g
    m_all = int(blades_of.sum())
    live = np.ones(m_all, dtype=bool) if live is None else np.ascontiguousarray(live, dtype=bool)
    assert live.shape == (m_all,)
    c = np.arange(cells)
    origin = np.stack([c % g, (c // g) % g, c // (g * g)], axis=-1) * pitch                    # [cells, 3]
    first_face = np.concatenate([[0], np.cumsum(blades_of + 1)])[:-1]                          # the cell's flat triangle
    first_blade = np.concatenate([[0], np.cumsum(blades_of)])[:-1]                             # the cell's first row of all_pairs
    nt = int((blades_of + 1).sum())
    tri = np.empty((nt, 3, 3), dtype=np.float64)
    all_pairs = np.empty((m_all, 2), dtype=np.uint32)
    flat = np.array([[0, 0, .5], [1, 0, .5], [0, 1, .5]], dtype=np.float64)
    tri[first_face] = origin[:, None, :] + s * flat[None]
    # the crosses in one go, the fans one by one
    u1, v1, w1 = _lattice(1)
    for cell0, cell1, (u, v, w) in [(0, K, (u1, v1, w1))] + [(K + f, K + f + 1, _lattice(j)) for f, j in enumerate(fans)]:
        if cell1 == cell0:
            continue
        j = u.shape[0]
        blade = np.stack([np.stack([u, v, np.full(j, .2)], -1), np.stack([u + w, v, np.full(j, .8)], -1), np.stack([u, v + w, np.full(j, .8)], -1)], 1)   # [j, 3, 3]
        cc = np.arange(cell0, cell1)
        faces = (first_face[cc][:, None] + 1 + np.arange(j)[None]).ravel()                     # [cells x j]
        rows = (first_blade[cc][:, None] + np.arange(j)[None]).ravel()
        t = origin[cc][:, None, None, :] + s * blade[None]                                     # [cells, j, 3, 3]
        t = t.reshape(-1, 3, 3)
        t[~live[rows], :, 2] += 0.5 * pitch
        tri[faces] = t
        all_pairs[rows, 0] = np.repeat(first_face[cc], j)
        all_pairs[rows, 1] = faces
    verts = np.ascontiguousarray(tri.reshape(-1, 3).astype(np.float32).astype(np.float64))
    vidx = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    fan_list = [(int(first_face[K + f]), int(first_face[K + f]) + 1, j) for f, j in enumerate(fans)]
    return Mesh(verts, vidx, all_pairs, live, fan_list, K)


# ---- ID maps: nt -> ids u32[nt], ids[face]
def _bitrev32(i):
    x = np.asarray(i, dtype=np.uint32).copy()
    for sh, mask in ((1, 0x55555555), (2, 0x33333333), (4, 0x0F0F0F0F), (8, 0x00FF00FF)):
        x = ((x >> np.uint32(sh)) & np.uint32(mask)) | ((x & np.uint32(mask)) << np.uint32(sh))
    return (x >> np.uint32(16)) | (x << np.uint32(16))


def _random_ids(nt: int, seed: int = 20240607):
    """A seeded injection over the whole uint32 range that takes 0 and 0xFFFFFFFF (no ID is reserved: module docstring)."""
    rng = np.random.Generator(np.random.PCG64(seed + nt))
    pool = np.unique(rng.integers(1, 0xFFFFFFFF, size=nt + nt // 8 + 16, dtype=np.uint64))   # 0 and the top value come in by hand
    assert pool.shape[0] >= nt
    ids = rng.permutation(pool)[:nt].astype(np.uint32)
    where = rng.permutation(nt)
    ids[where[0]] = 0xFFFFFFFF
    if nt > 1:
        ids[where[1]] = 0
    return ids


ID_MAPS = {
    "identity": lambda nt: np.arange(nt, dtype=np.uint32),
    "reversed": lambda nt: np.arange(nt, dtype=np.uint32)[::-1].copy(),
    "shl8": lambda nt: np.arange(nt, dtype=np.uint32) << np.uint32(8),
    "shl12_fff": lambda nt: (np.arange(nt, dtype=np.uint32) << np.uint32(12)) | np.uint32(0xFFF),
    "bitrev": lambda nt: _bitrev32(np.arange(nt, dtype=np.uint32)),            # the TOP byte varies fastest: no digit pass of the pair key is trivial
    "random": _random_ids,
}
LARGE_MAPS = ("bitrev", "random")


def ids_for(name: str, nt: int) -> np.ndarray:
    assert (name != "shl8" or nt <= 1 << 24) and (name != "shl12_fff" or nt <= 1 << 20)
    ids = np.ascontiguousarray(ID_MAPS[name](nt), dtype=np.uint32)
    assert ids.shape == (nt,)
    return ids


def place_hubs(ids: np.ndarray, mesh: Mesh, where: str) -> np.ndarray:
    """The same IDs with every fan's hub given the smallest / largest / middle ID of its fan (the blades keep the fan's other IDs in
    their order): 'smallest' -> the fan's keys share their HIGH word, 'largest' -> their LOW word, the hub in the second column."""
    out = ids.copy()
    for hub, first, j in mesh.fans:
        own = np.sort(ids[hub:hub + j + 1])
        k = {"smallest": 0, "largest": j, "middle": j // 2}[where]
        out[hub] = own[k]
        out[first:first + j] = np.delete(own, k)
    return out


# ---- the references: (a) of the by-construction list, (b) of the unordered list a step returned
def ordered(pairs_faces: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """Face pairs -> ID pairs (smaller ID, larger ID), in the given row order."""
    p = ids[np.asarray(pairs_faces, dtype=np.int64).reshape(-1, 2)]
    return np.ascontiguousarray(np.stack([p.min(1), p.max(1)], axis=-1), dtype=np.uint32).reshape(-1, 2)


def sort_rows(pairs: np.ndarray) -> np.ndarray:
    p = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    return np.ascontiguousarray(p[np.lexsort((p[:, 1], p[:, 0]))])


def id_set(pairs: np.ndarray) -> np.ndarray:
    return np.unique(np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1))


# ---- comparisons: exact, no tolerance anywhere
def _same(got, n, rc, want, what):
    assert rc == CD_OK, f"{what}: return code {rc}"
    assert n == want.shape[0], f"{what}: n = {n}, expected {want.shape[0]}"
    got = np.asarray(got)
    assert got.dtype == np.uint32 and got.shape == want.shape, f"{what}: {got.dtype}{got.shape}, expected uint32{want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(1))
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.shape[0]} entries differ, first at {bad[0]}: got {got[bad[0]]}, expected {want[bad[0]]}")


def same_sorted_pairs(res, want_rows, what="cd_sorted_pairs"):
    """res = (pairs, n, rc) of cd_sorted_pairs; want_rows: UNSORTED (smaller ID, larger ID) rows -- the reference sorts them."""
    got, n, rc = res
    _same(got, n, rc, sort_rows(want_rows), what)


def same_id_set(res, want_rows, what="cd_collision_triangles"):
    got, n, rc = res
    _same(got, n, rc, id_set(want_rows), what)


def same_step(res, want_rows, what="step"):
    """res = (pairs, n, rc) of a traversal; the pairs come in any order: the SET must be want_rows', with nothing twice."""
    got, n, rc = res
    _same(sort_rows(got), n, rc, sort_rows(want_rows), what)
