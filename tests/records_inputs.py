"""The meshes test_records_ref.py and test_records_gpu.py pin the fp32 records on: the smallest at which each part of the encoding
(cd_bvh.h, lines 16-40) can go wrong.  Deterministic, seeded, built on first use; the oracle's tree and the restatement's records of
each are computed once and shared (treat them as read-only).  No test in here."""
from __future__ import annotations

import functools

import numpy as np

import mi355_synth as synth
import oracle
import records_ref as rr

SIZES = (1, 2, 3, 64, 65, 512, 513, 600, 1300, 512 * 7 + 1)     # one wave and one more, one 512-leaf block and one more, two blocks, four block slots with one empty, seven blocks and one leaf
BRUTE_MAX = 2048                                                # the all-pairs theorem check runs up to here


def soup_double(n: int, e: float, seed: int):
    """mi355_synth.soup's recipe WITHOUT its rounding to float: every coordinate a full double (synth.soup's are fp32 values)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    c = synth.BOX_LO + (synth.BOX_HI - synth.BOX_LO) * rng.random((n, 3))
    d = (rng.random((n, 3, 3)) - 0.5) * e
    return np.ascontiguousarray((c[:, None, :] + d).reshape(3 * n, 3)), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def _f32(v):
    return np.ascontiguousarray(v.astype(np.float32).astype(np.float64))


def soup_snapped(n: int, e: float, seed: int):
    """A double soup whose coordinates crowd into few fp32 cells whatever n is: each is snapped to a grid of about 0.7 n values per axis (fp32
    values: bases) and then moved up by j / 8 of an fp32 ulp, j in 0 .. 3.  About three coordinates of an axis share a cell: ambiguous cells,
    bounds at the base (j = 0: fp32 values, never moved), moved bounds and cell mates below them, at every size of the series."""
    v, t = soup_double(n, e, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 7000))
    q = 4.0 * 2.0 ** -int(np.ceil(np.log2(max(n, 8))))
    base = np.round(v / q) * q                                                 # few bits: fp32 values (0.0 among them)
    b32 = base.astype(np.float32)
    assert np.array_equal(b32.astype(np.float64), base)
    ulp = np.nextafter(b32, np.float32(np.inf)).astype(np.float64) - base
    return np.ascontiguousarray(base + rng.integers(0, 4, size=base.shape) * (ulp / 8)), t


def _tris(pts):
    """[k, 3, 3] points -> private vertices."""
    pts = np.asarray(pts, dtype=np.float64)
    return np.ascontiguousarray(pts.reshape(-1, 3)), np.arange(3 * pts.shape[0], dtype=np.uint32).reshape(-1, 3)


def _bases():
    """Per k a float base b_k and a second double d_k = b_k + ulp / 4 in b_k's cell, on every axis: the cell is ambiguous.  Triangle 3k has
    its hi AT the base (never moved: nothing of the cell lies below it), triangle 3k + 1 at d_k (moved), and triangle 3k + 2 its LO at the
    base: against it the moved hi is the only thing that keeps b_k < d_k visible in fp32 (an unmoved one loses the pair); the other
    coordinates are doubles alone in their cells.  Negative bases too (the step goes toward zero there)."""
    rng = np.random.Generator(np.random.PCG64(501))
    K = 160
    b = (0.2 + 2.5 * rng.random((K, 3))) * np.where(rng.random((K, 3)) < 0.3, -1.0, 1.0)
    b = b.astype(np.float32)
    d = b.astype(np.float64) + (np.nextafter(b, np.float32(np.inf)).astype(np.float64) - b.astype(np.float64)) / 4
    pts = np.zeros((3 * K, 3, 3))
    for k in range(K):
        for t, top in ((3 * k, b[k].astype(np.float64)), (3 * k + 1, d[k])):
            low = top[None, :] - 0.01 - 0.05 * rng.random((2, 3))
            pts[t] = np.concatenate([low, top[None, :]])[rng.permutation(3)]
        bottom = b[k].astype(np.float64)
        high = bottom[None, :] + 0.01 + 0.05 * rng.random((2, 3))
        pts[3 * k + 2] = np.concatenate([bottom[None, :], high])[rng.permutation(3)]
    return _tris(pts)


def _zeros():
    """Both zeros and the double denormals on every axis.  -0.0 and +0.0 are one value; 5e-324 is a second double in the cell of 0 (an hi there moves
    from 0 to the smallest fp32 denormal); -5e-324 and -1e-323 share the cell of -1.4e-45 (an hi there moves to -0.0)."""
    t, u = 5e-324, 1e-323
    pts = [
        [[-1.0, -1.0, -0.0], [1.0, -1.0, -0.0], [0.25, 1.0, -0.0]],            # flat in the plane z = -0.0
        [[-0.5, -0.75, 0.0], [0.75, -0.5, 0.0], [0.125, 0.5, 0.0]],            # ... and in z = +0.0
        [[-1.3, -0.7, -0.9], [-0.2, -0.3, -0.4], [t, t, t]],                   # hi = 5e-324 on every axis: moved, 0 -> 1.4e-45
        [[-1.1, -0.6, -0.8], [-0.3, -0.2, -0.1], [0.0, 0.0, 0.0]],             # hi = +0.0: the base, not moved
        [[-1.2, -0.5, -0.7], [-0.4, -0.1, -0.2], [-0.0, -0.0, -0.0]],          # hi = -0.0: the base (kept as -0.0), not moved
        [[-1.4, -0.8, -0.6], [-0.6, -0.4, -0.3], [-t, -t, -t]],                # hi = -5e-324: the cell of -1.4e-45, ambiguous, moved to -0.0
        [[-1.5, -0.9, -0.5], [-0.7, -0.5, -0.4], [-u, -u, -u]],                # hi = -1e-323: the same cell, moved too
        [[-t, -t, -t], [0.6, 0.4, 0.3], [1.2, 0.8, 0.7]],                      # lo = -5e-324 -> -1.4e-45
        [[t, t, t], [0.7, 0.5, 0.2], [1.1, 0.9, 0.6]],                         # lo = 5e-324 -> +0.0
        [[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [0.5, 0.25, 0.125]],             # both zeros in one triangle: the first of equals stays
        [[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [-0.5, -0.25, -0.125]],
        [[t, -t, 0.0], [-t, t, -0.0], [0.0, -0.0, t]],                         # a box inside the denormals
    ]
    rng = np.random.Generator(np.random.PCG64(502))
    v, _ = soup_double(36, 0.5, 503)
    v = (v - np.array([1.5, -0.1, 0.75])) * 0.5                                # ordinary triangles around the origin, both signs
    allp = np.concatenate([np.asarray(pts, dtype=np.float64), v.reshape(-1, 3, 3)])
    return _tris(allp[rng.permutation(allp.shape[0])])


def _beyond_fp32():
    """Magnitudes 1e39 .. 1e300 beside ordinary ones.  x: two distinct doubles above FLT_MAX (1e39, 1e300) share FLT_MAX's cell -- an hi
    there is stored as +inf; y: ONE double above FLT_MAX (1e200, at several vertices) -- alone in its cell, stored as FLT_MAX; z: ordinary.
    Below -FLT_MAX a lo is stored as -inf (x: -1e39 and -1e300; y: -1e150)."""
    v, _ = soup_double(300, 0.2, 504)
    pts = v.reshape(-1, 3, 3).copy()
    pts[10, 0] = [1e39, 1e200, 0.5]
    pts[11, 1] = [1e300, 1e200, 0.25]
    pts[12, 2] = [1e39, 0.1, 0.75]
    pts[13, 0] = [-1e39, -1e150, 0.5]
    pts[14, 1] = [-1e300, 0.2, 1.5]
    pts[15] = [[1e300, 1e200, 1.0], [1e39, 1e200, 1.25], [1e300, 1e200, 1.5]]          # a whole box above FLT_MAX in x, flat in y
    pts[16] = [[-1e300, -1e150, 1.0], [1e300, 1e200, -0.25], [0.5, 0.1, 0.3]]          # -inf .. +inf
    return _tris(pts)


def _few_cells():
    """x takes eight distinct doubles (four cells, two doubles each: all ambiguous), shared by thousands of vertices -- the look-before-the-atomic
    path of k_amb_insert; y and z are a double soup's."""
    v, t = soup_double(4000, 0.05, 505)
    base = np.array([0.3, 0.9, 1.7, 2.6], dtype=np.float32).astype(np.float64)
    xs = np.concatenate([base + 2.0 ** -30, base + 2.0 ** -29])
    rng = np.random.Generator(np.random.PCG64(506))
    v[:, 0] = xs[rng.integers(0, 8, size=v.shape[0])]
    return v, t


def _cloth_double():
    """cloth_pair's sheets with full-double coordinates, moved to where fp32 cells are coarse against the mesh: at 20000 (ulp 2^-9) a column's x -- one double,
    shared by the column's boxes as a face -- often shares its cell with the other sheet's column 0.0007 away, and so a row's z; at 1000 (ulp 2^-14) the heights
    crowd into a few hundred cells.  Moved bounds on all three axes, and boxes none of whose bounds is moved."""
    v, t = synth.cloth_pair(22, round_f32=False)
    return np.ascontiguousarray(v + np.array([20000.0, 1000.0, 20000.0])), t


def _duplicates():
    v, t = soup_double(500, 0.1, 507)
    v[1::7] = v[0]                                                             # the same double at many vertices: equal values are not distinct
    v[2::11, 1] = v[5, 1]
    return v, np.ascontiguousarray(np.concatenate([t, t, t[:250]]))


def _mixed():
    v, t = soup_double(30000, 0.04, 78)
    v[: len(v) // 2] = _f32(v[: len(v) // 2])
    return v, t


def _cloth_float():
    v, t = _cloth_double()
    return _f32(v), t


def _negatives():
    v, t = soup_double(1500, 0.3, 508)
    return np.ascontiguousarray(v - 40.0), t


def _many_cells():
    return soup_double(40000, 0.03, 77)


_MAKERS = {
    "cloth_double": _cloth_double,
    "cloth_float": _cloth_float,
    "mixed": _mixed,
    "bases": _bases,
    "zeros": _zeros,
    "negatives": _negatives,
    "beyond_fp32": _beyond_fp32,
    "duplicates": _duplicates,
    "many_cells": _many_cells,
    "few_cells": _few_cells,
}
for _n in SIZES:
    _MAKERS[f"soup{_n}"] = functools.partial(soup_snapped, _n, 0.2, 600 + _n)

# triangles per mesh, known without building it (mesh() checks it)
N_TRIS = {"cloth_double": 1936, "cloth_float": 1936, "mixed": 30000, "bases": 480, "zeros": 48, "negatives": 1500, "beyond_fp32": 300, "duplicates": 1250,
          "many_cells": 40000, "few_cells": 4000, **{f"soup{_n}": _n for _n in SIZES}}
SMALL = tuple(m for m in _MAKERS if N_TRIS[m] <= BRUTE_MAX)                    # where the all-pairs theorem check runs
# meshes that hold a moved hi with a CELL MATE below it among the leaves' lo bounds: leaving that hi unmoved loses a pair, which the theorem check must notice.
# cloth_double, bases, zeros and the snapped soups have such mates by construction.  negatives and beyond_fp32 have them by chance of their seeded
# soups (a handful of bounds each): test_records_ref.py asserts that they are there, so another seed that loses them fails on the CPU, not silently
TEETH = ("cloth_double", "bases", "zeros", "negatives", "beyond_fp32") + tuple(f"soup{_n}" for _n in SIZES if 64 <= _n <= BRUTE_MAX)

MESHES = tuple(f"soup{_n}" for _n in SIZES) + ("cloth_double", "cloth_float", "mixed", "bases", "zeros", "negatives", "beyond_fp32", "duplicates", "many_cells", "few_cells")

# the classes of leaves each mesh is there for: "exact" (fp32 values, certain), "certain" (certain, not exact), "uncertain" (an hi was moved);
# and the classes it must NOT have
CLASSES = {
    "cloth_double": ({"certain", "uncertain"}, set()),
    "cloth_float": ({"exact"}, {"certain", "uncertain"}),
    "mixed": ({"exact", "certain", "uncertain"}, set()),
    "bases": ({"certain", "uncertain"}, set()),
    "zeros": ({"certain", "uncertain"}, set()),
    "negatives": ({"certain", "uncertain"}, set()),
    "beyond_fp32": ({"certain", "uncertain"}, set()),
    "duplicates": ({"certain"}, {"exact", "uncertain"}),
    "many_cells": ({"certain", "uncertain"}, set()),
    "few_cells": ({"uncertain"}, set()),
    **{f"soup{_n}": ({"certain", "uncertain"}, set()) for _n in SIZES if _n >= 64},
}


@functools.lru_cache(maxsize=None)
def mesh(name):
    v, t = _MAKERS[name]()
    v, t = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(t, dtype=np.uint32)
    assert t.shape[0] == N_TRIS[name], (name, t.shape[0])
    v.setflags(write=False); t.setflags(write=False)
    return v, t


@functools.lru_cache(maxsize=None)
def step(name):
    """The oracle's tree of the mesh in the reference frame."""
    v, t = mesh(name)
    return oracle.pipeline(v, t)


@functools.lru_cache(maxsize=None)
def want(name, mode=None):
    v, t = mesh(name)
    return rr.expected_records(v, t, step(name), mode)


def classes(w):
    """(exact, certain but not exact, not certain) leaves of an expectation."""
    e, c = w["leaf"]["exact"], w["leaf"]["certain"]
    return int(e.sum()), int((c & ~e).sum()), int((~c).sum())
