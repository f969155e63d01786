"""Meshes, motions and power-of-two scales for the range tests of the proximity and continuous collision queries, and the points of
the inside query's (tests/test_inside_gpu.py; tests/test_column_ref.py pins column_ref.points_inside's equivariance over SCALES).

Scaling every coordinate, dist and the motion by 2^k is exact in FP64 (no coordinate comes near the FP64 subnormal or overflow range
for k in SCALES), and the restatements (tests/proximity_ref.py, tests/ccd_ref.py) are equivariant under it over that band: the same
pairs, distances times 2^k, the same toi bits (tests/test_proximity_ref.py, tests/test_ccd_ref.py pin this).  The device filters work
in fp32, whose range the band runs off at both ends: from k = 127 on, coordinates lie above FLT_MAX (their fp32 cell is FLT_MAX's or
-FLT_MAX's, and rounding up gives +inf; from about k = 148 the pads' M 2^-20 does too), from k = -126 down they are fp32 subnormals,
and from about k = -155 down they all round to +-0 or +-2^-149.  So the device must give the k = 0 result, scaled, at every k
(tests/test_query_scales_gpu.py).

Where the band ends: on the cloth meshes here (largest |coordinate| about 12) between k = 256 and 264 and between k = -320 and -360,
the 17-axis contact predicate that tri_distance takes "in contact => 0" from overflows or underflows (it is the reference's, evaluated
on unscaled coordinates), and at |k| >~ 512 the rate bound L of the advancement (an unscaled sqrt of squares) becomes inf or 0.
Results there follow those predicates, not the scaled k = 0 result.
"""
from __future__ import annotations

import functools

import numpy as np

import mi355_synth as synth

# the band the tests pin: around FLT_MAX (127 .. 136), around where the pads round up to +inf (148, 149), into and through the fp32
# subnormals (-126, -127, -140, -149, -150), and far beyond both ends (-320, -200, 200, 256)
SCALES = (-320, -200, -150, -149, -140, -127, -126, -64, 0, 64, 127, 128, 129, 136, 148, 149, 200, 256)
EDGES = (0, 128, -149)          # the scales at which the device is compared with the restatement itself (elsewhere: with k = 0)

FLT_MAX = float(np.finfo(np.float32).max)


def box_soup(n, e, lo, hi, seed):
    """n triangles of private vertices, centroid uniform in [lo, hi]^3, vertices centroid + U(-e/2, e/2)^3, rounded to fp32."""
    g = np.random.default_rng(seed)
    c = lo + (hi - lo) * g.random((n, 3))
    v = (c[:, None, :] + (g.random((n, 3, 3)) - 0.5) * e).reshape(-1, 3)
    return np.ascontiguousarray(v.astype(np.float32).astype(np.float64)), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def meshes():
    """name -> (verts, vidx, edge).  Every axis has coordinates of magnitude > 1 (so > FLT_MAX at k >= 128); 'centred' has both signs
    on every axis (the -inf cell at k >= 128, -0 and +0 cells at k <= -150)."""
    out = {}
    v, i = box_soup(1000, 0.3, 1.0, 3.0, 11)
    out["dense"] = (v, i, 0.3)
    for name, r32 in (("cloth", True), ("cloth_double", False)):
        v, i = synth.cloth_pair(16, round_f32=r32)
        v = v * 4.0
        v[:, 1] -= 1.0                                                          # x in [0.24, 11.8], y in [-1.5, -1.3], z in [-1.4, 7.4]
        if r32:
            v = v.astype(np.float32).astype(np.float64)
        out[name] = (np.ascontiguousarray(v), i, 0.72)
    v, i = box_soup(1000, 0.4, -2.0, 2.0, 12)
    out["centred"] = (v, i, 0.4)
    return out


def motion(verts, edge, seed=7):
    """End positions x1 = x0 + N(0, 0.3 edge) per coordinate (the restatement's and the device's x1 at k = 0)."""
    g = np.random.default_rng(seed)
    return np.asarray(verts, dtype=np.float64) + g.normal(0.0, 0.3 * edge, np.shape(verts))


def scaled(x, k):
    """x 2^k, exact for the arrays and scales used here."""
    return np.ldexp(np.asarray(x, dtype=np.float64), k)


# ---------------------------------------------------------------- the inside query's points and restated answers (cached, never modified)
INSIDE_RANDOM = 500


@functools.lru_cache(maxsize=None)
def _meshes():
    return meshes()


@functools.lru_cache(maxsize=None)
def inside_points(name, axis):
    """The points of the inside query on mesh `name` at k = 0: INSIDE_RANDOM uniform in its bounding box, then every tenth vertex moved
    half an edge down the axis (its other two coordinates are the vertex's exactly: column_tri's tie rule decides).  Another scale
    takes scaled() of these, never points of its own."""
    v, _, edge = _meshes()[name]
    g = np.random.default_rng(50 + axis)
    under = v[::10].copy()
    under[:, axis] -= edge / 2
    return np.ascontiguousarray(np.concatenate([g.uniform(v.min(axis=0), v.max(axis=0), size=(INSIDE_RANDOM, 3)), under]))


@functools.lru_cache(maxsize=None)
def want_inside(name, axis, k=0, parity=False, shift=0.0):
    """column_ref.points_inside of the points on the mesh, both translated by `shift` and then scaled by 2^k."""
    import column_ref
    v, vidx, _ = _meshes()[name]
    return column_ref.points_inside(scaled(inside_points(name, axis) + shift, k), scaled(v + shift, k), vidx, axis, parity)
