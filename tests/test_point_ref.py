"""The point predicate's numpy restatement (tests/point_ref.py) against exact rational arithmetic, its scale equivariance, the tie rule
of the closest-point query, and the C ABI of the two new entry points without a device.  No GPU.

Scales.  pt_tri works on the triangle translated to the point and scaled so that the largest |component| m of p0 - p, p1 - p, p2 - p
lies in [0.5, 1): every rounding is a relative 2^-53 of an O(1) number, so the errors of dist and of the closest point q are
absolute in units of m, not relative to dist (a point ON the triangle has dist = 0 exactly and gets a few 2^-53 m).  The face
term's barycentrics carry the conditioning kappa = |e1|^2 |e2|^2 / den (one over the squared sine of the corner at p0), so on a
sliver q from the face term may lie a few 2^-53 kappa m along the triangle from the exact closest point; it still is a convex
combination of the vertices, so dist is never BELOW the exact distance by more than the rounding of forming it, and the edge terms
keep it within the sliver's width above.

Measured here (the classes of point_ref.WELL_CONDITIONED, N_EXACT pairs each, kappa <= 2^10):
    max |dist - sqrt(d2_exact)| / m : 3.00e-14 (below the exact distance: 2.77e-16)          max |q - q_exact|_inf / m : 2.17e-14
(the conditioning shows: up to kappa = 2^10 times the 2^-53 of one rounding; on the side that matters to the walk's filter, dist BELOW
the exact distance, it does not).  The sets are samples, not a worst case: 4 x the larger figure is asserted (ERR_BOUND), for dist and for q alike.

Features.  The feature is decided by the signs of the plane projection's three barycentrics and of t, 1 - t on the three edges (all
unclamped).  Their computed values are off by a few 2^-53 kappa rho, rho = 1 + |p - p0| / min(|e1|, |e2|); with kappa, rho <= 2^10 that
is below 2^-30, so a pair whose exact quantities are all at least MARGIN = 2^-20 away from 0 must report the exact feature."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import mi355cd
import point_ref as ptr
import scale_inputs as si
from conftest import has_gpu

N_EXACT = 300
ERR_MEASURED = 3.00e-14
ERR_BOUND = 4.0 * ERR_MEASURED
MARGIN = 2.0 ** -20
KAPPA_MAX = 2.0 ** 10


def _isqrt_float(fr):
    """sqrt of a non-negative Fraction, correct to a relative 2^-100 (integer square root of a scaled numerator)."""
    if fr == 0:
        return Fraction(0)
    sh = 2 * max(0, 120 - (fr.numerator.bit_length() - fr.denominator.bit_length()) // 2)
    return Fraction(math.isqrt((fr.numerator << sh) // fr.denominator), 1 << (sh // 2))


def _table():
    rows = []
    for name, (pts, tris) in ptr.pair_classes(N_EXACT, seed=5).items():
        dist, q, u, v, f, side = ptr.pt_tri_np(pts, tris)
        for i in range(pts.shape[0]):
            rows.append((name, i, pts[i], tris[i], dist[i], q[i], u[i], v[i], int(f[i]), int(side[i]), ptr.exact_pt_tri(pts[i], tris[i])))
    return rows


@pytest.fixture(scope="module")
def table():
    return _table()


def _cond(pt, tri):
    """(m, kappa, rho) in floats; kappa = inf for a degenerate triangle."""
    e1, e2, ap = tri[1] - tri[0], tri[2] - tri[0], pt - tri[0]
    m = float(np.abs(tri - pt).max())
    d00, d01, d11 = float(e1 @ e1), float(e1 @ e2), float(e2 @ e2)
    den = d00 * d11 - d01 * d01
    kappa = d00 * d11 / den if den > 0 else math.inf
    l = min(math.sqrt(d00), math.sqrt(d11))
    rho = 1.0 + (math.sqrt(float(ap @ ap)) / l if l > 0 else math.inf)
    return m, kappa, rho


def _errors(row):
    name, i, pt, tri, dist, q, u, v, f, side, (d2, eq, euv, ef, es, params) = row
    m, kappa, rho = _cond(pt, tri)
    if m == 0.0:
        return 0.0, 0.0, m, kappa, rho
    e_d = float(Fraction(float(dist)) - _isqrt_float(d2)) / m                  # signed: negative = below the exact distance
    e_q = max(abs(float(Fraction(float(q[k])) - eq[k])) for k in range(3)) / m
    return e_d, e_q, m, kappa, rho


def test_dist_and_closest_point_agree_with_exact_on_well_conditioned_pairs(table):
    worst_d, worst_q, below, n = 0.0, 0.0, 0.0, 0
    for row in table:
        if row[0] not in ptr.WELL_CONDITIONED:
            continue
        e_d, e_q, m, kappa, rho = _errors(row)
        if not kappa <= KAPPA_MAX:
            continue
        n += 1
        worst_d, worst_q, below = max(worst_d, abs(e_d)), max(worst_q, e_q), max(below, -e_d)
    print(f"well-conditioned pairs: {n}; max |dist - exact| / m = {worst_d:.3e} (below exact: {below:.3e}); max |q - q_exact| / m = {worst_q:.3e}; asserted {ERR_BOUND:.3e}")
    assert n > 4 * N_EXACT
    assert worst_d <= ERR_BOUND and worst_q <= ERR_BOUND


def test_slivers_and_degenerate_triangles_get_the_distance_of_the_point_set_they_are(table):
    """dist is never below the exact distance by more than the bound, and above it by at most the bound times the conditioning (a
    degenerate triangle's face term is +inf or a convex combination of collinear vertices: its edges decide, with no conditioning)."""
    n, worst_below, worst_above = 0, 0.0, 0.0
    for row in table:
        if row[0] not in ("sliver", "degenerate"):
            continue
        e_d, e_q, m, kappa, rho = _errors(row)
        n += 1
        worst_below, worst_above = max(worst_below, -e_d), max(worst_above, e_d)
        assert e_d >= -ERR_BOUND, (row[0], row[1], e_d)
        assert e_d <= ERR_BOUND * (kappa if math.isfinite(kappa) else 1.0), (row[0], row[1], e_d, kappa)
        assert math.isfinite(row[4]) and np.isfinite(row[5]).all()
    print(f"slivers and degenerate: {n} pairs; dist below exact by at most {worst_below:.3e} m, above by at most {worst_above:.3e} m")
    assert n == 2 * N_EXACT
    # three coincident vertices AT the point
    z = np.array([[0.25, -1.5, 3.0]])
    dist, q, u, v, f, side = ptr.pt_tri_np(z, np.repeat(z, 3, axis=0)[None])
    assert dist[0] == 0.0 and (q[0] == z[0]).all() and u[0] == 0.0 and v[0] == 0.0 and f[0] == 4 and side[0] == 0
    # a segment and a point, exactly
    seg = np.array([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])
    dist, q, u, v, f, side = ptr.pt_tri_np(np.array([[0.5, 3.0, 4.0]]), seg)
    assert dist[0] == 5.0 and (q[0] == [0.5, 0.0, 0.0]).all()
    dist, q, u, v, f, side = ptr.pt_tri_np(np.array([[3.0, 4.0, 0.0]]), np.zeros((1, 3, 3)))
    assert dist[0] == 5.0 and f[0] == 4 and (q[0] == 0.0).all()


def test_feature_and_side_agree_with_exact_where_decided(table):
    decided = {}
    for name, i, pt, tri, dist, q, u, v, f, side, (d2, eq, euv, ef, es, params) in table:
        m, kappa, rho = _cond(pt, tri)
        if not (kappa <= KAPPA_MAX and rho <= KAPPA_MAX) or any(x is None for x in params):
            continue
        if min(abs(float(x)) for x in params) < MARGIN:
            continue
        decided[name] = decided.get(name, 0) + 1
        assert f == ef, (name, i, f, ef, [float(x) for x in params])
        # (u, v) name the same point as the exact barycentrics
        assert abs(u - float(euv[0])) <= 2.0 ** -30 and abs(v - float(euv[1])) <= 2.0 ** -30, (name, i)
        # side: decided when p is off the plane by a margin (relative to m: the normal is a product of two O(m) edges)
        e1, e2, ap = tri[1] - tri[0], tri[2] - tri[0], pt - tri[0]
        nrm = np.cross(e1, e2)
        h = abs(float(ap @ nrm)) / max(float(np.sqrt(nrm @ nrm)), 1e-300)
        if h >= MARGIN * m:
            assert side == es, (name, i)
    print("decided pairs per class:", decided)
    assert decided.get("random", 0) > N_EXACT // 2 and decided.get("scaled", 0) > N_EXACT // 2
    assert sum(decided.values()) > 2 * N_EXACT


def test_features_on_a_right_triangle():
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    one = lambda x, y, z: tuple(a[0] for a in ptr.pt_tri_np(np.array([[x, y, z]]), tri))
    dist, q, u, v, f, side = one(0.25, 0.25, 2.0)
    assert (dist, u, v, f, side) == (2.0, 0.25, 0.25, 0, 1) and (q == [0.25, 0.25, 0.0]).all()
    assert one(0.25, 0.25, -2.0)[4:] == (0, 0)                                  # below: the other side of the plane
    dist, q, u, v, f, side = one(0.5, -1.0, 0.0)
    assert (dist, u, v, f) == (1.0, 0.5, 0.0, 1)                                # edge 01
    dist, q, u, v, f, side = one(1.0, 1.0, 0.0)
    assert (u, v, f) == (0.5, 0.5, 2) and dist == math.sqrt(0.5)                # edge 12
    dist, q, u, v, f, side = one(-1.0, 0.5, 0.0)
    assert (dist, u, v, f) == (1.0, 0.0, 0.5, 3)                                # edge 20
    assert one(-1.0, -1.0, 0.0)[2:5] == (0.0, 0.0, 4)                           # vertex 0
    assert one(3.0, -1.0, 0.0)[2:5] == (1.0, 0.0, 5)                            # vertex 1
    assert one(-1.0, 3.0, 0.0)[2:5] == (0.0, 1.0, 6)                            # vertex 2
    assert one(0.5, 0.0, 0.0)[4] == 0 and one(0.5, 0.0, 0.0)[0] == 0.0          # ON an edge: the face term (closed) keeps the tie
    assert one(1.0, 0.0, 0.0)[0] == 0.0 and (one(1.0, 0.0, 0.0)[1] == [1.0, 0.0, 0.0]).all()


def test_restatement_is_equivariant_under_power_of_two_scaling():
    for name, (pts, tris) in ptr.pair_classes(4096, seed=9).items():
        if name == "scaled":
            continue                                                            # (already at 2^+-100)
        base = ptr.pt_tri_np(pts, tris)
        assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all() and np.isfinite(base[2]).all() and np.isfinite(base[3]).all()
        for k in si.SCALES:
            got = ptr.pt_tri_np(np.ldexp(pts, k), np.ldexp(tris, k))
            want = (np.ldexp(base[0], k), np.ldexp(base[1], k)) + base[2:]
            for a, b, what in zip(want, got, ("dist", "q", "u", "v", "feature", "side")):
                assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), (name, k, what)


def test_finite_input_gives_no_nan():
    g = np.random.default_rng(3)
    n = 20000
    mag = np.ldexp(1.0, g.integers(-1000, 1000, (n, 1, 1)))
    tris = g.uniform(-1, 1, (n, 3, 3)) * mag * np.ldexp(1.0, g.integers(-40, 1, (n, 3, 1)))
    pts = g.uniform(-1, 1, (n, 3)) * mag[:, 0] * np.ldexp(1.0, g.integers(-40, 1, (n, 1)))
    tris[::7, 1] = tris[::7, 0]
    tris[::11] = 0.0
    pts[::13] = tris[::13, 2]
    for out in ptr.pt_tri_np(pts, tris):
        assert not np.isnan(out).any()
    ends = np.array([[np.finfo(np.float64).max, -np.finfo(np.float64).max, 5e-324]])
    for out in ptr.pt_tri_np(np.concatenate([ends, -ends, np.zeros((1, 3))]), np.stack([np.stack([ends[0], -ends[0], ends[0] * 0])] * 3)):
        assert not np.isnan(out).any()


def test_tie_rule_picks_the_smaller_id_then_the_smaller_face_index():
    import query_meshes as qm
    v, i, ids, edge = next(m[1:] for m in qm._meshes() if m[0] == "duplicates")
    nt = i.shape[0]
    tris = np.asarray(v)[np.asarray(i).astype(np.int64)]
    pts = ptr.mesh_points(v, i, 512, seed=1, edge=edge)
    face, oid, dist, q, uv, feat, side = ptr.closest_points_ref(v, i, None, pts)
    assert (face != ptr.NONE).all()
    first = {}
    for f in range(nt):                                                         # same geometry, two IDs: the first face of each geometry
        first.setdefault(tris[f].tobytes(), f)
    dup = np.array([first[tris[f].tobytes()] != f for f in range(nt)])
    assert dup.sum() >= 150 and not dup[face].any()                             # never the copy with the larger ID
    assert np.array_equal(oid, face)                                            # IDs = face indices here
    ids2 = (nt - 1 - np.arange(nt)).astype(np.uint32)                           # reversed IDs: now the LATER copy has the smaller ID
    face2 = ptr.closest_points_ref(v, i, ids2, pts)[0]
    hit_dup = np.array([tris[f].tobytes() in {tris[g].tobytes() for g in np.nonzero(dup)[0]} for f in face])
    assert hit_dup.sum() > 20 and dup[face2[hit_dup]].all()
    same_id = np.zeros(nt, dtype=np.uint32)                                     # all IDs equal: the smaller face index
    assert np.array_equal(ptr.closest_points_ref(v, i, same_id, pts)[0], face)


def test_closest_points_ref_is_the_all_pairs_minimum_and_honours_rmax():
    import mi355_synth as synth
    verts, vidx = synth.soup(300, e=0.3, seed=2)
    pts = ptr.mesh_points(verts, vidx, 256, seed=1, edge=0.3)
    ids = np.random.default_rng(3).integers(0, 40, vidx.shape[0]).astype(np.uint32)      # many equal IDs
    tris = verts[vidx.astype(np.int64)]
    inf = ptr.closest_points_ref(verts, vidx, ids, pts, pairs_per_chunk=7 * 300)
    rm = ptr.radii(inf[2], 0.3, seed=2)
    got = ptr.closest_points_ref(verts, vidx, ids, pts, rm, pairs_per_chunk=5 * 300)
    nf = 0
    for k in range(pts.shape[0]):
        d, q, u, v, f, s = ptr.pt_tri_np(np.repeat(pts[k:k + 1], tris.shape[0], axis=0), tris)
        ok = np.nonzero(d <= rm[k])[0]
        if ok.size == 0:
            assert got[0][k] == ptr.NONE and got[2][k] == np.inf and got[1][k] == 0 and not got[3][k].any() and not got[4][k].any() and got[5][k] == 0 and got[6][k] == 0
            continue
        nf += 1
        best = min((d[j], ids[j], j) for j in ok)
        j = best[2]
        assert (got[2][k], got[1][k], got[0][k]) == best
        assert (got[3][k] == q[j]).all() and got[4][k, 0] == u[j] and got[4][k, 1] == v[j] and got[5][k] == f[j] and got[6][k] == s[j]
    assert 64 < nf < 224, nf                                                    # a good share finds something, a good share nothing
    assert (got[0][2::4] != ptr.NONE).all()                                     # rmax == the nearest distance: closed, found


def test_argument_errors_of_the_point_calls_do_not_need_a_device():
    lib = mi355cd.load_library()
    assert lib.cd_closest_points(None, None, 0, 0, None, None, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG
    pts = np.zeros((1, 4)); face = np.zeros(1, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.cd_closest_points(None, vp(pts), 1, 0, vp(face), None, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_pt_tri_points(None, None, 4, None, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_pt_tri_points(vp(pts), None, 1, None, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert C.sizeof(mi355cd.CdPointInfo) == 24 and mi355cd.CD_POINT_ANY == 1
    assert mi355cd.pack_points(np.zeros((5, 3)), 2.0).shape == (5, 4) and (mi355cd.pack_points(np.zeros((5, 3)))[:, 3] == np.inf).all()


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a box without a GPU")
def test_pt_tri_points_without_a_device_is_an_error_not_a_fallback():
    with pytest.raises(mi355cd.CdError) as e:
        mi355cd.pt_tri_points(np.zeros((2, 3)), np.zeros((2, 3, 3)))
    assert e.value.rc == mi355cd.CD_ERR_NO_DEVICE
