"""cd_points_inside, cd_signed_distance and cd_column_tri_points on the device against the numpy restatement (tests/column_ref.py),
against closed-form answers on the closed meshes of tests/closed_meshes.py, and against the invariants the header states."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import closed_meshes as cm
import column_ref as ref
import mi355cd
import scale_inputs as si

pytestmark = pytest.mark.gpu

CAP = 1 << 20
AXES = (0, 1, 2)
NAMES = ("inside", "n_above", "n_below", "w_above", "w_below")


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _same_bits(got, want, what):
    """Bit for bit where the restatement is a number; a NaN where it is a NaN (payloads are not compared)."""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), what
    assert np.array_equal(_bits(g[~nan]), _bits(w[~nan])), what


def _ctx(v, f):
    cd = mi355cd.CollisionDetector(v, f)
    cd.build_tree()
    return cd


def _same(got, want, what):
    """points_inside's five arrays against the restatement's; info.n_inside against the count."""
    for name, g, w in zip(NAMES, got[:5], want):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert bad.size == 0 and g.dtype == w.dtype, (what, name, bad.size, bad[:4], np.asarray(g)[bad[:4]], np.asarray(w)[bad[:4]])
    assert got[5].n_inside == int(np.asarray(want[0]).sum()), (what, got[5].n_inside)


# ---------------------------------------------------------------- the inputs and their restated answers, computed once
@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "box":
        return cm.box_grid(4)
    if name == "torus":
        return cm.torus(24, 12)
    if name == "torus64":
        return cm.torus(64, 32)
    if name == "torus_far":
        v, f = cm.torus(24, 12)
        return cm.rotated(v), f
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _points(name, axis):
    if name == "box":
        return cm.lattice(axis)
    if name == "torus":                                        # under every vertex and edge midpoint, plus random ones
        v, f = _mesh("torus")
        e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), axis=1), axis=0)
        under = np.concatenate([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]])])
        under[:, axis] -= 0.01                                 # (off the surface; the other two coordinates are the vertex's, exactly)
        return np.ascontiguousarray(np.concatenate([under, cm.torus_points(600, seed=5 + axis)[0]]))
    if name == "torus64":
        return cm.torus_points(1200, seed=20 + axis)[0][:1000]
    if name == "torus_far":
        v, f = _mesh("torus_far")
        g = np.random.default_rng(30 + axis)
        lo, hi = v.min(axis=0), v.max(axis=0)
        under = v[::3].copy()
        under[:, axis] -= 0.01
        return np.ascontiguousarray(np.concatenate([under, g.uniform(lo, hi, size=(500, 3))]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name, axis, parity=False):
    v, f = _mesh(name)
    return ref.points_inside(_points(name, axis), v, f, axis, parity)


# ---------------------------------------------------------------- the pin of the device function
def _planted():
    """(point, triangle) rows where the tie rule decides, degenerate and NaN operands (axis 2 in mind; every axis is run)."""
    t = [[0.0, 0.0, 1.0], [1.0, 0.0, 2.0], [0.0, 1.0, 3.0]]
    m = [[1.0, 0.0, 2.0], [1.0, 1.0, 0.5], [0.0, 1.0, 3.0]]
    rows = []
    for tri in (t, m, t[::-1], m[::-1], [t[1], t[2], t[0]]):
        for p in ([0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0], [0.25, 0, 0], [0, 0.25, 0], [1, 0.5, 0], [0.5, 1, 0], [0.25, 0.25, 1.5],
                  [0.25, 0.25, 9.0], [2, 2, 0]):
            rows.append((p, tri))
    flat_b = [[0.0, 0.5, 0.0], [1.0, 0.5, 1.0], [0.5, 1.0, 2.0]]                 # an edge with equal b (and equal a on another axis)
    for p in ([0.5, 0.5, 0], [0.0, 0.5, 0], [1.0, 0.5, 0], [0.25, 0.5, 7]):
        rows += [(p, flat_b), (p, flat_b[::-1])]
    line = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 5.0]]
    dot = [[1.0, 1.0, 1.0]] * 3
    for p in ([1, 1, 0], [0.5, 0.5, 0], [1, 1, 1]):
        rows += [(p, line), (p, dot), (p, [dot[0], dot[0], [2.0, 2.0, 2.0]])]
    nan = float("nan")
    for k in range(9):
        tri = np.array(t).reshape(-1)
        tri[k] = nan
        rows.append(([0.25, 0.25, 0.0], tri.reshape(3, 3).tolist()))
    rows.append(([nan, 0.25, 0.0], t))
    rows.append(([0.25, 0.25, nan], t))
    rows.append(([0.25, 0.25, float("inf")], t))
    return np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows], dtype=np.float64)


@pytest.mark.parametrize("axis", AXES)
def test_column_tri_pin(axis):
    g = np.random.default_rng(40 + axis)
    n = 100000
    tri = g.uniform(-1.0, 1.0, size=(n, 3, 3))
    p = g.uniform(-1.0, 1.0, size=(n, 3))
    k = n // 2                                                                   # half of them over their triangle, so that covers are common
    w = g.dirichlet([1.0, 1.0, 1.0], size=k)
    p[:k] = np.einsum("ij,ijk->ik", w, tri[:k])
    p[:k, axis] += g.uniform(-0.5, 0.5, size=k)
    grid = np.round(g.uniform(-2, 2, size=(20000, 3, 3)))                        # small integers: exact zeros of E, equal coordinates
    gp = np.round(g.uniform(-2, 2, size=(20000, 3)))
    pp, pt = _planted()
    pts, tris = np.concatenate([p, gp, pp]), np.concatenate([tri, grid, pt])
    want = ref.column_tri(pts, tris, axis)
    cover, above, E, zc, S = mi355cd.column_tri_points(pts, tris, axis)
    assert cover.dtype == np.int8 and np.array_equal(cover, want["cover"])
    assert np.array_equal(above, want["above"])
    _same_bits(E, want["E"], "E")
    _same_bits(zc, want["zc"], "zc")
    _same_bits(S, want["S"], "S")
    assert (want["cover"][:n] != 0).sum() > n // 4 and (want["cover"][n:n + 20000] != 0).sum() > 500
    ties = (want["E"][n:n + 20000] == 0).any(axis=1) & (want["cover"][n:n + 20000] != 0)
    assert ties.sum() > 100, "the tie rule decided no cover: nothing here would test it"
    only_cover = np.zeros(pts.shape[0], dtype=np.int8)                           # every output but cover may be NULL
    assert mi355cd.load_library().cd_column_tri_points(pts.ctypes.data, np.ascontiguousarray(tris).ctypes.data, pts.shape[0], axis, only_cover.ctypes.data,
                                                        None, None, None, None) == mi355cd.CD_OK
    assert np.array_equal(only_cover, cover)


# ---------------------------------------------------------------- results against the restatement
@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("name", ["box", "torus", "torus64", "torus_far"])
def test_against_restatement(name, axis):
    v, f = _mesh(name)
    pts = _points(name, axis)
    with _ctx(v, f) as cd:
        got = cd.points_inside(pts, axis)
        _same(got, _want(name, axis), f"{name} axis {axis}")
        _same(cd.points_inside(pts, axis, parity=True), _want(name, axis, True), f"{name} axis {axis} parity")
        assert got[5].tri_tests >= int(got[1].sum() + got[2].sum()) and got[5].node_visits > 0
    if name != "torus_far":                                                      # the stated invariants, on the device output itself
        assert not (got[3] + got[4]).any(), "w_above + w_below != 0 on a closed mesh"
        assert np.array_equal(got[0], (got[1] & 1) != 0), "parity differs from winding"
    if name == "box":
        assert np.array_equal(got[0], cm.lattice_inside(pts, axis))


def test_torus_inside_is_the_same_on_every_axis_and_analytic():
    pts, want = cm.torus_points()
    with _ctx(*_mesh("torus")) as cd:
        res = [cd.points_inside(pts, axis) for axis in AXES]
        sd = [cd.signed_distance(pts, axis) for axis in AXES]
    for axis, r in zip(AXES, res):
        assert np.array_equal(r[0], want), axis
        assert not (r[3] + r[4]).any() and np.array_equal(r[0], (r[1] & 1) != 0)
    for s in sd:
        assert np.array_equal(s[0] < 0, want) and np.array_equal(s[6], want)


def test_inverted_mesh_negates_the_winding():
    v, f = _mesh("box")
    pts = _points("box", 2)
    inside, na, nb, wa, wb = _want("box", 2)
    with _ctx(v, cm.inverted(f)) as cd:
        _same(cd.points_inside(pts, 2), (inside, na, nb, -wa, -wb), "inverted box")
    between = np.array([[0.125, 0.5, 0.5], [0.5, 0.5, 0.125]])
    core = np.array([[0.5, 0.5, 0.5]])
    for invert, w_core in ((True, 0), (False, 2)):
        with _ctx(*cm.nested_boxes(4, invert)) as cd:
            for axis in AXES:
                assert np.array_equal(cd.points_inside(between, axis)[3], [1, 1]) and cd.points_inside(core, axis)[3][0] == w_core


def test_open_mesh_shows_the_hole():
    v, f, _ = cm.open_box(4)
    pts = cm.lattice(2)
    with _ctx(v, f) as cd:
        got = cd.points_inside(pts, 2)
        _same(got, ref.points_inside(pts, v, f, 2), "open box")
        hole = (0 <= pts[:, 0]) & (pts[:, 0] < 1) & (0 <= pts[:, 1]) & (pts[:, 1] < 1)
        assert np.array_equal((got[3] + got[4]) != 0, hole)
        px = cm.lattice(0)
        gx = cd.points_inside(px, 0)
        assert not (gx[3] + gx[4]).any() and np.array_equal(gx[0], cm.lattice_inside(px, 0))


# ---------------------------------------------------------------- shapes
def test_one_and_two_triangles():
    tri = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0]])
    g = np.random.default_rng(3)
    pts = np.concatenate([g.uniform(-0.2, 1.2, size=(200, 3)), [[0, 0, 0], [1, 0, 0], [0.5, 0.5, 0], [0.5, 0.5, 2], [1, 1, 0], [0.25, 0, 0]]])
    for f in (np.array([[0, 1, 2]], dtype=np.uint32), np.array([[0, 1, 2], [1, 3, 2]], dtype=np.uint32)):
        with _ctx(tri, f) as cd:
            for axis in AXES:
                got = cd.points_inside(pts, axis)
                want = ref.points_inside(pts, tri, f, axis)
                _same(got, want, f"{f.shape[0]} triangles axis {axis}")
                if f.shape[0] == 1:
                    assert got[5].node_visits == 0 and got[5].tri_tests == pts.shape[0]
            assert cd.points_inside(pts, 2)[1].sum() > 20


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_point_counts(n):
    pts = _points("torus", 2)[100:100 + n]
    want = tuple(a[100:100 + n] for a in _want("torus", 2))
    with _ctx(*_mesh("torus")) as cd:
        got = cd.points_inside(pts, 2)
        _same(got, want, f"n = {n}")
        assert all(a.shape == (n,) for a in got[:5])
        sd = cd.signed_distance(pts, 2)
        assert sd[0].shape == (n,) and np.array_equal(sd[6], want[0])
        if n == 0:
            assert (got[5].n_inside, got[5].node_visits, got[5].tri_tests) == (0, 0, 0)


# ---------------------------------------------------------------- independence
def test_independent_of_frame_traversal_cell_table_and_order():
    v, f = _mesh("torus64")
    pts = _points("torus64", 2)
    want = _want("torus64", 2)
    perm = np.random.default_rng(9).permutation(pts.shape[0])
    with mi355cd.CollisionDetector(v, f) as cd:
        for frame in (mi355cd.CD_FRAME_REFERENCE, mi355cd.CD_FRAME_AUTO):
            for trav in (0, 1, 3):
                for table in (0, 1):
                    cd.set_option(mi355cd.CD_OPT_TRAVERSAL, trav)
                    cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
                    cd.set_morton_frame(frame)
                    cd.self_collide(cap=CAP)                                     # the tree of this setting (the collision step builds it)
                    _same(cd.points_inside(pts, 2), want, f"frame {frame} traversal {trav} cell table {table}")
        cd.build_tree()
        got = cd.points_inside(pts[perm], 2)
        _same(got, tuple(a[perm] for a in want), "permuted points")
        for axis in (0, 1):
            _same(cd.points_inside(_points("torus64", axis), axis), _want("torus64", axis), f"axis {axis}")


@pytest.mark.parametrize("k", [-100, 0, 100])
@pytest.mark.parametrize("name", ["box", "torus"])
def test_scaled_by_a_power_of_two(name, k):
    v, f = _mesh(name)
    with _ctx(np.ldexp(v, k), f) as cd:
        for axis in AXES:
            _same(cd.points_inside(np.ldexp(_points(name, axis), k), axis), _want(name, axis), f"{name} 2^{k} axis {axis}")


# ---------------------------------------------------------------- the fp32 range
SCALE_MESHES = si.meshes()
FRAMES = ((mi355cd.CD_FRAME_REFERENCE, "reference"), (mi355cd.CD_FRAME_AUTO, "auto"))
SHIFT = 2.0 ** 20 + 0.37


def _run_all(cd, pts, want, want_parity, parity_axis, what):
    """Both cell-table settings and the Morton frames, on the tree cd_self_collide builds for each (test_query_scales_gpu.py's _run_all).
    pts: the points per axis; want: per axis the lists of restated answers the device must equal (the same integers in each);
    want_parity: the restated answer with parity on parity_axis."""
    for table in (1, 0):
        cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
        for frame, fname in FRAMES:
            w = f"{what} table={table} frame={fname}"
            cd.set_morton_frame(frame)
            assert cd.self_collide(cap=CAP)[2] == mi355cd.CD_OK, w
            for axis in AXES:
                got = cd.points_inside(pts[axis], axis)
                for j, ww in enumerate(want[axis]):
                    _same(got, ww, f"{w} axis {axis} restatement {j}")
                sd = cd.signed_distance(pts[axis], axis)
                assert np.array_equal(sd[6], want[axis][0][0]), f"{w} axis {axis} signed distance"
                assert np.array_equal(_bits(np.abs(sd[0])), _bits(cd.closest_points(pts[axis])[2])), f"{w} axis {axis} |sdist|"
                assert np.array_equal(np.signbit(sd[0]), sd[6] & (np.abs(sd[0]) > 0)), f"{w} axis {axis} sign"
            _same(cd.points_inside(pts[parity_axis], parity_axis, parity=True), want_parity, f"{w} axis {parity_axis} parity")


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """tests/scale_inputs.py's meshes and inside points scaled by 2^k, past FLT_MAX (stored bounds of +-inf) and below the smallest
    fp32 subnormal (all +-0): the k = 0 restatement's integers on every axis (tests/test_column_ref.py: the restatement is
    equivariant there), and at si.EDGES the restatement on the scaled inputs itself; parity on one axis; cd_signed_distance's inside
    and the bits of its |sdist| against cd_closest_points."""
    v, vidx, edge = SCALE_MESHES[name]
    verts = si.scaled(v, k)
    if k >= 128:                                                                 # the range end is really reached: the FLT_MAX cell is ambiguous
        for a in AXES:
            assert np.unique(verts[np.abs(verts[:, a]) > si.FLT_MAX, a]).size >= 2, (name, k, a)
    pts = [si.scaled(si.inside_points(name, a), k) for a in AXES]
    want = [[si.want_inside(name, a)] + ([si.want_inside(name, a, k)] if k in si.EDGES else []) for a in AXES]
    pa = k % 3
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        _run_all(cd, pts, want, si.want_inside(name, pa, 0, True), pa, f"{name} k={k}")


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_by_2_pow_20(name):
    """World coordinates: mesh and points translated by 2^20 + 0.37 (the pad 2^-20 max(M, |p|) is then several edges wide, and the
    points under a vertex still have its other two coordinates exactly), against the restatement on the translated inputs."""
    v, vidx, edge = SCALE_MESHES[name]
    pts = [si.inside_points(name, a) + SHIFT for a in AXES]
    want = [[si.want_inside(name, a, 0, False, SHIFT)] for a in AXES]
    assert all(int(((w[0][1] + w[0][2]) > 0).sum()) >= 200 for w in want), name
    with mi355cd.CollisionDetector(v + SHIFT, vidx) as cd:
        _run_all(cd, pts, want, si.want_inside(name, 1, 0, True, SHIFT), 1, f"{name} translated")


# ---------------------------------------------------------------- the signed distance
@pytest.mark.parametrize("axis", AXES)
def test_signed_distance_is_closest_points_with_the_sign(axis):
    pts = _points("torus", axis)
    with _ctx(*_mesh("torus")) as cd:
        face, ids, dist, closest, uv, feature, side, _ = cd.closest_points(pts)
        inside = cd.points_inside(pts, axis)[0]
        sd, sface, sids, sclosest, suv, sfeature, sinside, info = cd.signed_distance(pts, axis)
        par = cd.signed_distance(pts, axis, parity=True)
    assert np.array_equal(_bits(np.abs(sd)), _bits(dist)) and np.array_equal(sface, face) and np.array_equal(sids, ids)
    assert np.array_equal(_bits(sclosest), _bits(closest)) and np.array_equal(_bits(suv), _bits(uv)) and np.array_equal(sfeature, feature)
    assert np.array_equal(sinside, inside) and np.array_equal(np.signbit(sd), inside & (dist > 0))
    assert np.array_equal(sinside, _want("torus", axis)[0]) and info.n_found == pts.shape[0]
    assert np.array_equal(par[6], _want("torus", axis, True)[0]) and np.array_equal(_bits(par[0]), _bits(sd))


def test_signed_distance_zero_stays_positive_and_null_outputs():
    v, f = _mesh("box")
    pts = np.array([[0.5, 0.5, 0.5], [0.25, 0.25, 0.0], [0.5, 0.5, 1.0], [2.0, 0.5, 0.5], [0.5, 0.5, 0.25]])
    lib = mi355cd.load_library()
    with _ctx(v, f) as cd:
        sd, _, _, _, _, _, inside, _ = cd.signed_distance(pts, 2)
        assert np.array_equal(_bits(sd), _bits([-0.5, 0.0, 0.0, 1.0, -0.25])), sd     # on the surface: +0 whichever side it is given
        assert inside[0] and inside[4] and not inside[3]
        only = np.full(pts.shape[0] + 4, -7.0)
        assert lib.cd_signed_distance(cd._ctx, pts.ctypes.data, pts.shape[0], 2, 0, only.ctypes.data, None, None, None, None, None, None, None) == mi355cd.CD_OK
        assert np.array_equal(_bits(only[:-4]), _bits(sd)) and (only[-4:] == -7.0).all()
        ins = np.full(pts.shape[0] + 4, 7, dtype=np.uint8)
        assert lib.cd_points_inside(cd._ctx, pts.ctypes.data, pts.shape[0], 2, 0, ins.ctypes.data, None, None, None, None, None) == mi355cd.CD_OK
        assert np.array_equal(ins[:-4].astype(bool), inside) and (ins[-4:] == 7).all()


# ---------------------------------------------------------------- the use case: a contained object
def test_contained_object_is_seen():
    tv, tf = _mesh("torus")
    bv, bf = cm.box_grid(4, -0.1, 0.1)
    bv = bv + np.array([1.0, 0.0, 0.0])                                          # wholly inside the tube
    with _ctx(tv, tf) as t, _ctx(bv, bf) as b:
        pairs, n, rc = t.find_collisions_between(b, cap=CAP)
        assert rc == mi355cd.CD_OK and n == 0
        for axis in AXES:
            assert t.points_inside(bv, axis)[0].all()
            assert (t.signed_distance(bv, axis)[0] < 0).all()
        assert not b.points_inside(tv, 2)[0].any()                               # and the torus is not inside the box


# ---------------------------------------------------------------- errors and state
def _raw(lib, ctx, pts, axis, flags):
    n = pts.shape[0]
    out = [np.full(n + 4, 7, dtype=np.uint8), np.full(n + 4, 7, dtype=np.uint32), np.full(n + 4, 7, dtype=np.uint32), np.full(n + 4, 7, dtype=np.int32),
           np.full(n + 4, 7, dtype=np.int32)]
    info = mi355cd.CdInsideInfo(5, 5, 5)
    rc = lib.cd_points_inside(ctx, pts.ctypes.data if n else None, n, axis, flags, *[a.ctypes.data for a in out], C.byref(info))
    sd = np.full(n + 4, -7.0)
    pinfo = mi355cd.CdPointInfo(5, 5, 5)
    rc2 = lib.cd_signed_distance(ctx, pts.ctypes.data if n else None, n, axis, flags, sd.ctypes.data, None, None, None, None, None, out[0].ctypes.data, C.byref(pinfo))
    untouched = all((a == 7).all() for a in out) and (sd == -7.0).all() and (info.n_inside, info.node_visits, info.tri_tests) == (5, 5, 5) \
        and (pinfo.n_found, pinfo.node_visits, pinfo.tri_tests) == (5, 5, 5)
    return rc, rc2, untouched


def test_errors():
    lib = mi355cd.load_library()
    v, f = _mesh("torus")
    pts = np.ascontiguousarray(_points("torus", 2)[:70])
    bad = pts.copy()
    bad[69, 1] = np.nan
    inf = pts.copy()
    inf[0, 2] = np.inf
    with mi355cd.CollisionDetector(v, f) as cd:
        assert _raw(lib, cd._ctx, pts, 2, 0) == (mi355cd.CD_ERR_ORDER, mi355cd.CD_ERR_ORDER, True)       # no tree yet
        cd.build_tree()
        for p, axis, flags in ((pts, 3, 0), (pts, -1, 0), (pts, 2, 2), (pts, 2, 3), (pts, 2, -1), (bad, 2, 0), (inf, 0, 1)):
            assert _raw(lib, cd._ctx, p, axis, flags) == (mi355cd.CD_ERR_ARG, mi355cd.CD_ERR_ARG, True), (axis, flags)
        ins = np.full(70, 7, dtype=np.uint8)
        assert lib.cd_points_inside(cd._ctx, None, 70, 2, 0, ins.ctypes.data, None, None, None, None, None) == mi355cd.CD_ERR_ARG
        assert lib.cd_points_inside(cd._ctx, pts.ctypes.data, 70, 2, 0, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG
        assert lib.cd_signed_distance(cd._ctx, pts.ctypes.data, 70, 2, 0, None, None, None, None, None, None, ins.ctypes.data, None) == mi355cd.CD_ERR_ARG
        assert (ins == 7).all()
        rc, rc2, untouched = _raw(lib, cd._ctx, pts[:0], 2, 0)                                           # n = 0
        assert (rc, rc2) == (mi355cd.CD_OK, mi355cd.CD_OK)
        assert _raw(lib, cd._ctx, pts, 2, 0)[:2] == (mi355cd.CD_OK, mi355cd.CD_OK)


def test_moving_mesh_needs_a_tree_of_its_current_vertices():
    lib = mi355cd.load_library()
    v, f = _mesh("torus")
    moved = v * np.array([1.0, 1.0, 0.5]) + np.array([0.25, 0.0, 0.0])
    pts = cm.torus_points(700, seed=77, margin=0.0)[0]
    with _ctx(v, f) as cd:
        _same(cd.points_inside(pts, 2), ref.points_inside(pts, v, f, 2), "before the move")
        for verts, rebuild in ((moved, "build_tree"), (v, "self_collide")):
            cd.update_vertices(verts)
            assert _raw(lib, cd._ctx, pts, 2, 0) == (mi355cd.CD_ERR_ORDER, mi355cd.CD_ERR_ORDER, True)
            cd.build_tree() if rebuild == "build_tree" else cd.self_collide(cap=CAP)
            want = ref.points_inside(pts, verts, f, 2)
            _same(cd.points_inside(pts, 2), want, f"after {rebuild}")
            assert np.array_equal(cd.signed_distance(pts, 2)[6], want[0])
        assert 50 < want[0].sum() < 650


def test_leaves_the_context_as_it_was():
    import between_ref as br
    import oracle
    va, ia = br.soup(20000, 0.02, 21)
    pts = va[::50]
    with mi355cd.CollisionDetector(va, ia) as a:
        a.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)                             # what a captured step needs (graph_eligible)
        a.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
        a.set_option(mi355cd.CD_OPT_GRAPH, 1)
        ref_pairs = oracle.pipeline(a.verts, a.vidx)
        for _ in range(4):                                                       # capture, then replays
            a.self_collide(cap=CAP)
        assert a.stats().traverse_launches == 0, "the self step does not replay: nothing here would be tested"
        st0, sp0, tri0 = bytes(a.stats()), oracle.pair_set(a.sorted_pairs(cap=CAP)[0]).tobytes(), a.collision_triangles()[0]
        hint0, cp0 = a.debug_hint()[:2], a.closest_points(pts)[:7]
        captures = a.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES)
        r0 = a.points_inside(pts, 2)
        a.points_inside(va, 0, parity=True)                                      # (a larger call: the buffers grow)
        s0 = a.signed_distance(pts, 1)
        assert np.array_equal(_bits(np.abs(s0[0])), _bits(cp0[2])) and np.array_equal(s0[1], cp0[0])
        assert bytes(a.stats()) == st0
        assert oracle.pair_set(a.sorted_pairs(cap=CAP)[0]).tobytes() == sp0
        assert np.array_equal(a.collision_triangles()[0], tri0)
        assert a.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES) == captures
        assert all(np.array_equal(x, y) for x, y in zip(a.debug_hint()[:2], hint0))
        assert all(np.array_equal(x, y) for x, y in zip(a.closest_points(pts)[:7], cp0))
        rep0 = a.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)                     # the next self step still replays, and matches the oracle
        p, n, rc = a.self_collide(cap=CAP)
        assert a.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + 1 and a.stats().traverse_launches == 0
        assert a.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES) == captures
        assert rc == mi355cd.CD_OK and np.array_equal(oracle.pair_set(p), oracle.pair_set(ref_pairs["pairs"]))
        again = a.points_inside(pts, 2)
        assert all(np.array_equal(x, y) for x, y in zip(again[:5], r0[:5]))
