"""cd_nearest_self on the device against the CPU restatement (tests/nearest_self_ref.py: every admissible pair, no tree, no bound) and,
on meshes too large for that, against the device's own pinned cd_find_proximity_witness reduced per face on the host: faces, IDs, the
bits of dist, the witness's points, barycentrics, features and played faces, and n_found, for both flags."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import between_ref as br
import ccd_ref as cr
import mi355cd
import moving_inputs as mv
import nearest_ref as nr
import nearest_self_ref as ns
import oracle
import proximity_ref as pr
import query_meshes as qm
import scale_inputs as si
import witness_ref as wr

pytestmark = pytest.mark.gpu

CAP = 1 << 20
NONE = ns.NONE
INF = float("inf")


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _same(got, want, what):
    """A Nearest of the device (with its witness) against (NearestRows, played faces)."""
    rows, played = want
    w = got.witness
    bad = np.nonzero((got.faces != rows.faces).any(axis=1) | (got.ids != rows.ids).any(axis=1) | (_bits(got.dist) != _bits(rows.dist))
                     | (w.faces != played).any(axis=1) | (_bits(w.points) != _bits(rows.points)).any(axis=(1, 2))
                     | (_bits(w.bary) != _bits(rows.bary)).any(axis=(1, 2)) | (w.feature != rows.feature).any(axis=1))[0]
    k = bad[:4]
    assert bad.size == 0, (what, bad.size, k, got.faces[k], rows.faces[k], got.dist[k], rows.dist[k], w.faces[k], played[k], w.feature[k], rows.feature[k])
    assert got.info.n_found == int((rows.faces[:, 0] != NONE).sum()), (what, got.info.n_found)


def _check(cd, want, rmax, what):
    """Both flags at one radius; want: the restatement's rows at that radius.  -> the MIN row of the device."""
    _same(cd.nearest_self(rmax, witness=True), want, f"{what} rmax={rmax}")
    m = cd.nearest_self(rmax, minimum=True, witness=True)
    _same(m, ns.nearest_min(want), f"{what} rmax={rmax} MIN")
    return m


def _is_nothing(m):
    return (m.faces == NONE).all() and m.dist[0] == INF and not m.ids.any() and (m.witness.faces == NONE).all() and not m.witness.points.any() \
        and not m.witness.bary.any() and not m.witness.feature.any()


# ---------------------------------------------------------------- against the restatement
QM = {m[0]: m[1:] for m in qm._meshes() if m[0] in ("soup10k", "cloth100", "cloth100d", "comb", "duplicates", "custom_ids", "n1", "n2", "n3", "n63", "n64", "n65")}


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """name -> (verts, vidx, ids)"""
    if name in ("n1", "n2", "n3", "n63", "n64", "n65", "comb", "duplicates"):
        v, i, ids, _ = QM[name]
        return v, i, ids
    if name == "custom_ids2000":
        v, i, ids, _ = QM["custom_ids"]
        return v, i[:2000], ids[:2000]
    if name == "fan":
        return ns.fan(40) + (None,)
    if name == "fan_far":
        return ns.fan_and_far(40) + (None,)
    if name == "cloth16":
        import mi355_synth as synth
        return synth.cloth_pair(16) + (None,)
    if name == "soup700":
        return br.soup(700, 0.06, 5) + (None,)
    if name in ("doubled_nine", "doubled_mod3"):
        v, i = nr.doubled(*br.soup(150, 0.1, 42))
        n = i.shape[0]
        return v, i, np.full(n, 9, dtype=np.uint32) if name == "doubled_nine" else (np.arange(n) % 3).astype(np.uint32)
    raise KeyError(name)


SMALL = ("n1", "n2", "n3", "n63", "n64", "n65", "fan", "fan_far", "cloth16", "soup700", "duplicates", "custom_ids2000", "comb", "doubled_nine",
         "doubled_mod3")


@functools.lru_cache(maxsize=None)
def _rows_inf(name):
    v, i, ids = _mesh(name)
    return ns.nearest_rows(v, i, INF, ids)


@pytest.mark.parametrize("name", SMALL)
def test_against_restatement(name):
    """rmax = inf, 0, EXACTLY the clearance (found, closed), the next double below it (MIN finds nothing), the median row distance.
    (The rows of a smaller radius are nearest_self_ref.within of the rows at inf: tests/test_nearest_self_ref.py pins that.)"""
    v, i, ids = _mesh(name)
    want = _rows_inf(name)
    rows = want[0]
    nt = rows.dist.shape[0]
    found = rows.faces[:, 0] != NONE
    with _ctx(v, i, ids) as cd:
        g = cd.nearest_self(INF)
        assert g.witness is None and np.array_equal(g.faces, rows.faces)
        _check(cd, want, INF, name)
        _check(cd, ns.within(want, 0.0), 0.0, name)
        if name in ("fan", "n1"):                                               # no admissible pair: nothing is evaluated
            assert not found.any() and g.info.tri_tests == 0 and g.info.n_found == 0
            assert _is_nothing(cd.nearest_self(INF, minimum=True, witness=True))
            return
        assert found.all() or name == "duplicates"                              # (duplicates: face (5, 5, 5) and its like may have partners or not)
        sep = float(ns.nearest_min(want)[0].dist[0])
        m = _check(cd, ns.within(want, sep), sep, name)
        assert m.faces[0, 0] != NONE and m.dist[0] == sep                       # closed: the pair AT rmax is found
        if sep > 0.0:
            below = float(np.nextafter(sep, -INF))
            m = _check(cd, ns.within(want, below), below, name)
            assert _is_nothing(m)
        else:
            assert (m.witness.feature == wr.FEATURE_NONE).all() and not m.witness.points.any()
        med = float(np.median(rows.dist[found]))
        _check(cd, ns.within(want, med), med, name)
    if name == "cloth16":
        assert nt == 1024 and (rows.dist == 0.0).any() and (rows.dist > 0.0).any()
    if name == "custom_ids2000":
        assert (rows.ids[:, 0] == ids).all() and (rows.ids[:, 1] == ids[rows.faces[:, 1]]).all()
    if name == "fan_far":
        assert (rows.faces[:40, 1] == 40).all()


# ---------------------------------------------------------------- larger meshes, against the device's own pinned proximity query
def _reduced_proximity(cd, dist):
    cap = cd.find_proximity(dist, cap=1)[2]                                     # (the pair count: the witness arrays get exactly that room)
    p, d, n, rc, wit = cd.find_proximity_witness(dist, cap=max(cap, 1))
    assert rc == mi355cd.CD_OK and n == cap
    return ns.reduce_pairs(cd.nt, wit.faces[:n], p[:n], d[:n], wit.points[:n], wit.bary[:n], wit.feature[:n]), n


@pytest.mark.parametrize("edges", [2, INF])
@pytest.mark.parametrize("name", ["soup10k", "cloth100"])
def test_large_meshes_against_the_proximity_query(name, edges):
    """rmax = 2 edges and inf; for inf the proximity query gets the largest row distance times (1 + 2^-20).  MIN equals the minimum of
    the rows."""
    v, i, ids, edge = QM[name]
    rmax = edges * edge
    with _ctx(v, i, ids) as cd:
        nt = cd.nt
        got = cd.nearest_self(rmax, witness=True)
        dist = rmax
        if np.isinf(rmax):
            assert (got.faces[:, 0] == np.arange(nt)).all() and got.info.n_found == nt
            dist = float(got.dist.max()) * (1 + 2.0 ** -20)
        want, n = _reduced_proximity(cd, dist)
        print(f"{name} rmax={rmax}: {n} pairs within {dist / edge:.2f} edges, {got.info.node_visits / nt:.1f} boxes and "
              f"{got.info.tri_tests / nt:.2f} tri_distance a row")
        _same(got, want, f"{name} rmax={rmax}")
        m = cd.nearest_self(rmax, minimum=True, witness=True)
        _same(m, ns.nearest_min(want), f"{name} rmax={rmax} MIN")
        print(f"  MIN: {m.info.node_visits / nt:.1f} boxes and {m.info.tri_tests / nt:.2f} tri_distance a row")


def test_walk_does_not_degenerate_into_all_pairs():
    """A condition, not a measurement: with no radius, a walk with a wrong seed or a loose bound would test a large share of the mesh."""
    import mi355_synth as synth
    v, i = synth.cloth_pair(300)
    with _ctx(v, i) as cd:
        nt = cd.nt
        g = cd.nearest_self(INF)
    print(f"cloth300 rmax=inf: {g.info.tri_tests / nt:.2f} tri_distance and {g.info.node_visits / nt:.1f} boxes a row (nt / 100 = {nt / 100:.0f})")
    assert g.info.n_found == nt
    assert g.info.tri_tests / nt <= nt / 100


# ---------------------------------------------------------------- independence
def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def test_independent_of_frame_traversal_and_build():
    name = "soup700"
    v, i, ids = _mesh(name)
    want = _rows_inf(name)
    med = float(np.median(want[0].dist))
    want_med = ns.within(want, med)
    with mi355cd.CollisionDetector(v, i) as cd:
        for frame in (mi355cd.CD_FRAME_REFERENCE, mi355cd.CD_FRAME_AUTO, mi355cd.CD_FRAME_CUSTOM):
            for trav, stagewise in ((0, 0), (1, 0), (3, 0), (3, 1)):
                cd.set_option(mi355cd.CD_OPT_TRAVERSAL, trav)
                cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, stagewise)
                _frame(cd, frame)
                cd.self_collide(cap=CAP)                                        # the tree of this setting (the collision step builds it)
                what = f"frame {frame} traversal {trav} stagewise {stagewise}"
                _check(cd, want, INF, what)
                _check(cd, want_med, med, what)
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)
        cd.build_tree()                                                         # cd_build_tree's tree against cd_self_collide's
        _check(cd, want, INF, "build_tree")
        wmin = ns.nearest_min(want)
        for rep in range(3):                                                    # the shared bound: counters may differ, the row may not
            _same(cd.nearest_self(INF, minimum=True, witness=True), wmin, f"MIN repeat {rep}")


def test_independent_of_the_cell_table():
    """cloth100d (vertices that are not fp32 values): CD_OPT_CELL_TABLE 0 / 1 give the same rows, the proximity query's."""
    v, i, ids, edge = QM["cloth100d"]
    rmax = 2 * edge
    res = []
    with mi355cd.CollisionDetector(v, i) as cd:
        for table in (1, 0):
            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
            cd.self_collide(cap=CAP)
            res.append((cd.nearest_self(rmax, witness=True), cd.nearest_self(INF, minimum=True, witness=True)))
        want, _ = _reduced_proximity(cd, rmax)
    for g, m in res:
        _same(g, want, "cloth100d")
        _same(m, ns.nearest_min(want), "cloth100d MIN")


# ---------------------------------------------------------------- the fp32 range
SCALE_MESHES = si.meshes()


@functools.lru_cache(maxsize=None)
def _scale_rows(name, k=0):
    v, vidx, _ = SCALE_MESHES[name]
    return ns.nearest_rows(si.scaled(v, k), vidx, INF)


def _scaled_rows(want, k):
    rows, played = want
    return rows._replace(dist=np.ldexp(rows.dist, k), points=np.ldexp(rows.points, k)), played


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """tests/scale_inputs.py's meshes scaled by 2^k: the k = 0 rows with dist and points times 2^k, at rmax = inf and at a quarter of
    an edge; at si.EDGES the restatement itself on the scaled mesh."""
    v, vidx, edge = SCALE_MESHES[name]
    want = _scaled_rows(_scale_rows(name), k)
    if k in si.EDGES:
        own = _scale_rows(name, k)
        assert all(np.array_equal(x, y) for x, y in zip(own[0] + (own[1],), want[0] + (want[1],))), (name, k)   # the restatement is equivariant too
        want = own
    r = float(np.ldexp(edge / 4, k))
    with _ctx(si.scaled(v, k), vidx) as cd:
        _check(cd, want, INF, f"{name} k={k}")
        _check(cd, ns.within(want, r), r, f"{name} k={k}")


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_by_2_pow_20(name):
    v, vidx, edge = SCALE_MESHES[name]
    v = v + (2.0 ** 20 + 0.37)
    want = ns.nearest_rows(v, vidx, INF)
    with _ctx(v, vidx) as cd:
        _check(cd, want, INF, f"{name} translated")
        _check(cd, ns.within(want, edge / 4), edge / 4, f"{name} translated")


# ---------------------------------------------------------------- a mesh that moves
def test_moving_mesh_needs_a_tree_of_its_current_vertices():
    s = mv.seq("slide")
    lib = mi355cd.load_library()
    r = 2 * s.edge
    with mi355cd.CollisionDetector(s.frames[0], s.vidx) as cd:
        cd.build_tree()
        for f, rebuild in ((0, None), (1, "self_collide"), (0, "build_tree")):
            if rebuild:
                cd.update_vertices(s.frames[f])
                faces = np.full((cd.nt + 8, 2), 0xDEADBEEF, dtype=np.uint32)
                for flags in (0, mi355cd.CD_NEAREST_MIN):
                    assert lib.cd_nearest_self(cd._ctx, INF, flags, faces.ctypes.data, None, None, None, None) == mi355cd.CD_ERR_ORDER
                assert (faces == 0xDEADBEEF).all()
                cd.build_tree() if rebuild == "build_tree" else cd.self_collide(cap=CAP)
            want = wr.cached(("nearest_self", "slide", f), lambda: ns.nearest_rows(s.frames[f], s.vidx, INF))
            _check(cd, want, INF, f"slide frame {f}")
            _check(cd, ns.within(want, r), r, f"slide frame {f}")


# ---------------------------------------------------------------- the context's state
def _same_prox(got, want, what):
    gp, gd = pr.sort_pairs(got[0], got[1])
    wp, wd = want
    assert got[3] == mi355cd.CD_OK and np.array_equal(gp, wp) and np.array_equal(_bits(gd), _bits(wd)), what


def test_leaves_the_context_as_it_was():
    va, ia = br.soup(20000, 0.02, 21)
    vb, ib = br.soup(5000, 0.04, 22)
    x1 = br.motion(va, 0.005, 1)
    pts = va[::50]
    with mi355cd.CollisionDetector(va, ia) as a, _ctx(vb, ib) as b:
        a.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)                             # what a captured step needs (graph_eligible)
        a.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
        a.set_option(mi355cd.CD_OPT_GRAPH, 1)
        ref = oracle.pipeline(a.verts, a.vidx)
        for _ in range(4):                                                       # capture, then replays
            a.self_collide(cap=CAP)
        assert a.stats().traverse_launches == 0, "the self step does not replay: nothing here would be tested"
        before = (bytes(a.stats()), oracle.pair_set(a.sorted_pairs(cap=CAP)[0]).tobytes(), a.collision_triangles()[0], a.find_proximity(0.004, cap=CAP),
                  a.find_ccd(x1, 0.004, cap=CAP), a.debug_hint()[:2], a.closest_points(pts)[:7], a.nearest_between(b, INF, witness=True))
        captures = a.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES)
        r0 = a.nearest_self(INF, witness=True)
        a.nearest_self(0.004, minimum=True, witness=True)
        assert a.nearest_self(INF, minimum=True).faces[0, 0] != NONE
        st0, sp0, tri0, px0, cc0, hint0, cp0, nb0 = before
        assert bytes(a.stats()) == st0
        assert oracle.pair_set(a.sorted_pairs(cap=CAP)[0]).tobytes() == sp0
        assert np.array_equal(a.collision_triangles()[0], tri0)
        assert a.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES) == captures
        assert all(np.array_equal(x, y) for x, y in zip(a.debug_hint()[:2], hint0))
        _same_prox(a.find_proximity(0.004, cap=CAP), pr.sort_pairs(px0[0], px0[1]), "proximity after the nearest calls")      # (rows unordered)
        gp, gt, gd = cr.sort_pairs(*a.find_ccd(x1, 0.004, cap=CAP)[:3])
        wp, wt, wd = cr.sort_pairs(*cc0[:3])
        assert np.array_equal(gp, wp) and np.array_equal(_bits(gt), _bits(wt)) and np.array_equal(_bits(gd), _bits(wd))
        assert all(np.array_equal(x, y) for x, y in zip(a.closest_points(pts)[:7], cp0))
        nb1 = a.nearest_between(b, INF, witness=True)
        assert np.array_equal(nb1.faces, nb0.faces) and np.array_equal(_bits(nb1.dist), _bits(nb0.dist))
        assert np.array_equal(_bits(nb1.witness.points), _bits(nb0.witness.points))
        rep0 = a.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)                     # the next self step still replays, and matches the oracle
        p, n, rc = a.self_collide(cap=CAP)
        assert a.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + 1 and a.stats().traverse_launches == 0
        assert a.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES) == captures
        assert rc == mi355cd.CD_OK and np.array_equal(oracle.pair_set(p), oracle.pair_set(ref["pairs"]))
        again = a.nearest_self(INF, witness=True)                                # and the query itself gives the same rows after all that
        assert np.array_equal(again.faces, r0.faces) and np.array_equal(_bits(again.dist), _bits(r0.dist))
        assert np.array_equal(again.witness.faces, r0.witness.faces) and np.array_equal(_bits(again.witness.points), _bits(r0.witness.points))


# ---------------------------------------------------------------- errors, NULL outputs, canaries
def _raw(lib, ctx, rmax, flags, rows, want_ids=True, want_dist=True, members=(1, 1, 1, 1), info=None):
    """The C call on arrays with 8 canary rows behind `rows`.  -> (rc, arrays)."""
    n = rows + 8
    arr = dict(faces=np.full((n, 2), 0xDEADBEEF, dtype=np.uint32), ids=np.full((n, 2), 0xDEADBEEF, dtype=np.uint32), dist=np.full(n, -7.0),
               wfaces=np.full((n, 2), 0xDEADBEEF, dtype=np.uint32), points=np.full((n, 2, 3), -7.0), bary=np.full((n, 2, 2), -7.0),
               feature=np.full((n, 2), 0xEE, dtype=np.uint8))
    p = lambda x: x.ctypes.data                                                  # noqa: E731
    w = mi355cd.CdWitnessOut(*(p(arr[k]) if on else None for k, on in zip(("wfaces", "points", "bary", "feature"), members)))
    rc = lib.cd_nearest_self(ctx, rmax, flags, p(arr["faces"]), p(arr["ids"]) if want_ids else None, p(arr["dist"]) if want_dist else None,
                             C.byref(w) if any(members) else None, C.byref(info) if info is not None else None)
    return rc, arr


def _untouched(arr, first=0, skip=()):
    for k, x in arr.items():
        if k in skip:
            continue
        filler = 0xEE if x.dtype == np.uint8 else (0xDEADBEEF if x.dtype == np.uint32 else -7.0)
        assert (x[first:] == filler).all(), k


def test_errors():
    name = "soup700"
    v, i, ids = _mesh(name)
    nt = i.shape[0]
    lib = mi355cd.load_library()
    E, O = mi355cd.CD_ERR_ARG, mi355cd.CD_ERR_ORDER
    with _ctx(v, i) as cd:
        info = mi355cd.CdNearestInfo(5, 5, 5)
        for ctx, r, f in [(None, 1.0, 0), (cd._ctx, float("nan"), 0), (cd._ctx, -1e-300, 0), (cd._ctx, -INF, 0), (cd._ctx, float("nan"), 1),
                          (cd._ctx, 1.0, 2), (cd._ctx, 1.0, -1), (cd._ctx, 1.0, 3)]:
            rc, arr = _raw(lib, ctx, r, f, nt, info=info)
            assert rc == E, (r, f)
            _untouched(arr)
            assert (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)
        for f in (0, mi355cd.CD_NEAREST_MIN):
            assert lib.cd_nearest_self(cd._ctx, 1.0, f, None, None, None, None, None) == E             # NULL faces
        cd.update_vertices(cd.verts)                                            # update_vertices without a rebuild
        for f in (0, mi355cd.CD_NEAREST_MIN):
            rc, arr = _raw(lib, cd._ctx, 1.0, f, nt, info=info)
            assert rc == O
            _untouched(arr)
        assert (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)
        cd.build_tree()
        # canaries behind every output, for both flags; and every output but faces may be NULL
        want = _rows_inf(name)
        for flags, rows, (w, played) in ((0, nt, want), (mi355cd.CD_NEAREST_MIN, 1, ns.nearest_min(want))):
            rc, arr = _raw(lib, cd._ctx, INF, flags, rows, info=info)
            assert rc == mi355cd.CD_OK and info.n_found == rows and info.tri_tests >= rows
            _untouched(arr, first=rows)
            assert np.array_equal(arr["faces"][:rows], w.faces) and np.array_equal(arr["wfaces"][:rows], played) and np.array_equal(arr["ids"][:rows], w.ids)
            assert np.array_equal(_bits(arr["dist"][:rows]), _bits(w.dist)) and np.array_equal(_bits(arr["points"][:rows]), _bits(w.points))
            assert np.array_equal(_bits(arr["bary"][:rows]), _bits(w.bary)) and np.array_equal(arr["feature"][:rows], w.feature)
            rc, arr = _raw(lib, cd._ctx, INF, flags, rows, want_ids=False, want_dist=False, members=(0, 0, 0, 0))
            assert rc == mi355cd.CD_OK and np.array_equal(arr["faces"][:rows], w.faces)
            _untouched(arr, skip=("faces",))
            _untouched(arr, first=rows)
            rc, arr = _raw(lib, cd._ctx, INF, flags, rows, want_ids=False, members=(0, 1, 0, 1))
            assert rc == mi355cd.CD_OK and np.array_equal(_bits(arr["points"][:rows]), _bits(w.points)) and np.array_equal(arr["feature"][:rows], w.feature)
            _untouched(arr, skip=("faces", "dist", "points", "feature"))
            _untouched(arr, first=rows)
            rc, arr = _raw(lib, cd._ctx, INF, flags, rows, want_dist=False, members=(1, 0, 0, 0))           # the played faces alone
            assert rc == mi355cd.CD_OK and np.array_equal(arr["wfaces"][:rows], played) and np.array_equal(arr["ids"][:rows], w.ids)
            _untouched(arr, skip=("faces", "ids", "wfaces"))
            _untouched(arr, first=rows)
    with mi355cd.CollisionDetector(v, i) as cd:                                  # never built
        assert _raw(lib, cd._ctx, 1.0, 0, nt)[0] == O
        assert _raw(lib, cd._ctx, 1.0, mi355cd.CD_NEAREST_MIN, nt)[0] == O
