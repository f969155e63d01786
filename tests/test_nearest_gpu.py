"""cd_nearest_between on the device against the CPU restatement (tests/nearest_ref.py: every a x b pair, no tree, no bound) and, on
meshes too large for that, against the device's own pinned cd_find_proximity_between_witness reduced on the host: faces, IDs, the bits
of dist, and the witness's points, barycentrics and features, for both flags."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import between_ref as br
import ccd_ref as cr
import mi355_synth as synth
import mi355cd
import nearest_ref as nr
import oracle
import proximity_ref as pr
import query_meshes as qm
import scale_inputs as si

pytestmark = pytest.mark.gpu

CAP = 1 << 20
NONE = nr.NONE
INF = float("inf")


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _same(got, want, what):
    """A Nearest of the device (with its witness) against NearestRows."""
    w = got.witness
    bad = np.nonzero((got.faces != want.faces).any(axis=1) | (got.ids != want.ids).any(axis=1) | (_bits(got.dist) != _bits(want.dist))
                     | (w.faces != want.faces).any(axis=1) | (_bits(w.points) != _bits(want.points)).any(axis=(1, 2))
                     | (_bits(w.bary) != _bits(want.bary)).any(axis=(1, 2)) | (w.feature != want.feature).any(axis=1))[0]
    k = bad[:4]
    assert bad.size == 0, (what, bad.size, k, got.faces[k], want.faces[k], got.dist[k], want.dist[k], w.feature[k], want.feature[k])
    assert got.info.n_found == int((want.faces[:, 0] != NONE).sum()), (what, got.info.n_found)


def _check(a, b, rows, rmax, what):
    """Both flags at one radius; rows: the restatement's rows at that radius.  -> the MIN row of the device."""
    _same(a.nearest_between(b, rmax, witness=True), rows, f"{what} rmax={rmax}")
    m = a.nearest_between(b, rmax, minimum=True, witness=True)
    _same(m, nr.nearest_min(rows), f"{what} rmax={rmax} MIN")
    return m


# ---------------------------------------------------------------- the small between cases, against the restatement
CASES = nr.between_cases()


def _case(name, swap):
    va, ia, vb, ib = CASES[name]
    return (vb, ib, va, ia) if swap else (va, ia, vb, ib)


@functools.lru_cache(maxsize=None)
def _rows_inf(name, swap):
    return nr.nearest_rows(*_case(name, swap), INF)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_restatement(name, swap):
    """rmax = inf, 0, EXACTLY the separation distance (found), the next double below it (MIN finds nothing), the median row distance.
    (The rows of a smaller radius are nearest_ref.within of the rows at inf: tests/test_nearest_ref.py pins that to the definition.)"""
    assert {"soup_1_1_s1", "soup_1_400_s2", "soup_400_1_s3", "soup_2_600_s4", "soup_700_900_s5", "soup_1500_500_s6", "disjoint", "shared_positions",
            "degenerate"} == set(CASES)
    va, ia, vb, ib = _case(name, swap)
    rows = _rows_inf(name, swap)
    assert (rows.faces[:, 0] == np.arange(ia.shape[0])).all()                  # rmax = +inf: every row finds something
    sep = float(nr.nearest_min(rows).dist[0])
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        _check(a, b, rows, INF, name)
        _check(a, b, nr.within(rows, 0.0), 0.0, name)
        m = _check(a, b, nr.within(rows, sep), sep, name)
        assert m.faces[0, 0] != NONE and m.dist[0] == sep                      # closed: the pair AT rmax is found
        if sep > 0.0:
            below = float(np.nextafter(sep, -INF))
            m = _check(a, b, nr.within(rows, below), below, name)
            assert (m.faces == NONE).all() and m.dist[0] == INF and not m.ids.any() and not m.witness.points.any() and not m.witness.feature.any()
        med = float(np.median(rows.dist))
        _check(a, b, nr.within(rows, med), med, name)
        if ib.shape[0] == 1:                                                    # no records: one test a row, no box
            g = a.nearest_between(b, INF)
            assert g.info.tri_tests == ia.shape[0] and g.info.node_visits == 0 and g.witness is None
    assert name != "disjoint" or sep > 1.0                                      # (a case whose separation distance is not 0)


# ---------------------------------------------------------------- split meshes
MESHES = {m[0]: m[1:] for m in qm._meshes() if m[0] in ("soup10k", "comb", "duplicates", "custom_ids", "n1", "n2", "n3", "n63", "n64", "n65")}


def _both_radii(va, ia, vb, ib, ida, idb, what):
    rows = nr.nearest_rows(va, ia, vb, ib, INF, ida, idb)
    med = float(np.median(rows.dist))
    with _ctx(va, ia, ida) as a, _ctx(vb, ib, idb) as b:
        _check(a, b, rows, INF, what)
        _check(a, b, nr.within(rows, med), med, what)
    return rows


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("name", ["n1", "n2", "n3", "n63", "n64", "n65"])
def test_tiny_mesh_against_soup10k(name, swap):
    v, i, _, _ = MESHES[name]
    vb, ib, _, _ = MESHES["soup10k"]
    if swap:
        _both_radii(vb, ib, v, i, None, None, f"soup10k vs {name}")
    else:
        _both_radii(v, i, vb, ib, None, None, f"{name} vs soup10k")


@pytest.mark.parametrize("name,k", [("comb", 60), ("duplicates", 300), ("custom_ids", 200), ("custom_ids", 4800)])
def test_split_meshes_keep_their_ids(name, k):
    """comb: 60 levels deep on both sides.  duplicates: coincident and degenerate triangles.  custom_ids: IDs that are not face indices
    (200 | 4800 and 4800 | 200: a x b stays within the all-pairs restatement)."""
    v, i, ids, _ = MESHES[name]
    va, ia, vb, ib = br.split(v, i, k)
    ida, idb = (None, None) if ids is None else (ids[:k], ids[k:])
    rows = _both_radii(va, ia, vb, ib, ida, idb, f"{name} split at {k}")
    if ids is not None:
        assert (rows.ids[:, 0] == ids[:k]).all() and (rows.ids[:, 1] == ids[k:][rows.faces[:, 1]]).all()


def test_repeated_ids_in_both_meshes_the_face_index_decides():
    va, ia = br.soup(200, 0.1, 41)
    vb, ib = nr.doubled(*br.soup(150, 0.1, 42))
    va, ia = nr.doubled(va, ia)
    ida, idb = np.full(ia.shape[0], 9, dtype=np.uint32), (np.arange(ib.shape[0]) % 3).astype(np.uint32)
    rows = _both_radii(va, ia, vb, ib, ida, idb, "repeated ids")
    assert (rows.dist[:200] == rows.dist[200:]).all() and (rows.faces[:200, 1] == rows.faces[200:, 1]).all()
    m = nr.nearest_min(rows)
    assert m.faces[0, 0] < 200                                                  # of a's two copies at the minimum: the smaller face


# ---------------------------------------------------------------- invariance
def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def test_independent_of_frames_traversal_build_and_cell_table():
    name = "soup_1500_500_s6"
    va, ia, vb, ib = CASES[name]
    rows = _rows_inf(name, False)
    med = float(np.median(rows.dist))
    rows_med = nr.within(rows, med)
    frames = (mi355cd.CD_FRAME_REFERENCE, mi355cd.CD_FRAME_AUTO)
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:
        for fa in frames:
            for fb in frames:
                for trav, stagewise, table in ((0, 0, 1), (1, 0, 0), (3, 0, 1), (3, 1, 1), (3, 0, 0)):
                    for cd, f in ((a, fa), (b, fb)):
                        cd.set_option(mi355cd.CD_OPT_TRAVERSAL, trav)
                        cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
                        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, stagewise)
                        _frame(cd, f)
                        cd.self_collide(cap=CAP)                               # the tree of this setting (the collision step builds it)
                    what = f"frames {fa}/{fb} traversal {trav} stagewise {stagewise} table {table}"
                    _check(a, b, rows, INF, what)
                    _check(a, b, rows_med, med, what)
        for cd in (a, b):
            cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)
            cd.build_tree()                                                    # the staged build
        _check(a, b, rows, INF, "build_tree")
        want = nr.nearest_min(rows)
        for rep in range(3):                                                    # the shared bound: counters may differ, the row may not
            _same(a.nearest_between(b, INF, minimum=True, witness=True), want, f"MIN repeat {rep}")


# ---------------------------------------------------------------- the fp32 range
SCALE_MESHES = si.meshes()


def _halves(name):
    v, vidx, edge = SCALE_MESHES[name]
    k = vidx.shape[0] // 2
    return np.asarray(v, dtype=np.float64).reshape(-1, 3), vidx[:k], vidx[k:], edge      # (the vertex array stays whole on both sides)


@functools.lru_cache(maxsize=None)
def _scale_rows(name, k=0):
    vv, ia, ib, _ = _halves(name)
    v = si.scaled(vv, k)
    return nr.nearest_rows(v, ia, v, ib, INF)


def _scaled_rows(rows, k):
    return rows._replace(dist=np.ldexp(rows.dist, k), points=np.ldexp(rows.points, k))


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """tests/scale_inputs.py's meshes split in two and scaled by 2^k: the k = 0 rows with dist and points times 2^k, at rmax = inf and
    at a quarter of an edge; at si.EDGES the restatement itself on the scaled mesh."""
    vv, ia, ib, edge = _halves(name)
    rows = _scale_rows(name, k) if k in si.EDGES else _scaled_rows(_scale_rows(name), k)
    if k in si.EDGES:
        _same_rows = _scaled_rows(_scale_rows(name), k)
        assert all(np.array_equal(x, y) for x, y in zip(rows, _same_rows)), (name, k)      # the restatement is equivariant too
    v = si.scaled(vv, k)
    r = float(np.ldexp(edge / 4, k))
    with _ctx(v, ia) as a, _ctx(v, ib) as b:
        _check(a, b, rows, INF, f"{name} k={k}")
        _check(a, b, nr.within(rows, r), r, f"{name} k={k}")


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_by_2_pow_20(name):
    vv, ia, ib, edge = _halves(name)
    v = vv + (2.0 ** 20 + 0.37)
    rows = nr.nearest_rows(v, ia, v, ib, INF)
    with _ctx(v, ia) as a, _ctx(v, ib) as b:
        _check(a, b, rows, INF, f"{name} translated")
        _check(a, b, nr.within(rows, edge / 4), edge / 4, f"{name} translated")


# ---------------------------------------------------------------- larger meshes, against the device's own pinned proximity query
def _sheets(quads):
    verts, vidx = synth.cloth_pair(quads)
    na, half = vidx.shape[0] // 2, verts.shape[0] // 2
    assert vidx[:na].max() < half and vidx[na:].min() >= half
    return verts[:half], vidx[:na], verts[half:], (vidx[na:] - half).astype(np.uint32)


def _reduce_pairs(na, pairs, dists, wit):
    """The rows of cd_find_proximity_between_witness (IDs are face indices) reduced per face of a by (dist, face of b)."""
    out = nr.nothing(na)
    first = nr._first_per_face(pairs[:, 0], dists, pairs[:, 1], pairs[:, 1])
    i = pairs[first, 0].astype(np.int64)
    assert np.array_equal(wit.faces, pairs)
    for dst, src in zip(out, (pairs, pairs, dists, wit.points, wit.bary, wit.feature)):
        dst[i] = src[first]
    return out


@pytest.mark.parametrize("edges", [2, INF])
@pytest.mark.parametrize("quads", [100, 300])
def test_cloth_sheets_against_the_proximity_query(quads, edges):
    """rmax = 2 quad edges and inf; for inf the proximity query gets a dist above the sheets' largest clearance, taken from the first
    call.  MIN equals the minimum of the rows."""
    va, ia, vb, ib = _sheets(quads)
    na = ia.shape[0]
    edge = 2.88 / quads
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        for rmax in (edges * edge,):
            got = a.nearest_between(b, rmax, witness=True)
            dist = rmax
            if np.isinf(rmax):
                assert (got.faces[:, 0] == np.arange(na)).all() and got.info.n_found == na
                dist = float(got.dist.max()) * (1 + 2.0 ** -20)
            cap = a.find_proximity_between(b, dist, cap=1)[2]                     # (the pair count: the witness arrays get exactly that room)
            p, d, n, rc, wit = a.find_proximity_between_witness(b, dist, cap=cap)
            assert rc == mi355cd.CD_OK and n == cap
            want = _reduce_pairs(na, p, d, wit)
            print(f"cloth{quads} rmax={rmax}: {n} pairs within {dist / edge:.2f} edges, {got.info.node_visits / na:.1f} boxes and "
                  f"{got.info.tri_tests / na:.2f} tri_distance a row")
            del p, d, wit
            _same(got, want, f"cloth{quads} rmax={rmax}")
            m = a.nearest_between(b, rmax, minimum=True, witness=True)
            _same(m, nr.nearest_min(want), f"cloth{quads} rmax={rmax} MIN")
            print(f"  MIN: {m.info.node_visits / na:.1f} boxes and {m.info.tri_tests / na:.2f} tri_distance a row")


def test_walk_does_not_degenerate_into_all_pairs():
    """A cap, as the closest-point query's: with no radius a walk without a seed or with a loose bound would test a large share of b."""
    va, ia, vb, ib = _sheets(300)
    na, nb = ia.shape[0], ib.shape[0]
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        g = a.nearest_between(b, INF)
    print(f"cloth300 rmax=inf: {g.info.tri_tests / na:.2f} tri_distance and {g.info.node_visits / na:.1f} boxes a row (nb / 1000 = {nb / 1000:.0f})")
    assert g.info.tri_tests / na <= nb / 100


# ---------------------------------------------------------------- the contexts' state
def _same_prox(got, want, what):
    gp, gd = pr.sort_pairs(got[0], got[1])
    wp, wd = want
    assert got[3] == mi355cd.CD_OK and np.array_equal(gp, wp) and np.array_equal(_bits(gd), _bits(wd)), what


def test_leaves_both_contexts_as_they_were():
    va, ia = br.soup(20000, 0.02, 21)
    vb, ib = br.soup(20000, 0.02, 22)
    x1a, x1b = br.motion(va, 0.005, 1), br.motion(vb, 0.005, 2)
    pts = va[::50]
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:
        for cd in (a, b):                                    # what a captured step needs (graph_eligible)
            cd.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)
            cd.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
            cd.set_option(mi355cd.CD_OPT_GRAPH, 1)
        refs = {id(cd): oracle.pipeline(cd.verts, cd.vidx) for cd in (a, b)}
        for _ in range(3):                                   # capture, then replays
            for cd in (a, b):
                cd.self_collide(cap=CAP)
        before = {}
        for cd in (a, b):
            p, n, rc = cd.self_collide(cap=CAP)
            assert cd.stats().traverse_launches == 0, "the self step does not replay: nothing here would be tested"
            before[id(cd)] = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(), cd.collision_triangles()[0],
                              cd.find_proximity(0.004, cap=CAP), cd.find_ccd(x1a if cd is a else x1b, 0.004, cap=CAP), cd.debug_hint()[:2],
                              cd.closest_points(pts)[:7], a.find_proximity_between(b, 0.004, cap=CAP) if cd is a else None)
        r0 = a.nearest_between(b, INF, witness=True)
        a.nearest_between(b, 0.004, minimum=True, witness=True)
        r1 = b.nearest_between(a, INF, minimum=True)
        assert r1.faces[0, 0] != NONE
        for cd in (a, b):
            st0, sp0, tri0, px0, cc0, hint0, cp0, bw0 = before[id(cd)]
            assert bytes(cd.stats()) == st0
            assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == sp0
            assert np.array_equal(cd.collision_triangles()[0], tri0)
            assert all(np.array_equal(x, y) for x, y in zip(cd.debug_hint()[:2], hint0))
            _same_prox(cd.find_proximity(0.004, cap=CAP), pr.sort_pairs(px0[0], px0[1]), "proximity after the nearest calls")   # (rows unordered)
            gp, gt, gd = cr.sort_pairs(*cd.find_ccd(x1a if cd is a else x1b, 0.004, cap=CAP)[:3])
            wp, wt, wd = cr.sort_pairs(*cc0[:3])
            assert np.array_equal(gp, wp) and np.array_equal(_bits(gt), _bits(wt)) and np.array_equal(_bits(gd), _bits(wd))
            assert all(np.array_equal(x, y) for x, y in zip(cd.closest_points(pts)[:7], cp0))
            if bw0 is not None:
                _same_prox(a.find_proximity_between(b, 0.004, cap=CAP), pr.sort_pairs(bw0[0], bw0[1]), "between after the nearest calls")
        for cd in (a, b):                                    # the next self step still replays, and matches the oracle
            rep0 = cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
            p, n, rc = cd.self_collide(cap=CAP)
            assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + 1 and cd.stats().traverse_launches == 0
            r = refs[id(cd)]
            assert rc == mi355cd.CD_OK and np.array_equal(oracle.pair_set(p), oracle.pair_set(r["pairs"]))
        again = a.nearest_between(b, INF, witness=True)      # and the query itself gives the same rows after all that
        assert np.array_equal(again.faces, r0.faces) and np.array_equal(_bits(again.dist), _bits(r0.dist))
        assert np.array_equal(_bits(again.witness.points), _bits(r0.witness.points))


# ---------------------------------------------------------------- errors, NULL outputs, canaries
def _raw(lib, a, b, rmax, flags, rows, want_ids=True, want_dist=True, members=(1, 1, 1, 1), info=None):
    """The C call on arrays with 8 canary rows behind `rows`.  -> (rc, arrays)."""
    n = rows + 8
    arr = dict(faces=np.full((n, 2), 0xDEADBEEF, dtype=np.uint32), ids=np.full((n, 2), 0xDEADBEEF, dtype=np.uint32), dist=np.full(n, -7.0),
               wfaces=np.full((n, 2), 0xDEADBEEF, dtype=np.uint32), points=np.full((n, 2, 3), -7.0), bary=np.full((n, 2, 2), -7.0),
               feature=np.full((n, 2), 0xEE, dtype=np.uint8))
    p = lambda x: x.ctypes.data                                                  # noqa: E731
    w = mi355cd.CdWitnessOut(*(p(arr[k]) if on else None for k, on in zip(("wfaces", "points", "bary", "feature"), members)))
    rc = lib.cd_nearest_between(a, b, rmax, flags, p(arr["faces"]), p(arr["ids"]) if want_ids else None, p(arr["dist"]) if want_dist else None,
                                C.byref(w) if any(members) else None, C.byref(info) if info is not None else None)
    return rc, arr


def _untouched(arr, first=0, skip=()):
    for k, x in arr.items():
        if k in skip:
            continue
        filler = 0xEE if x.dtype == np.uint8 else (0xDEADBEEF if x.dtype == np.uint32 else -7.0)
        assert (x[first:] == filler).all(), k


def test_errors():
    va, ia, vb, ib = CASES["soup_700_900_s5"]
    na = ia.shape[0]
    lib = mi355cd.load_library()
    E, O = mi355cd.CD_ERR_ARG, mi355cd.CD_ERR_ORDER
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        info = mi355cd.CdNearestInfo(5, 5, 5)
        bad = [(a._ctx, a._ctx, 1.0, 0), (None, b._ctx, 1.0, 0), (a._ctx, None, 1.0, 0), (a._ctx, b._ctx, float("nan"), 0), (a._ctx, b._ctx, -1e-300, 0),
               (a._ctx, b._ctx, -INF, 0), (a._ctx, b._ctx, 1.0, 2), (a._ctx, b._ctx, 1.0, -1), (a._ctx, b._ctx, 1.0, 3)]
        for x, y, r, f in bad:
            rc, arr = _raw(lib, x, y, r, f, na, info=info)
            assert rc == E, (r, f)
            _untouched(arr)
            assert (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)
        for f in (0, mi355cd.CD_NEAREST_MIN):
            assert lib.cd_nearest_between(a._ctx, b._ctx, 1.0, f, None, None, None, None, None) == E            # NULL faces
        for cd in (a, b):                                                       # update_vertices without a rebuild, on either side
            cd.update_vertices(cd.verts)
            for x, y in ((a, b), (b, a)):
                rc, arr = _raw(lib, x._ctx, y._ctx, 1.0, 0, max(na, ib.shape[0]), info=info)
                assert rc == O
                _untouched(arr)
            cd.build_tree()
        # canaries behind every output, for both flags; and every output but faces may be NULL
        want = nr.nearest_rows(va, ia, vb, ib, INF)
        for flags, rows, w in ((0, na, want), (mi355cd.CD_NEAREST_MIN, 1, nr.nearest_min(want))):
            rc, arr = _raw(lib, a._ctx, b._ctx, INF, flags, rows, info=info)
            assert rc == mi355cd.CD_OK and info.n_found == rows and info.tri_tests >= rows
            _untouched(arr, first=rows)
            assert np.array_equal(arr["faces"][:rows], w.faces) and np.array_equal(arr["wfaces"][:rows], w.faces) and np.array_equal(arr["ids"][:rows], w.ids)
            assert np.array_equal(_bits(arr["dist"][:rows]), _bits(w.dist)) and np.array_equal(_bits(arr["points"][:rows]), _bits(w.points))
            assert np.array_equal(_bits(arr["bary"][:rows]), _bits(w.bary)) and np.array_equal(arr["feature"][:rows], w.feature)
            rc, arr = _raw(lib, a._ctx, b._ctx, INF, flags, rows, want_ids=False, want_dist=False, members=(0, 0, 0, 0))
            assert rc == mi355cd.CD_OK and np.array_equal(arr["faces"][:rows], w.faces)
            _untouched(arr, skip=("faces",))
            _untouched(arr, first=rows)
            rc, arr = _raw(lib, a._ctx, b._ctx, INF, flags, rows, want_ids=False, members=(0, 1, 0, 1))
            assert rc == mi355cd.CD_OK and np.array_equal(_bits(arr["points"][:rows]), _bits(w.points)) and np.array_equal(arr["feature"][:rows], w.feature)
            _untouched(arr, skip=("faces", "dist", "points", "feature"))
            _untouched(arr, first=rows)
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:      # never built
        assert _raw(lib, a._ctx, b._ctx, 1.0, 0, na)[0] == O
        a.build_tree()
        assert _raw(lib, a._ctx, b._ctx, 1.0, 0, na)[0] == O
        assert _raw(lib, b._ctx, a._ctx, 1.0, 0, na)[0] == O
