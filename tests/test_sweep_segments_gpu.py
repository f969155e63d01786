"""The swept-segment queries on the device (cd_seg_advance_points, cd_sweep_segments_all, cd_sweep_segments) against the restatement of
tests/swept_segment_ref.py -- which uses no tree and no box filter beyond the gate -- as sets of (item, face) and bit for bit in every
value of a row, and against the device's own swept-point, segment and ray queries where the contract says they are the same thing.
Every step has bounded size; every reference is computed once and shared."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import mi355_synth as synth
import mi355cd
import moving_inputs as mi
import oracle
import scale_inputs as si
import segment_ref as sref
import sweep_ref as swr
import swept_segment_ref as ssr
import within_ref as wr

pytestmark = pytest.mark.gpu

CAP = 1 << 20
NAMES = ssr.SMALL + ["cloth100"]
OK, OVERFLOW = mi355cd.CD_OK, mi355cd.CD_OVERFLOW
NONE = mi355cd.SWEEP_NONE


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _ends(it):
    return it[:, 0:3], it[:, 3:6], it[:, 6:9], it[:, 9:12], it[:, 12]


def _sweep(cd, it, x1, what, skip=None, cap=CAP):
    """sweep_segments_all's rows as a SweepSegRows sorted by (item, face); the call fitted its capacity."""
    got = cd.sweep_segments_all(*_ends(it), verts_end=x1, skip_vertices=skip, cap=cap)
    assert got[13] == OK and got[12] == got[0].shape[0], (what, got[12:])
    info = cd.sweep_segments_info
    assert info.n_candidates >= info.n_tested >= got[12] and info.n_evals >= info.n_tested, what
    return ssr.SweepSegRows(*wr.sort_rows(*got[:12]))


def _first(cd, it, x1, skip=None):
    got = cd.sweep_segments(*_ends(it), verts_end=x1, skip_vertices=skip)
    assert got[12].n_found == int((got[0] != NONE).sum())
    return got


def _same_tuple(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        if b.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        assert np.array_equal(a, b), (what, k)


def _counts(cd):
    return (cd.sweep_segments_info.n_tested, cd.sweep_segments_info.n_evals, cd.sweep_segments_info.n_unresolved)


def _sub(w, m):
    return type(w)(*(a[w.rows[:, 0] < m] for a in w))


# ---------------------------------------------------------------- 1: the pin
@functools.lru_cache(maxsize=None)
def _pin():
    it, t = ssr.pin_all(1200, seed=1)                                          # 17 classes of 1200 and 2 of 150, mixed: every wave meets every branch
    o = np.random.default_rng(2).permutation(it.shape[0])
    it, t = np.ascontiguousarray(it[o]), np.ascontiguousarray(t[o])
    return it, t, ssr.seg_advance_np(it, t)


def test_seg_advance_is_the_restatement_bit_for_bit():
    it, t, want = _pin()
    ssr.pin_conditions(it, t, want)
    _same_tuple(mi355cd.seg_advance_points(it, t), want[:11], "pin")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_seg_advance_grid_edge(n):
    it, t, want = _pin()
    _same_tuple(mi355cd.seg_advance_points(it[:n], t[:n]), tuple(a[:n] for a in want[:11]), f"pin, n = {n}")


# ---------------------------------------------------------------- 2: the row sets
@pytest.mark.parametrize("name", NAMES)
def test_row_sets_are_the_restatement(name):
    v, i, ids, edge = ssr.MESHES[name]
    it, x1 = ssr.items(name), ssr.mesh_end(name)
    want, counts = ssr.want(name)
    n = it.shape[0]
    per = np.bincount(want.rows[:, 0].astype(np.int64), minlength=n)
    print(f"{name}: {want.rows.shape[0]} rows, {int((per == 0).sum())} of {n} items with none, {int((per >= 2).sum())} with several, counts {counts}")
    assert counts[2] == 0 and (per == 0).sum() >= n // 8 and (want.cross == 1).any() and (want.cross == 0).any() and ((want.toi > 0) & (want.toi < 1)).sum() >= 10
    if i.shape[0] >= 500:
        assert (per >= 2).sum() >= n // 8 and ((want.toi > 0) & (want.toi < 1)).sum() >= 100 and (want.toi == 1.0).any()
    with _ctx(v, i, ids) as cd:
        wr.same_rows(_sweep(cd, it, x1, name), want, name)
        assert _counts(cd) == counts, (name, _counts(cd), counts)
        assert i.shape[0] > 1 or cd.sweep_segments_info.n_candidates == n       # one triangle: no records, every item meets leaf 0
        for m in (1, 63, 64, 65):                                               # the grid edge of the descent
            sub, sub_counts = ssr.sweep_segment_rows_ref(v, x1, i, ids, it[:m], counts=True)
            _same_tuple(sub, _sub(want, m), f"{name}, {m} items: the restatement's own prefix")
            wr.same_rows(_sweep(cd, it[:m], x1, f"{name}, {m} items"), sub, f"{name}, {m} items")
            assert _counts(cd) == sub_counts, (name, m)


def test_unresolved_rows_are_the_restatements():
    """Constructed: segments whose near end runs along a face at 1.5 dist for some 2000 dist are left unresolved after 1024 evaluations."""
    it, t = ssr.pin_class("pt_unresolved", 8, np.random.default_rng(4))
    v = np.ascontiguousarray(t[:, :3].reshape(-1, 3))
    i = np.arange(24, dtype=np.uint32).reshape(8, 3)
    want, counts = ssr.sweep_segment_rows_ref(v, None, i, None, it, counts=True)
    own = want.rows[:, 0] == want.rows[:, 1]
    assert counts[2] >= 8 and own.sum() == 8 and np.all(want.dist[own] > it[:, 12])
    with _ctx(v, i) as cd:
        wr.same_rows(_sweep(cd, it, None, "unresolved"), want, "unresolved")
        assert _counts(cd) == counts
        _same_tuple(_first(cd, it, None)[:12], ssr.first_of(want, 8), "unresolved, first contact")


# ---------------------------------------------------------------- 3: first contact
@pytest.mark.parametrize("name", NAMES)
def test_first_contact_is_the_smallest_row_of_the_devices_own_rows(name):
    v, i, ids, edge = ssr.MESHES[name]
    it, x1 = ssr.items(name), ssr.mesh_end(name)
    n = it.shape[0]
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, x1, name)
        evals = cd.sweep_segments_info.n_evals
        got = _first(cd, it, x1)
        _same_tuple(got[:12], ssr.first_of(rows, n), name)
        assert np.array_equal(np.bincount(rows.rows[:, 0].astype(np.int64), minlength=n) == 0, got[0] == NONE)
        assert got[12].tri_tests <= evals                                       # the cut-off only saves evaluations
        for m in (1, 63, 64, 65):
            _same_tuple(_first(cd, it[:m], x1)[:12], tuple(a[:m] for a in got[:12]), f"{name}, {m} items")


def _grid(n):
    """An integer-grid sheet of n x n quads in z = 0, two triangles a quad."""
    x, y = np.meshgrid(np.arange(n + 1.0), np.arange(n + 1.0), indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1)
    k = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    f = np.concatenate([np.stack([k, k + n + 1, k + n + 2], axis=1), np.stack([k, k + n + 2, k + 1], axis=1)])
    return v, f.astype(np.uint32)


def test_ties_at_equal_toi_go_to_the_smaller_id_then_face_index():
    """Segments a quarter above an integer grid, from a vertex to a neighbour or to the quad's centre, dist a half: every face they pass
    over reports at toi = 0; IDs that repeat leave the face index to decide."""
    v, f = _grid(9)
    g = np.random.default_rng(6)
    ids = g.integers(0, 6, f.shape[0]).astype(np.uint32)                      # (few IDs: many ties go on to the face index)
    up = np.array([0.0, 0.0, 0.25])
    inner = v[(v[:, 0] < 9) & (v[:, 1] < 9)]
    a0 = np.concatenate([inner, inner]) + up
    b0 = np.concatenate([inner + np.array([1.0, 0.0, 0.0]), inner + np.array([0.5, 0.5, 0.0])]) + up
    it = ssr.pack(a0, b0, a0 - 2 * up, b0 - 2 * up, 0.5)
    n = it.shape[0]
    with _ctx(v, f, ids) as cd:
        rows = _sweep(cd, it, None, "grid")
        got = _first(cd, it, None)
    assert np.all(rows.toi == 0.0) and np.all(got[2] == 0.0) and np.all(got[0] != NONE)
    face, bid = got[0].astype(np.int64), got[1]
    by_id = by_face = 0
    for k in range(n):
        at = np.nonzero(rows.rows[:, 0] == k)[0]
        key = min((int(rows.ids[r]), int(rows.rows[r, 1])) for r in at)
        assert (int(bid[k]), int(face[k])) == key, k
        by_id += len({int(rows.ids[r]) for r in at}) > 1
        by_face += sum(int(rows.ids[r]) == key[0] for r in at) > 1
    assert by_id > 50 and by_face > 30, (by_id, by_face)
    _same_tuple(got[:12], ssr.first_of(rows, n), "grid")


# ---------------------------------------------------------------- 4: consistency with the swept-point and the static queries
@pytest.mark.parametrize("name", ["soup10k", "cloth100", "n1", "n65"])
def test_point_items_are_the_swept_point_queries(name):
    """a0 == b0 and a1 == b1: cd_sweep_points_all's rows and cd_sweep_points' answers bit for bit (toi, dist, u, v, feature, side, qt)."""
    v, i, ids, edge = ssr.MESHES[name]
    x1 = ssr.mesh_end(name)
    p0 = wr.points(name)
    p1 = p0 + np.random.default_rng(11).normal(size=p0.shape) * 0.6 * edge
    it = ssr.pack(p0, p0, p1, p1, 0.25 * edge)
    n = it.shape[0]
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, x1, name)
        seg_counts = _counts(cd)
        first = _first(cd, it, x1)
        pts = cd.sweep_points_all(p0, p1, 0.25 * edge, verts_end=x1, cap=CAP)
        pt_counts = (cd.sweep_info.n_tested, cd.sweep_info.n_evals, cd.sweep_info.n_unresolved)
        pfirst = cd.sweep_points(p0, p1, 0.25 * edge, verts_end=x1)
    assert pts[9] == OK and pts[8] > (20 if i.shape[0] > 1 else 0) and seg_counts == pt_counts
    want = swr.SweepRows(*wr.sort_rows(*pts[:8]))
    wr.same_rows((rows.rows, rows.ids, rows.toi, rows.dist, rows.on_tri, rows.uv, rows.feature, rows.side), want, name)
    assert np.all(rows.s == 0.0) and np.all(rows.end == 1) and not rows.cross.any()
    at = rows.rows[:, 0].astype(np.int64)
    moved = (it[at, 0:3] + rows.toi[:, None] * (it[at, 6:9] - it[at, 0:3]))
    inner = (rows.toi > 0) & (rows.toi < 1)
    assert np.array_equal(_bits(rows.on_seg[inner]), _bits(moved[inner])) and np.array_equal(_bits(rows.on_seg[rows.toi == 0]), _bits(it[at[rows.toi == 0], 0:3]))
    _same_tuple((first[0], first[1], first[2], first[3], first[6], first[7], first[8], first[11]), pfirst[:8], name + ", first contact")


@pytest.mark.parametrize("name", ["soup10k", "cloth100", "n1", "n65"])
def test_no_motion_is_segments_within(name):
    v, i, ids, edge = ssr.MESHES[name]
    s = sref.segments(name)
    it = ssr.pack(s[:, 0:3], s[:, 3:6], s[:, 0:3], s[:, 3:6], edge)
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, None, name)
        assert cd.sweep_segments_info.n_evals == cd.sweep_segments_info.n_tested and cd.sweep_segments_info.n_unresolved == 0   # one evaluation a pair
        sw = cd.segments_within(s[:, 0:3], s[:, 3:6], edge, cap=CAP)
    assert sw[12] == OK and np.all(rows.toi == 0.0)
    static = sref.SegRows(*wr.sort_rows(*sw[:11]))
    mine = (rows.rows, rows.ids, *rows[3:])
    wr.same_rows(mine, static, name)
    wr.same_rows(mine, sref.want(name, 1.0), name + ", restated")


@pytest.mark.parametrize("name", ["soup10k", "cloth100"])
def test_rows_at_toi_zero_are_segments_within_on_x0(name):
    v, i, ids, edge = ssr.MESHES[name]
    it, x1 = ssr.items(name), ssr.mesh_end(name)
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, x1, name)
        sw = cd.segments_within(it[:, 0:3], it[:, 3:6], it[:, 12], cap=CAP)
    z = rows.toi == 0.0
    assert z.sum() > 20 and (~z).sum() > 20
    wr.same_rows(tuple(a[z] for a in (rows.rows, rows.ids, *rows[3:])), sref.SegRows(*wr.sort_rows(*sw[:11])), name)


@pytest.mark.parametrize("name", ["soup10k", "cloth100"])
def test_every_ray_hit_of_the_start_segment_is_a_crossing_row_at_toi_zero(name):
    v, i, ids, edge = ssr.MESHES[name]
    it, x1 = ssr.items(name), ssr.mesh_end(name)
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, x1, name)
        d = it[:, 3:6] - it[:, 0:3]
        ray = np.nonzero((d != 0.0).any(axis=1))[0]                             # (a ray needs a direction: the moving points among the items have no crossing)
        hits = cd.cast_rays_all(it[ray, 0:3], d[ray], 1.0, cap=CAP)
    assert hits[6] == OK and hits[5] > 30 and ray.size < it.shape[0], hits[5:]
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(32)) | r[:, 1].astype(np.uint64)
    hr = hits[0].copy(); hr[:, 0] = ray[hr[:, 0]]
    h = wr.sort_rows(hr, *hits[1:5])
    kr, kh = key(rows.rows), key(h[0])
    at = np.minimum(np.searchsorted(kr, kh), kr.size - 1)
    assert np.array_equal(kr[at], kh), "a crossing without a row"
    assert np.all(rows.toi[at] == 0.0) and np.all(rows.cross[at] == 1) and np.all(rows.dist[at] == 0.0)
    assert np.array_equal(_bits(rows.s[at]), _bits(h[2])) and np.array_equal(_bits(rows.uv[at]), _bits(h[3]))       # ray_tri's own t, u, v
    assert ((rows.cross == 1) & (rows.toi == 0.0)).sum() == kh.size             # and no other crossing at the start
    print(f"{name}: {hits[5]} crossings, {rows.rows.shape[0]} rows")


def test_edge_on_pass_through_a_thin_sheet_is_reported_where_the_substitutes_see_nothing():
    """The test that motivates the call.  Long segments parallel to a sheet pass through it inside the step, every end far outside it.
    cd_segments_within at both ends of the step returns nothing; cd_sweep_points_all on the two ends and the midpoint, at three times
    the distance, returns nothing; cd_sweep_segments_all reports the edge-edge contact with 0 < toi < 1 and an edge feature."""
    v, f = _grid(8)
    g = np.random.default_rng(3)
    n = 200
    # the chord from P = (px, 0) to Q = (0, py) cuts the sheet's corner at the origin; the segment runs on from half a chord before P to
    # three chords beyond Q, so that both ends and the midpoint lie beside the sheet, more than half a quad away from it
    px, py = g.uniform(1.0, 3.0, n), g.uniform(1.0, 3.0, n)
    P, Q = np.stack([px, 0 * px, 1 + 0 * px], axis=1), np.stack([0 * py, py, 1 + 0 * py], axis=1)
    a0, b0 = P - 0.5 * (Q - P), Q + 3.0 * (Q - P)
    down = np.array([0.0, 0.0, -2.0])
    dist = 0.01
    it = ssr.pack(a0, b0, a0 + down, b0 + down, dist)
    mid = 0.5 * (a0 + b0)
    assert np.all(a0[:, 1] <= -0.5) and np.all(b0[:, 0] <= -3.0) and np.all(mid[:, 0] <= -0.75)
    with _ctx(v, f) as cd:
        for z in (0.0, 1.0):
            assert cd.segments_within(a0 + z * down, b0 + z * down, dist, cap=CAP)[11] == 0     # nothing at either end of the step
        for p in (a0, b0, mid):
            assert cd.sweep_points_all(p, p + down, 3 * dist, cap=CAP)[8] == 0                   # nothing for any sample point
        rows = _sweep(cd, it, None, "sheet")
        got = _first(cd, it, None)
    assert np.all((rows.toi > 0.0) & (rows.toi < 1.0)) and np.all(rows.dist <= dist) and np.all(rows.cross == 0)
    assert np.all(rows.end == 0) and np.all((rows.feature >= 1) & (rows.feature <= 6))          # the segment's inside against edges (and, beside the chord, vertices)
    assert np.array_equal(np.unique(rows.rows[rows.feature <= 3, 0]), np.arange(n))             # every item: an edge-edge contact
    assert np.all((got[2] >= 0.495 - 1e-12) & (got[2] <= 0.4975 + 1e-12))      # z = 1 - 2 t: within dist from t = 0.495 on, within h from 0.4975 on
    assert np.all((got[8] >= 1) & (got[8] <= 6)) and np.all(got[9] == 0) and np.all(got[10] == 0)


# ---------------------------------------------------------------- 5: skip_vertices
def test_skip_vertices_on_a_cloths_own_edges():
    v, f = synth.cloth_pair(24)
    v = np.asarray(v, dtype=np.float64)
    f = np.asarray(f)
    edge = 2.88 / 24
    x1 = v + np.random.default_rng(8).normal(size=v.shape) * 0.2 * edge
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), axis=1), axis=0)
    e = np.ascontiguousarray(e[::3].astype(np.uint32))                          # every third edge: 1000 and some, a ragged count
    ne = e.shape[0]
    it = ssr.pack(v[e[:, 0]], v[e[:, 1]], x1[e[:, 0]], x1[e[:, 1]], 0.2 * edge)
    want, counts = ssr.sweep_segment_rows_ref(v, x1, f, None, it, skip=e, counts=True)
    plain_want = ssr.sweep_segment_rows_ref(v, x1, f, None, it)
    assert counts[2] == 0 and want.rows.shape[0] > 100 and ne % 64 != 0
    with _ctx(v, f) as cd:
        rows = _sweep(cd, it, x1, "cloth, skip", skip=e)
        assert _counts(cd) == counts
        plain = _sweep(cd, it, x1, "cloth, no skip")
        first = _first(cd, it, x1, skip=e)
        some = e.copy(); some[::2] = NONE                                       # every second item without a filter
        mixed = _sweep(cd, it, x1, "cloth, every second skip", skip=some)
        half = e.copy(); half[:, 1] = NONE                                      # one index and none
        one = _sweep(cd, it, x1, "cloth, first index only", skip=half)
    wr.same_rows(rows, want, "cloth, skip")
    wr.same_rows(plain, plain_want, "cloth, no skip")
    fv = f[rows.rows[:, 1].astype(np.int64)].astype(np.int64)
    assert not (fv[:, :, None] == e[rows.rows[:, 0].astype(np.int64)].astype(np.int64)[:, None, :]).any()      # no row's face holds either index
    pv = f[plain.rows[:, 1].astype(np.int64)].astype(np.int64)
    pe = e[plain.rows[:, 0].astype(np.int64)].astype(np.int64)
    inc = (pv[:, :, None] == pe[:, None, :]).any(axis=(1, 2))
    assert inc.sum() >= ne and np.all(plain.toi[inc] == 0.0)                    # without the skip every face at the edge's ends is a row at toi 0
    wr.same_rows(type(plain)(*(a[~inc] for a in plain)), want, "cloth, the rest")
    wr.same_rows(mixed, type(plain)(*(a[~inc | (plain.rows[:, 0] % 2 == 0)] for a in plain)), "cloth, every second skip")
    wr.same_rows(one, type(plain)(*(a[~(pv == pe[:, 0:1]).any(axis=1)] for a in plain)), "cloth, first index only")
    _same_tuple(first[:12], ssr.first_of(rows, ne), "cloth, first contact with skip")


# ---------------------------------------------------------------- 6: independence
def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def test_independent_of_frame_traversal_build_cell_table_and_item_order():
    name = "soup10k"
    v, i, ids, edge = ssr.MESHES[name]
    it, x1 = ssr.items(name), ssr.mesh_end(name)
    want, counts = ssr.want(name)
    n = it.shape[0]
    perm = np.random.default_rng(4).permutation(n).astype(np.uint32)
    first_want = ssr.first_of(want, n)

    def check(cd, what):
        wr.same_rows(_sweep(cd, it, x1, what), want, what)
        assert _counts(cd) == counts, what
        w = _sweep(cd, it[perm], x1, what + ", permuted")
        rows = w.rows.copy(); rows[:, 0] = perm[rows[:, 0]]
        wr.same_rows(wr.sort_rows(rows, *w[1:]), want, what + ", permuted")
        _same_tuple(_first(cd, it, x1)[:12], first_want, what)

    with mi355cd.CollisionDetector(v, i) as cd:
        for frame in (mi355cd.CD_FRAME_REFERENCE, mi355cd.CD_FRAME_AUTO, mi355cd.CD_FRAME_CUSTOM):
            for trav in (0, 1, 3):
                for stagewise in (0, 1):
                    if stagewise and trav != 3:
                        continue
                    cd.set_option(mi355cd.CD_OPT_TRAVERSAL, trav)
                    cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, stagewise)
                    _frame(cd, frame)
                    cd.self_collide(cap=CAP)                               # the tree of this setting (the collision step builds it)
                    check(cd, f"frame {frame} traversal {trav} stagewise {stagewise}")
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)
        cd.set_morton_frame(mi355cd.CD_FRAME_REFERENCE)
        cd.set_option(mi355cd.CD_OPT_CELL_TABLE, 0)
        cd.self_collide(cap=CAP)
        check(cd, "cell table 0")
        cd.build_tree()                                                    # the staged build
        check(cd, "cell table 0, build_tree")
        still, still_counts = ssr.want(name, moving=False)                 # a mesh that does not move: NULL, or its own vertices
        assert still.rows.shape[0] > 50 and not np.array_equal(still.rows, want.rows)
        wr.same_rows(_sweep(cd, it, None, "verts_end None"), still, "verts_end None")
        wr.same_rows(_sweep(cd, it, np.asarray(v, dtype=np.float64), "verts_end = the vertices"), still, "verts_end None against the vertices themselves")
        _same_tuple(_first(cd, it, np.asarray(v, dtype=np.float64))[:12], _first(cd, it, None)[:12], "first contact, verts_end None against the vertices themselves")


# ---------------------------------------------------------------- 7: overflow and growth, through the C interface
SENTINEL = 7
FIELDS = (("ids", np.uint32, ()), ("toi", np.float64, ()), ("dist", np.float64, ()), ("s", np.float64, ()), ("on_seg", np.float64, (3,)), ("on_tri", np.float64, (3,)),
          ("uv", np.float64, (2,)), ("feature", np.uint8, ()), ("end", np.uint8, ()), ("cross", np.uint8, ()), ("side", np.uint8, ()))


class _Raw:
    """A cd_sweep_segments_all call through the C interface into sentinel-filled arrays of `room` rows."""

    def __init__(self, cd, room):
        self.cd = cd
        self.rows = np.full((max(room, 1), 2), SENTINEL, dtype=np.uint32)
        self.vals = [np.full((max(room, 1),) + shape, SENTINEL, dtype=dt) for _, dt, shape in FIELDS]
        self.out = mi355cd.CdSweepSegmentRows(*(a.ctypes.data for a in self.vals))
        self.n, self.info = C.c_uint64(SENTINEL), mi355cd.CdCcdInfo(SENTINEL, SENTINEL, SENTINEL, SENTINEL)

    def call(self, items, cap, x1=None, skip=None, n=None, null=False):
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        n = items.shape[0] if n is None else n
        return self.cd.lib.cd_sweep_segments_all(self.cd._ctx, vp(x1), vp(items), n, vp(skip), None if null else vp(self.rows), cap, C.byref(self.n),
                                                 None if null else C.byref(self.out), C.byref(self.info))

    def untouched_from(self, at):
        return all((a[at:] == SENTINEL).all() for a in [self.rows] + self.vals)

    def nothing_written(self):
        return self.untouched_from(0) and self.n.value == SENTINEL and self.info.n_tested == SENTINEL and self.info.n_candidates == SENTINEL

    def written(self, count):
        return (self.rows[:count],) + tuple(a[:count] for a in self.vals)


def _distinct_members(got, want, what):
    g = wr.sort_rows(*got)
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(32)) | r[:, 1].astype(np.uint64)
    kg, kw = key(g[0]), key(want.rows)
    assert np.unique(kg).size == kg.size, what
    at = np.minimum(np.searchsorted(kw, kg), kw.size - 1)
    assert np.array_equal(kw[at], kg), what
    wr.same_rows(g, type(want)(*(a[at] for a in want)), what)


def test_overflow():
    name = "soup10k"
    v, i, ids, edge = ssr.MESHES[name]
    it, x1 = ssr.items(name), ssr.mesh_end(name)
    want, counts = ssr.want(name)
    total = want.rows.shape[0]
    assert total > 130
    far = it.copy(); far[:, 0:12] += 100.0
    with _ctx(v, i, ids) as cd:
        r = _Raw(cd, 0)                                                     # the count-only call
        assert r.call(it, 0, x1, null=True) == OVERFLOW and r.n.value == total and r.info.n_tested == counts[0]
        assert r.call(far, 0, x1, null=True) == OK and r.n.value == 0
        r = _Raw(cd, total + 64)                                            # one row short
        assert r.call(it, total - 1, x1) == OVERFLOW and r.n.value == total
        assert r.untouched_from(total - 1), "written at or past cap_rows"
        _distinct_members(r.written(total - 1), want, "cap = n_rows - 1")
        r = _Raw(cd, total + 64)                                            # a small prefix
        assert r.call(it, 65, x1) == OVERFLOW and r.n.value == total and r.untouched_from(65)
        _distinct_members(r.written(65), want, "cap = 65")
        r = _Raw(cd, total + 64)                                            # exactly enough
        assert r.call(it, total, x1) == OK and r.n.value == total and r.untouched_from(total)
        wr.same_rows(r.written(total), want, "cap = n_rows")
        r = _Raw(cd, total)                                                 # rows only: out and info NULL
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert cd.lib.cd_sweep_segments_all(cd._ctx, vp(x1), vp(it), it.shape[0], None, vp(r.rows), total, C.byref(r.n), None, None) == OK
        assert np.array_equal(wr.sort_rows(r.rows)[0], want.rows) and all((a == SENTINEL).all() for a in r.vals)


def test_candidate_buffer_grows_and_shrinking_calls_still_work():
    name = "soup10k"
    v, i, ids, edge = ssr.MESHES[name]
    it, x1 = ssr.items(name), ssr.mesh_end(name)
    want, counts = ssr.want(name)
    nt = i.shape[0]
    p = np.ascontiguousarray(np.concatenate([it[:, 0:3], it[:, 0:3], it[:48, 0:3]], axis=0))
    assert p.shape[0] == 2048 and 2048 * nt >= 2 * mi355cd.WITHIN_SHARD_FIRST * mi355cd.WITHIN_SHARDS       # twice the first allocation, and more
    one = _sub(want, 1)
    with _ctx(v, i, ids) as cd:
        wr.same_rows(_sweep(cd, it[:1], x1, "one item"), one, "one item")
        # resting points with a dist beyond the whole scene, the mesh at rest: every triangle is a candidate and a row, one evaluation each
        rows, *_, n, rc = cd.sweep_segments_all(p, p, p, p, 1.0e4, cap=0)
        info = cd.sweep_segments_info
        assert rc == OVERFLOW and rows.shape[0] == 0 and n == 2048 * nt, (rc, n)
        assert info.n_candidates == info.n_tested == info.n_evals == 2048 * nt and info.n_unresolved == 0
        wr.same_rows(_sweep(cd, it[:1], x1, "one item again"), one, "one item again")
        wr.same_rows(_sweep(cd, it, x1, "all items"), want, "all items after the growth")


# ---------------------------------------------------------------- 8: the context, errors, a mesh that moves
def test_leaves_the_context_as_it_was_and_errors_write_nothing():
    name = "soup10k"
    v, i, ids, edge = ssr.MESHES[name]
    v = np.asarray(v, dtype=np.float64)
    it, x1 = ssr.items(name), ssr.mesh_end(name)
    want, counts = ssr.want(name)
    it64 = np.ascontiguousarray(it[:64])
    p0, p1 = np.ascontiguousarray(it[:, 0:3]), np.ascontiguousarray(it[:, 6:9])
    with mi355cd.CollisionDetector(v, i) as cd:
        r = _Raw(cd, 256)                                                   # before a build
        assert r.call(it64, 256, x1) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        cd.self_collide(cap=CAP)
        ccd = cd.find_ccd(x1, 0.1 * edge, cap=CAP)
        assert ccd[3] > 0
        before = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(), cd.debug_swept(),
                  cd.sweep_points_all(p0, p1, 0.5 * edge, verts_end=x1, cap=CAP), cd.segments_within(it[:, 0:3], it[:, 3:6], edge, cap=CAP))
        wr.same_rows(_sweep(cd, it, x1, name), want, name)
        _first(cd, it, x1)
        other = v + 0.37 * edge                                             # another x1: the shared swept records change, the CCD pass's do not
        assert _sweep(cd, it, other, name + ", another x1").rows.shape[0] > 0
        assert bytes(cd.stats()) == before[0]
        assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == before[1]
        after = cd.debug_swept()
        assert before[2][0].shape[0] == i.shape[0] and all(np.array_equal(a, b) for a, b in zip(before[2][:3], after[:3])) and before[2][3:] == after[3:]
        _same_tuple(wr.sort_rows(*cd.sweep_points_all(p0, p1, 0.5 * edge, verts_end=x1, cap=CAP)[:8]), wr.sort_rows(*before[3][:8]), "sweep_points_all after the segment sweeps")
        _same_tuple(wr.sort_rows(*cd.segments_within(it[:, 0:3], it[:, 3:6], edge, cap=CAP)[:11]), wr.sort_rows(*before[4][:11]), "segments_within after the segment sweeps")
        assert before[3][8] > 50 and before[4][11] > 50
        wr.same_rows(_sweep(cd, it, x1, name + ", after the swept-point call"), want, name + ", after the swept-point call")
        again = cd.find_ccd(x1, 0.1 * edge, cap=CAP)
        assert again[3] == ccd[3] and np.array_equal(np.sort(again[0].view(np.uint64).ravel()), np.sort(ccd[0].view(np.uint64).ravel()))

        vp = lambda a: a.ctypes.data_as(C.c_void_p)

        def first_raw(items, n, flags=0, face_null=False):
            face = np.full(64, SENTINEL, dtype=np.uint32)
            o = _Raw(cd, 64)
            info = mi355cd.CdPointInfo(SENTINEL, SENTINEL, SENTINEL)
            rc = cd.lib.cd_sweep_segments(cd._ctx, vp(x1), vp(items), n, None, flags, None if face_null else vp(face), C.byref(o.out), C.byref(info))
            return rc, (face == SENTINEL).all() and o.untouched_from(0) and info.n_found == SENTINEL

        def bad(items, what, n=None):
            r = _Raw(cd, 256)
            assert r.call(items, 256, x1, n=n) == mi355cd.CD_ERR_ARG and r.nothing_written(), what
            assert first_raw(items, items.shape[0] if n is None else n) == (mi355cd.CD_ERR_ARG, True), what

        for col in range(12):
            for val in (np.nan, np.inf, -np.inf):
                x = it64.copy(); x[63, col] = val                           # the LAST item: nothing may have been launched for the others
                bad(x, (col, val))
        for val in (0.0, -1.0, np.inf, -np.inf, np.nan):
            x = it64.copy(); x[63, 12] = val
            bad(x, ("dist", val))
        bad(it64, "n = 2^32 + 1", n=(1 << 32) + 1)                          # (checked before the 64 items are read)
        r = _Raw(cd, 256)
        assert cd.lib.cd_sweep_segments_all(cd._ctx, None, None, 64, None, vp(r.rows), 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG        # NULL items
        assert cd.lib.cd_sweep_segments_all(cd._ctx, None, vp(it64), 64, None, None, 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG           # NULL rows with room asked for
        assert cd.lib.cd_sweep_segments_all(cd._ctx, None, vp(it64), 64, None, vp(r.rows), 256, None, None, None) == mi355cd.CD_ERR_ARG and r.nothing_written()   # NULL n_rows
        assert r.call(it64, 256, n=0) == OK and r.n.value == 0 and r.untouched_from(0)                                                          # n = 0
        assert first_raw(it64, 64, flags=1) == (mi355cd.CD_ERR_ARG, True)                                                                        # flags
        assert first_raw(it64, 64, face_null=True) == (mi355cd.CD_ERR_ARG, True)                                                                 # NULL face
        assert first_raw(it64, 0)[0] == OK

        g = np.random.default_rng(9)
        moved = v + g.normal(0.0, 0.5 * edge, v.shape)
        cd.update_vertices(moved)
        r = _Raw(cd, 256)                                                   # after update_vertices without a rebuild
        assert r.call(it64, 256, x1) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        assert first_raw(it64, 64) == (mi355cd.CD_ERR_ORDER, True)
        cd.build_tree()
        new = ssr.sweep_segment_rows_ref(moved, x1, i, None, it)
        assert new.rows.shape != want.rows.shape or not np.array_equal(new.rows, want.rows)      # the answer did change
        wr.same_rows(_sweep(cd, it, x1, "moved"), new, "after update_vertices and a rebuild")
        _same_tuple(_first(cd, it, x1)[:12], ssr.first_of(new, it.shape[0]), "first contact after update_vertices and a rebuild")


def test_a_mesh_that_steps_through_every_rebuild_path():
    """The `slide` sequence of tests/moving_inputs.py, one frame through each rebuild entry of tests/test_moving_mesh_gpu.py: after every
    rebuild the frame's own edges (every fifth, skip_vertices = the edge) swept to the frame's x1 give the restatement's rows of THIS
    frame, and the first contacts their minima; between update_vertices and the rebuild the calls return CD_ERR_ORDER."""
    from test_moving_mesh_gpu import ENTRIES, _enter
    name = "slide"
    s = mi.seq(name)
    f = np.asarray(s.vidx)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64), axis=1), axis=0)
    e = np.ascontiguousarray(e[::5].astype(np.uint32))
    assert len(s.frames) >= len(ENTRIES) and e.shape[0] % 64 != 0
    used, sizes = [], []
    with mi355cd.CollisionDetector(s.frames[0], s.vidx) as cd:
        for k, v in enumerate(s.frames):
            v = np.asarray(v, dtype=np.float64)
            x1 = np.asarray(mi.x1(name, k), dtype=np.float64)
            it = ssr.pack(v[e[:, 0]], v[e[:, 1]], x1[e[:, 0]], x1[e[:, 1]], 0.25 * mi.edge_at(name, k))
            cd.update_vertices(v)
            r = _Raw(cd, 16)
            assert r.call(it, 16, x1, skip=e) == mi355cd.CD_ERR_ORDER and r.nothing_written()
            entry = ENTRIES[k % len(ENTRIES)]
            _enter(cd, entry, x1, mi.prox_dist(name, k), mi.ccd_dist(name, k))
            used.append(entry)
            want, counts = ssr.sweep_segment_rows_ref(v, x1, s.vidx, None, it, skip=e, counts=True)
            what = f"{name} frame {k} behind {entry}"
            wr.same_rows(_sweep(cd, it, x1, what, skip=e), want, what)
            assert _counts(cd) == counts, what
            _same_tuple(_first(cd, it, x1, skip=e)[:12], ssr.first_of(want, it.shape[0]), what + ", first contact")
            sizes.append(want.rows.shape[0])
    assert set(used) == set(ENTRIES) and sum(n > 0 for n in sizes) >= len(sizes) - 1 and len(set(sizes)) > 2, sizes


# ---------------------------------------------------------------- 9: the scales inside seg_tri's band, and a translated mesh
SCALE_MESHES = {k: v for k, v in si.meshes().items() if k in ("cloth", "centred")}
BAND = tuple(k for k in si.SCALES if abs(k) <= 256)                            # seg_tri's band is ray_tri's, about 2^-300 .. 2^300; -320 lies outside
NSCALE = 512


@functools.lru_cache(maxsize=None)
def _scale_case(name, off=0.0):
    """512 segments at the mesh (translated by off) moved by about 0.6 edge, dist a quarter edge, the mesh moving to scale_inputs.motion:
    the restatement's rows and counts."""
    import point_ref as ptr
    v, vidx, edge = SCALE_MESHES[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    g = np.random.default_rng(21)
    a0 = ptr.mesh_points(vv, vidx, NSCALE, seed=3, edge=edge)
    b0 = a0 + g.normal(size=a0.shape) * edge
    common = g.normal(size=a0.shape) * 0.6 * edge
    it = ssr.pack(a0, b0, a0 + common + g.normal(size=a0.shape) * 0.2 * edge, b0 + common + g.normal(size=a0.shape) * 0.2 * edge, 0.25 * edge)
    x1 = si.motion(vv, edge)
    if off:
        vv, x1 = vv + off, x1 + off
        it[:, 0:12] += off
    want, counts = ssr.sweep_segment_rows_ref(vv, x1, vidx, None, it, counts=True)
    return vv, vidx, x1, it, want, counts


def _scale_conditions(want, counts):
    per = np.bincount(want.rows[:, 0].astype(np.int64), minlength=NSCALE)
    inside = int(((want.toi > 0) & (want.toi < 1)).sum())
    assert (per == 0).sum() >= 32 and (per >= 2).sum() >= 32 and inside >= 4 and (want.cross == 1).any(), ((per == 0).sum(), (per >= 2).sum(), inside, counts)


@pytest.mark.parametrize("k", BAND)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_scales_in_band(name, k):
    """Mesh, end positions and all thirteen columns of the items scaled by 2^k, past both fp32 ends: the k = 0 rows, IDs, toi bits, s, u,
    v, feature, end, cross and side, dist, qs and qt times 2^k exactly, and the k = 0 counts; at the scales of scale_inputs.EDGES also
    the restatement on the scaled inputs themselves; first contact: first_of of those rows."""
    vv, vidx, x1, it, want, counts = _scale_case(name)
    _scale_conditions(want, counts)
    what = f"{name} 2^{k}"
    ws = want._replace(dist=si.scaled(want.dist, k), on_seg=si.scaled(want.on_seg, k), on_tri=si.scaled(want.on_tri, k))
    vs, xs, its = si.scaled(vv, k), si.scaled(x1, k), si.scaled(it, k)
    with _ctx(vs, vidx) as cd:
        rows = _sweep(cd, its, xs, what)
        wr.same_rows(rows, ws, what)
        assert _counts(cd) == counts, (what, _counts(cd), counts)
        if k in si.EDGES:
            direct, direct_counts = ssr.sweep_segment_rows_ref(vs, xs, vidx, None, its, counts=True)
            wr.same_rows(rows, direct, what + ", the restatement on the scaled inputs")
            assert _counts(cd) == direct_counts, (what, _counts(cd), direct_counts)
        _same_tuple(_first(cd, its, xs)[:12], ssr.first_of(ws, NSCALE), what + ", first contact")


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_mesh_gives_the_restatement(name):
    """Mesh, end positions and the items' twelve coordinates translated by 2^20 + 0.37: M is 2^20 while the motion is a fraction of an
    edge, so the pad's M 2^-20 term (about 1) decides which candidates pass the fp32 filters."""
    vt, vidx, xt, itt, want, counts = _scale_case(name, 2.0 ** 20 + 0.37)
    per = np.bincount(want.rows[:, 0].astype(np.int64), minlength=NSCALE)
    print(f"{name} translated: {want.rows.shape[0]} rows, {int((per == 0).sum())} of {NSCALE} items with none, {int((per >= 2).sum())} with several, counts {counts}")
    assert (per == 0).sum() >= 32 and (per >= 2).sum() >= 32
    with _ctx(vt, vidx) as cd:
        wr.same_rows(_sweep(cd, itt, xt, name), want, f"{name} translated")
        assert _counts(cd) == counts, (name, _counts(cd), counts)
        _same_tuple(_first(cd, itt, xt)[:12], ssr.first_of(want, NSCALE), f"{name} translated, first contact")
