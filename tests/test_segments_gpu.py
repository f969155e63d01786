"""The segment queries on the device (cd_segments_within, cd_segments_closest, cd_seg_tri_points) against the all-pairs restatement of
tests/segment_ref.py -- which uses no box filter of any kind -- as sets of (item, face) and bit for bit in every value of a row, and
against the device's own point and ray queries where the contract says they are the same thing.  Every step has bounded size."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import mi355_synth as synth
import mi355cd
import oracle
import proximity_ref as pr
import scale_inputs as si
import segment_ref as sr
import within_ref as wr

pytestmark = pytest.mark.gpu

CAP = 1 << 20
NAMES = sr.SMALL + ["cloth100"]
OK, OVERFLOW = mi355cd.CD_OK, mi355cd.CD_OVERFLOW
BAND = (-300, -127, 127, 300)                                                  # ray_tri's band ends and the fp32 ends


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _within(cd, segs, r, what, cap=CAP):
    """segments_within's rows as a SegRows sorted by (item, face); the call fitted its capacity."""
    got = cd.segments_within(segs[:, 0:3], segs[:, 3:6], r, cap=cap)
    assert got[12] == OK and got[11] == got[0].shape[0] and cd.segments_tested >= got[11], (what, got[11:], cd.segments_tested)
    return sr.SegRows(*wr.sort_rows(*got[:11]))


def _same_tuple(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        if b.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        assert np.array_equal(a, b), (what, k)


# ---------------------------------------------------------------- 1: the predicate's pin
def test_seg_tri_points_is_the_restatement_bit_for_bit():
    """cd_seg_tri_points on the CPU tests' vectors, and on those of order 1 scaled to the ends of the band."""
    segs, tris = sr.pin_inputs(512, 7)
    unit = np.abs(segs).max(axis=1) < 64.0                                      # (not the offset classes: another 2^300 leaves the band)
    sets = [(segs, tris)] + [(np.ldexp(segs[unit], k), np.ldexp(tris[unit], k)) for k in BAND]
    for s, p in sets:
        want = sr.seg_tri_np(s, p)
        got = mi355cd.seg_tri_points(s, p)
        _same_tuple(got, want[:9], "seg_tri")
    got = mi355cd.load_library().cd_seg_tri_points                             # every output but dist may be NULL
    dist = np.zeros(8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    s8, p8 = np.ascontiguousarray(segs[:8]), np.ascontiguousarray(tris[:8])
    assert got(vp(s8), vp(p8), 8, vp(dist), *([None] * 8)) == OK and np.array_equal(_bits(dist), _bits(sr.seg_tri_np(s8, p8).dist))


# ---------------------------------------------------------------- 2, 3: the row sets, and their minima against the single-answer call
@pytest.mark.parametrize("name", NAMES)
def test_row_sets_are_the_restatements(name):
    """Segments at radius edge and 3 edge: the restatement's set of (item, face), and every value of every row bit for bit."""
    sr.input_conditions(name)
    v, i, ids, edge = sr.MESHES[name]
    segs = sr.segments(name)
    assert segs.shape[0] == sr.n_items(name)
    with _ctx(v, i, ids) as cd:
        for factor in sr.FACTORS:
            want = sr.want(name, factor)
            wr.same_rows(_within(cd, segs, factor * edge, name), want, f"{name}, segments within {factor} edge")
            print(f"{name}: {want.rows.shape[0]} rows within {factor} edge, {cd.segments_tested} seg_tri")
            assert i.shape[0] > 1 or cd.segments_tested == segs.shape[0]        # one triangle: no records, every item tests leaf 0


@pytest.mark.parametrize("name", NAMES)
def test_the_smallest_row_of_an_item_is_segments_closests_answer(name):
    """By definition: per item the row with the smallest (dist, ID, face) is segments_closest's answer of the DEVICE, bit for bit, the
    items with no row are its 0xFFFFFFFF items, and CD_SEGMENT_ANY finds exactly those that have a row.  With no radius the answer is
    the restatement's nearest triangle."""
    v, i, ids, edge = sr.MESHES[name]
    segs = sr.segments(name)
    n = segs.shape[0]
    with _ctx(v, i, ids) as cd:
        for factor in sr.FACTORS:
            rows = _within(cd, segs, factor * edge, name)
            single = cd.segments_closest(segs[:, 0:3], segs[:, 3:6], factor * edge)
            _same_tuple(single[:11], sr.closest_of(rows, n), f"{name}, {factor} edge")
            _same_tuple(single[:11], sr.closest_of(sr.want(name, factor), n), f"{name}, {factor} edge, the restatement")
            none = wr.rows_per_item(rows, n) == 0
            assert np.array_equal(none, single[0] == mi355cd.SEGMENT_NONE) and single[11].n_found == n - none.sum()
            face, info = cd.segments_closest(segs[:, 0:3], segs[:, 3:6], factor * edge, any_within=True)
            assert np.array_equal(face == mi355cd.SEGMENT_NONE, none) and info.n_found == n - none.sum()
            key = set(map(tuple, rows.rows.tolist()))
            assert all((k, int(f)) in key for k, f in enumerate(face) if f != mi355cd.SEGMENT_NONE)      # SOME triangle within r
        if i.shape[0] <= 5000:                                                  # the nearest triangle wherever it is
            m = min(n, 128)
            single = cd.segments_closest(segs[:m, 0:3], segs[:m, 3:6])
            items = np.concatenate([segs[:m], np.full((m, 1), np.inf)], axis=1)
            _same_tuple(single[:11], sr.segments_closest_ref(v, i, ids, items), f"{name}, r = +inf")
            assert (single[0] != mi355cd.SEGMENT_NONE).all()


# ---------------------------------------------------------------- 4: independence
def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def _unpermuted(w, perm):
    """The rows of a call on items[perm], as rows of the items: item j of the call is item perm[j]."""
    rows = w.rows.copy()
    rows[:, 0] = perm[rows[:, 0]]
    return type(w)(*wr.sort_rows(rows, *w[1:]))


def test_independent_of_frame_traversal_build_cell_table_and_item_order():
    name = "soup10k"
    v, i, ids, edge = sr.MESHES[name]
    segs = sr.segments(name)
    n = segs.shape[0]
    want = sr.want(name, 3.0)
    want_single = sr.closest_of(want, n)
    perm = np.random.default_rng(4).permutation(n).astype(np.uint32)

    def check(cd, what):
        wr.same_rows(_within(cd, segs, 3 * edge, what), want, what)
        wr.same_rows(_unpermuted(_within(cd, segs[perm], 3 * edge, what), perm), want, what + ", permuted")
        _same_tuple(cd.segments_closest(segs[:, 0:3], segs[:, 3:6], 3 * edge)[:11], want_single, what + ", closest")
        got = cd.segments_closest(segs[perm, 0:3], segs[perm, 3:6], 3 * edge)[:11]
        _same_tuple(got, tuple(x[perm] for x in want_single), what + ", closest permuted")

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


# ---------------------------------------------------------------- 5, 6: a point is a point, a crossing is a ray's hit
@pytest.mark.parametrize("name", ["soup10k", "custom_ids", "n65", "cloth100"])
def test_point_segments_are_the_point_queries(name):
    """Items with a == b: points_within's rows and closest_points' answers of the device, bit for bit."""
    v, i, ids, edge = sr.MESHES[name]
    a = sr.segments(name)[:, 0:3]
    pp = np.concatenate([a, a], axis=1)
    with _ctx(v, i, ids) as cd:
        for factor in sr.FACTORS:
            s = _within(cd, pp, factor * edge, name)
            got = cd.points_within(a, factor * edge, cap=CAP)
            assert got[8] == OK
            p = wr.PointRows(*wr.sort_rows(*got[:7]))
            assert p.rows.shape[0] > 0
            _same_tuple((s.rows, s.ids, s.dist, s.on_tri, s.uv, s.feature, s.side), tuple(p), f"{name}, {factor} edge")
            assert (s.cross == 0).all() and (s.end == 1).all() and (s.s == 0.0).all() and np.array_equal(_bits(s.on_seg), _bits(a[s.rows[:, 0].astype(np.int64)]))
            c = cd.segments_closest(a, a, factor * edge)
            q = cd.closest_points(a, factor * edge)
            _same_tuple((c[0], c[1], c[2], c[5], c[6], c[7], c[10]), q[:7], f"{name}, {factor} edge, closest")


@pytest.mark.parametrize("name", ["soup10k", "custom_ids", "n65", "cloth100"])
def test_crossing_rows_are_cast_rays_alls_rows(name):
    """The cross = 1 rows of an item set are exactly cast_rays_all(a, b - a, tmax = 1)'s rows, with s = t and uv, side bit for bit.
    (The zero-length items have no direction: they have no crossing row and are not cast.)"""
    v, i, ids, edge = sr.MESHES[name]
    segs = sr.segments(name)
    d = segs[:, 3:6] - segs[:, 0:3]
    live = np.nonzero((d != 0.0).any(axis=1))[0]
    with _ctx(v, i, ids) as cd:
        s = _within(cd, segs, 3 * edge, name)
        assert not np.isin(s.rows[s.cross == 1, 0], np.setdiff1d(np.arange(segs.shape[0]), live)).any()
        got = cd.cast_rays_all(segs[live, 0:3], d[live], 1.0, cap=CAP)
        assert got[6] == OK
        rows = got[0].copy()
        rows[:, 0] = live[rows[:, 0]]
        r = wr.RayRows(*wr.sort_rows(rows, *got[1:5]))
        c = s.cross == 1
        assert c.sum() > 0
        _same_tuple((s.rows[c], s.ids[c], s.s[c], s.uv[c], s.side[c]), tuple(r), name)
        assert (s.dist[c] == 0.0).all() and (s.feature[c] == 0).all()


# ---------------------------------------------------------------- 7: capacity and growth, through the C interface
SENTINEL = 7
ROW = (("ids", np.uint32, ()), ("dist", np.float64, ()), ("s", np.float64, ()), ("on_seg", np.float64, (3,)), ("on_tri", np.float64, (3,)), ("uv", np.float64, (2,)),
       ("feature", np.uint8, ()), ("end", np.uint8, ()), ("cross", np.uint8, ()), ("side", np.uint8, ()))


class _Raw:
    """A call through the C interface into sentinel-filled arrays of `room` rows."""

    def __init__(self, cd, room):
        self.cd, self.room = cd, room
        self.rows = np.full((max(room, 1), 2), SENTINEL, dtype=np.uint32)
        self.face = np.full(max(room, 1), SENTINEL, dtype=np.uint32)
        self.vals = [np.full((max(room, 1),) + shape, SENTINEL, dtype=dt) for _, dt, shape in ROW]
        self.out = mi355cd.CdSegmentRows(*(a.ctypes.data for a in self.vals))
        self.n, self.tested = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
        self.info = mi355cd.CdSegmentInfo(SENTINEL, SENTINEL, SENTINEL)

    def call(self, items, cap, n=None, null=False):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        n = items.shape[0] if n is None else n
        return self.cd.lib.cd_segments_within(self.cd._ctx, vp(items), n, None if null else vp(self.rows), cap, C.byref(self.n), C.byref(self.tested),
                                              None if null else C.byref(self.out))

    def closest(self, items, flags=0, n=None, out=True):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        n = items.shape[0] if n is None else n
        return self.cd.lib.cd_segments_closest(self.cd._ctx, vp(items), n, flags, vp(self.face), C.byref(self.out) if out else None, C.byref(self.info))

    def untouched_from(self, at):
        return all((a[at:] == SENTINEL).all() for a in [self.rows] + self.vals)

    def nothing_written(self):
        return (self.untouched_from(0) and (self.face == SENTINEL).all() and self.n.value == SENTINEL and self.tested.value == SENTINEL and
                (self.info.n_found, self.info.node_visits, self.info.tri_tests) == (SENTINEL,) * 3)

    def written(self, count):
        return (self.rows[:count],) + tuple(a[:count] for a in self.vals)


def _distinct_members(got, want, what):
    """got's rows are distinct rows of want's set, with want's values."""
    g = wr.sort_rows(*got)
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(32)) | r[:, 1].astype(np.uint64)
    kg, kw = key(g[0]), key(want.rows)
    assert np.unique(kg).size == kg.size, what
    at = np.minimum(np.searchsorted(kw, kg), kw.size - 1)
    assert np.array_equal(kw[at], kg), what
    wr.same_rows(g, type(want)(*(a[at] for a in want)), what)


def test_overflow():
    name = "soup10k"
    v, i, ids, edge = sr.MESHES[name]
    items, want = sr.items(name, 3.0), sr.want(name, 3.0)
    empty = items.copy(); empty[:, 0:6] += 100.0; empty[:, 6] = 0.0            # far from the mesh, radius 0: no rows
    total = want.rows.shape[0]
    assert total > 64
    with _ctx(v, i, ids) as cd:
        r = _Raw(cd, 0)                                                         # the count-only call
        assert r.call(items, 0, null=True) == OVERFLOW and r.n.value == total and r.tested.value >= total
        assert r.call(empty, 0, null=True) == OK and r.n.value == 0
        r = _Raw(cd, total + 64)                                                # one row short
        assert r.call(items, total - 1) == OVERFLOW and r.n.value == total
        assert r.untouched_from(total - 1), "written at or past cap_rows"
        _distinct_members(r.written(total - 1), want, "cap = n_rows - 1")
        r = _Raw(cd, total + 64)                                                # a small prefix
        assert r.call(items, 65) == OVERFLOW and r.n.value == total and r.untouched_from(65)
        _distinct_members(r.written(65), want, "cap = 65")
        r = _Raw(cd, total + 64)                                                # exactly enough
        assert r.call(items, total) == OK and r.n.value == total and r.untouched_from(total)
        wr.same_rows(r.written(total), want, "cap = n_rows")
        r = _Raw(cd, total + 64)                                                # one above
        assert r.call(items, total + 1) == OK and r.n.value == total and r.untouched_from(total)
        wr.same_rows(r.written(total), want, "cap = n_rows + 1")
        r = _Raw(cd, total)                                                     # rows only: out and n_tested NULL
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert cd.lib.cd_segments_within(cd._ctx, vp(items), items.shape[0], vp(r.rows), total, C.byref(r.n), None, None) == OK
        assert np.array_equal(wr.sort_rows(r.rows)[0], want.rows) and all((a == SENTINEL).all() for a in r.vals)


def test_infinite_radius_returns_every_triangle():
    v, i, ids, edge = sr.MESHES["n65"]
    segs = sr.segments("n65")[:130]
    with _ctx(v, i, ids) as cd:
        rows = _within(cd, segs, np.inf, "n65")
        assert rows.rows.shape[0] == 130 * 65 and cd.segments_tested == 130 * 65
        assert np.array_equal(rows.rows, np.stack(np.divmod(np.arange(130 * 65, dtype=np.uint32), np.uint32(65)), axis=1))
        wr.same_rows(rows, sr.segments_within_ref(v, i, ids, np.concatenate([segs, np.full((130, 1), np.inf)], axis=1)), "n65, r = +inf")


def test_candidate_buffer_grows_and_shrinking_calls_still_work():
    name = "soup10k"
    v, i, ids, edge = sr.MESHES[name]
    nt = i.shape[0]
    segs = sr.segments(name)
    big = np.ascontiguousarray(np.concatenate([segs, segs, segs[:48]], axis=0))
    assert big.shape[0] == 2048 and 2048 * nt >= 2 * mi355cd.WITHIN_SHARD_FIRST * mi355cd.WITHIN_SHARDS      # twice the first allocation, and more
    one = sr.segments_within_ref(v, i, ids, sr.items(name, 3.0)[:1])
    with _ctx(v, i, ids) as cd:
        wr.same_rows(_within(cd, segs[:1], 3 * edge, "one segment"), one, "one segment")
        got = cd.segments_within(big[:, 0:3], big[:, 3:6], np.inf, cap=0)
        assert got[12] == OVERFLOW and got[0].shape[0] == 0 and got[11] == 2048 * nt and cd.segments_tested == 2048 * nt, (got[11:], cd.segments_tested)
        wr.same_rows(_within(cd, segs[:1], 3 * edge, "one segment again"), one, "one segment again")
        wr.same_rows(_within(cd, segs, 3 * edge, "all segments"), sr.want(name, 3.0), "all segments after the growth")


# ---------------------------------------------------------------- 8: the context, and errors
def test_leaves_the_context_as_it_was_and_errors_write_nothing():
    name = "soup10k"
    v, i, ids, edge = sr.MESHES[name]
    segs = sr.segments(name)
    s7 = sr.items(name, 3.0)[:64].copy()
    with mi355cd.CollisionDetector(v, i) as cd:
        r = _Raw(cd, 256)                                                  # before a build
        assert r.call(s7, 256) == mi355cd.CD_ERR_ORDER and r.closest(s7) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        cd.self_collide(cap=CAP)
        pts = wr.points(name)
        before = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(), cd.find_proximity(0.004, cap=CAP),
                  cd.points_within(pts, 3 * edge, cap=CAP), cd.closest_points(pts, 3 * edge))
        wr.same_rows(_within(cd, segs, 3 * edge, name), sr.want(name, 3.0), name)
        _same_tuple(cd.segments_closest(segs[:, 0:3], segs[:, 3:6], 3 * edge)[:11], sr.closest_of(sr.want(name, 3.0), segs.shape[0]), name)
        assert bytes(cd.stats()) == before[0]
        assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == before[1]
        gp, gd = pr.sort_pairs(*cd.find_proximity(0.004, cap=CAP)[:2])
        wp, wd = pr.sort_pairs(*before[2][:2])
        assert gp.shape[0] > 0 and np.array_equal(gp, wp) and np.array_equal(_bits(gd), _bits(wd))
        wr.same_rows(cd.points_within(pts, 3 * edge, cap=CAP)[:7], wr.PointRows(*wr.sort_rows(*before[3][:7])), "points_within after the segment queries")
        _same_tuple(cd.closest_points(pts, 3 * edge)[:7], before[4][:7], "closest_points after the segment queries")
        wr.same_rows(_within(cd, segs, 3 * edge, name), sr.want(name, 3.0), name + ", after the other queries")

        def bad(items, what, n=None):
            r = _Raw(cd, 256)
            assert r.call(items, 256, n=n) == mi355cd.CD_ERR_ARG and r.nothing_written(), what
            assert r.closest(items, n=n) == mi355cd.CD_ERR_ARG and r.nothing_written(), what

        for col, val in ((0, np.nan), (1, np.inf), (5, -np.inf), (6, np.nan), (6, -1.0), (6, -np.inf)):
            x = s7.copy(); x[63, col] = val                               # the LAST item: nothing may have been launched for the others
            bad(x, ("segment", col, val))
        bad(s7, "n = 2^32", n=1 << 32)                                    # (checked before the 64 items are read)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        r = _Raw(cd, 256)
        assert cd.lib.cd_segments_within(cd._ctx, None, 64, vp(r.rows), 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG            # NULL items
        assert cd.lib.cd_segments_within(cd._ctx, vp(s7), 64, None, 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG                # NULL rows with room asked for
        assert cd.lib.cd_segments_within(cd._ctx, vp(s7), 64, vp(r.rows), 256, None, None, None) == mi355cd.CD_ERR_ARG                  # NULL n_rows
        assert r.closest(s7, flags=2) == mi355cd.CD_ERR_ARG and r.closest(s7, flags=mi355cd.CD_SEGMENT_ANY) == mi355cd.CD_ERR_ARG       # bad flags; out with ANY
        assert cd.lib.cd_segments_closest(cd._ctx, vp(s7), 64, 0, None, None, None) == mi355cd.CD_ERR_ARG and r.nothing_written()       # NULL face
        assert r.call(s7, 256, n=0) == OK and r.n.value == 0 and r.untouched_from(0)                                                    # n = 0
        assert r.closest(s7, n=0) == OK and (r.face == SENTINEL).all() and (r.info.n_found, r.info.node_visits, r.info.tri_tests) == (0, 0, 0)
        zero = s7.copy(); zero[:, 6] = 0.0                                 # r = 0 is a value, not an error
        assert _Raw(cd, 256).call(zero, 256) == OK
        r = _Raw(cd, 256)                                                  # the single-answer call with no optional output at all
        assert r.closest(s7, out=False) == OK and r.untouched_from(0) and (r.face[64:] == SENTINEL).all()
        assert np.array_equal(r.face[:64], sr.closest_of(sr.want(name, 3.0), segs.shape[0])[0][:64])

        moved = np.asarray(v) + 0.001
        cd.update_vertices(moved)
        r = _Raw(cd, 256)                                                  # after update_vertices without a rebuild
        assert r.call(s7, 256) == mi355cd.CD_ERR_ORDER and r.closest(s7) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        cd.build_tree()
        wr.same_rows(_within(cd, segs[:64], 3 * edge, "moved"), sr.segments_within_ref(moved, i, ids, s7), "after update_vertices and a rebuild")


# ---------------------------------------------------------------- 9: the use
def test_edges_of_one_cloth_sheet_against_the_other():
    """What the query is for: the edges of one sheet of cloth_pair(100) (every fourth, to keep the comparison small) against the other
    sheet's triangles at a cloth thickness of half an edge.  Every row's dist is proximity_ref's tri_distance of the degenerate triangle
    (a, b, b) against the face within the recorded bound -- on the rows that are no crossing and that tri_distance's contact early-out
    does not take -- and the nearest row of an edge is segments_closest's answer."""
    v, i = synth.cloth_pair(100)
    v = np.asarray(v, dtype=np.float64)
    i = np.asarray(i)
    half = i.shape[0] // 2
    sheets = []
    for f in (i[:half], i[half:]):
        used = np.unique(f)
        sheets.append((np.ascontiguousarray(v[used]), np.searchsorted(used, f).astype(np.uint32)))
    (va, fa), (vb, fb) = sheets
    e = np.unique(np.sort(np.concatenate([fa[:, [0, 1]], fa[:, [1, 2]], fa[:, [2, 0]]], axis=0), axis=1), axis=0)[::4]
    a, b = va[e[:, 0]], va[e[:, 1]]
    h = 0.5 * 2.88 / 100
    with _ctx(vb, fb) as cd:
        rows = _within(cd, np.concatenate([a, b], axis=1), h, "sheet a's edges against sheet b")
        single = cd.segments_closest(a, b, h)
    _same_tuple(single[:11], sr.closest_of(rows, e.shape[0]), "per-edge minimum")
    k, f = rows.rows[:, 0].astype(np.int64), rows.rows[:, 1].astype(np.int64)
    tris = vb[fb[f].astype(np.int64)]
    pair = np.concatenate([a[k, None], b[k, None], b[k, None], tris], axis=1)
    ok = (rows.cross == 0) & ~pr.in_contact(pair)
    M = np.maximum(np.abs(pair).max(axis=(1, 2)), 0.0)
    err = np.abs(pr.tri_distance_np(pair) - rows.dist)[ok] / M[ok]
    c = wr.rows_per_item(rows, e.shape[0])
    print(f"{e.shape[0]} edges, {rows.rows.shape[0]} rows ({int((rows.cross == 1).sum())} crossings, {int(ok.sum())} compared), {c.min()} .. {c.max()} an edge, "
          f"worst {err.max():.3g} M, {cd.segments_tested} seg_tri")
    assert ok.sum() > 1000 and (rows.cross == 1).sum() > 0 and c.max() > 1 and (c == 0).any()
    assert (err <= sr.TRI_DISTANCE_BOUND).all() and (rows.dist <= h).all()


# ---------------------------------------------------------------- 10: the scales inside seg_tri's band, and a translated mesh
SCALE_BAND = tuple(k for k in si.SCALES if abs(k) <= 256)                      # seg_tri's band is ray_tri's, about 2^-300 .. 2^300; -320 lies outside


def _check_scale_case(vv, vidx, items, want, what):
    """The rows of `items` on the mesh are `want`, and segments_closest is closest_of of them.  -> the rows"""
    with _ctx(vv, vidx) as cd:
        rows = _within(cd, items[:, 0:6], items[:, 6], what)
        wr.same_rows(rows, want, what)
        single = cd.segments_closest(items[:, 0:3], items[:, 3:6], items[:, 6])
        _same_tuple(single[:11], sr.closest_of(want, sr.NSCALE), what + ", closest")
        assert single[11].n_found == int((wr.rows_per_item(want, sr.NSCALE) > 0).sum()), what
    return rows


@pytest.mark.parametrize("k", SCALE_BAND)
@pytest.mark.parametrize("name", sr.SCALE_MESHES)
def test_scales_in_band(name, k):
    """Mesh, both ends and the radius scaled by 2^k, past both fp32 ends -- where the stored boxes SegFilter::meets walks hold +-inf, 0
    and subnormals and the pad 2^-20 max(M, |a|, |b|) overflows or vanishes: the k = 0 rows, with IDs, s, u, v, feature, end, cross and
    side unchanged and dist, on_seg and on_tri times 2^k exactly (tests/test_segment_ref.py: the restatement's own property); at the
    scales of scale_inputs.EDGES also the restatement on the scaled inputs themselves; segments_closest: closest_of of those rows."""
    vv, vidx, items, want = sr.scale_case(name)
    sr.scale_conditions(want)
    what = f"{name} 2^{k}"
    vs, its = si.scaled(vv, k), si.scaled(items, k)
    rows = _check_scale_case(vs, vidx, its, sr.scaled_rows(want, k), what)
    if k in si.EDGES:
        wr.same_rows(rows, sr.segments_within_ref(vs, vidx, None, its), what + ", the restatement on the scaled inputs")


@pytest.mark.parametrize("name", sr.SCALE_MESHES)
def test_translated_mesh_gives_the_restatement(name):
    """Mesh and both ends translated by 2^20 + 0.37: M is 2^20 while the radius is a fraction of an edge, so the pad's M 2^-20 term
    (about 1) decides which leaves pass the fp32 filter."""
    vt, vidx, items, want = sr.scale_case(name, 2.0 ** 20 + 0.37)
    per = sr.scale_conditions(want)
    print(f"{name} translated: {want.rows.shape[0]} rows, {int((per == 0).sum())} of {sr.NSCALE} items with none, {int((per >= 2).sum())} with several")
    _check_scale_case(vt, vidx, items, want, f"{name} translated")
