"""The plane queries on the device (cd_planes_cut_all, cd_planes_count, cd_plane_tri_points) against the restatements of
tests/plane_ref.py -- every plane against every face, no box of any kind -- as sets of (plane, face) and in every value of a row,
and against each other through the definitions that link them.  Every step has bounded size."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import box_ref as br
import closed_meshes as cm
import mi355cd
import moving_inputs as mov
import oracle
import plane_ref as plr
import scale_inputs as si

pytestmark = pytest.mark.gpu

CAP = 1 << 20
OK, OVERFLOW = mi355cd.CD_OK, mi355cd.CD_OVERFLOW


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _rows(cd, planes, what, cap=CAP):
    """planes_cut_all's rows as a PlaneRows sorted by (plane, face); the call fitted its capacity and no (plane, face) comes twice."""
    got = cd.planes_cut_all(planes[:, :3], planes[:, 3], cap=cap)
    n, rc = got[6], got[7]
    assert rc == OK and n == got[0].shape[0] and cd.planes_tested >= n, (what, n, rc, cd.planes_tested)
    key = got[0][:, 0].astype(np.uint64) << np.uint64(32) | got[0][:, 1].astype(np.uint64)
    assert np.unique(key).size == key.size, (what, "a (plane, face) was reported by two slabs")
    return plr.PlaneRows(*plr.wr.sort_rows(*got[:6]))


def _check_counts(cd, planes, cls, what):
    """planes_count against the per-plane sums of the restatement's classes.  -> info"""
    nt = cls.shape[1]
    want = plr.counts_of_classes(cls)
    n_cut, n_below, n_above, info = cd.planes_count(planes[:, :3], planes[:, 3])
    for name, a, b in zip(("n_cut", "n_below", "n_above"), (n_cut, n_below, n_above), want):
        assert np.array_equal(a, b), (what, name, np.nonzero(a != b)[0][:4], a[a != b][:4], b[a != b][:4])
    assert (n_cut.astype(np.int64) + n_below + n_above == nt).all(), what
    assert info.n_found == (want[0] > 0).sum(), what
    return info


# ---------------------------------------------------------------- 1: the pin
def _same_pin(got, want, what):
    for name, a, b in zip(("cls", "seg", "edge", "t", "on"), got, want):
        if b.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero((a.reshape(a.shape[0], -1) != b.reshape(b.shape[0], -1)).any(axis=1))[0]
        assert bad.size == 0, (what, name, bad.size, bad[:8])


def test_plane_tri_points_is_the_restatement_bit_for_bit():
    for what, (planes, tris) in (("integer", plr.integer_family()), ("constructed", plr.constructed_family()), ("unit cube", plr.random_family(0.0)),
                                 ("offset", plr.random_family(plr.OFFSET))):
        want = plr.plane_tri_np(planes, tris)
        _same_pin(mi355cd.plane_tri_points(planes, tris), want, what)
        print(f"{what}: {planes.shape[0]} cases, classes {np.bincount(want[0], minlength=3).tolist()}, with a vertex in the plane {int((want[4] != 0).sum())}")
    assert plr.random_family(0.0)[0].shape[0] == 100_000
    cls = plr.plane_tri_np(*plr.random_family(0.0))[0]
    assert (np.bincount(cls, minlength=3) > 10_000).all()


BAND = tuple(k for k in si.SCALES if abs(k) <= 300) + (-300, 300)              # plane_tri's band (csrc/cd_math.h): ray_tri's


@pytest.mark.parametrize("k", BAND)
def test_plane_tri_points_scaled(k):
    """Triangles and d scaled by 2^k: the k = 0 classes, edges, t and on; a and b scaled; and the restatement on the scaled operands."""
    planes, tris = plr.random_family(0.0, 4000)
    p0, t0 = plr.constructed_family()
    planes, tris = np.concatenate([planes, p0]), np.concatenate([tris, t0])
    want = plr.plane_tri_np(planes, tris)
    pk = planes.copy()
    pk[:, 3] = si.scaled(pk[:, 3], k)
    tk = si.scaled(tris, k)
    got = mi355cd.plane_tri_points(pk, tk)
    _same_pin(got, (want[0], si.scaled(want[1], k), want[2], want[3], want[4]), f"2^{k} against k = 0")
    _same_pin(got, plr.plane_tri_np(pk, tk), f"2^{k} against the restatement")


# ---------------------------------------------------------------- 2: rows and counts
@pytest.mark.parametrize("name", plr.NAMES + plr.SOUPS + plr.CLOSED)
def test_rows_and_counts_are_the_restatements(name):
    """At 1, 63, 64, 65 and 1000 planes: the restatement's set of (plane, face), each once, with every value bit for bit; the counts
    are its per-plane sums (so the rows grouped by plane are planes_count's n_cut); n_above + n_below + n_cut == n."""
    plr.input_conditions(name)
    v, i, ids, edge = plr.mesh(name)
    nt = i.shape[0]
    planes, want_all, cls = plr.planes(name), plr.want_rows(name), plr.want_classes(name)
    with _ctx(v, i, ids) as cd:
        for m in plr.COUNTS:
            want = plr.take_items(want_all, m)
            plr.same_rows(_rows(cd, planes[:m], f"{name} {m}", cap=want.rows.shape[0] + 64), want, f"{name}, {m} planes")
            tested = cd.planes_tested
            info = _check_counts(cd, planes[:m], cls[:m], f"{name}, {m} planes")
            if nt == 1:
                assert tested == m and info.tri_tests == m and info.node_visits == 0        # no records: every plane tests leaf 0
            else:
                assert info.node_visits >= m * -(-nt // plr.L)                              # every lane sees the root
        print(f"{name}: {want_all.rows.shape[0]} rows, {tested} plane_tri in the rows call, {info.tri_tests} in the count call, {info.node_visits} boxes")


def test_the_large_soup_gives_one_plane_two_waves_of_slabs():
    assert -(-plr.mesh(plr.SOUPS[-1])[1].shape[0] // plr.L) == 65 and plr.SOUP_SIZES[-1] == 64 * mi355cd.CD_PLANE_SLAB + 1


# ---------------------------------------------------------------- 3: the shortcut
@pytest.mark.parametrize("name", ["soup10k", "cloth100", plr.SOUPS[-1], "torus"])
def test_a_side_is_counted_without_walking_it(name):
    v, i, ids, edge = plr.mesh(name)
    nt = i.shape[0]
    used = np.asarray(v, dtype=np.float64)[i.astype(np.int64)].reshape(-1, 3)
    lo, hi = used.min(axis=0), used.max(axis=0)
    mid = 0.5 * (lo + hi)
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.3, -0.5, 0.81]])
    d = np.array([lo[2] - 1.0, hi[2] + 1.0, mid[2], float(np.array([0.3, -0.5, 0.81]) @ mid)])
    planes = mi355cd.pack_planes(nrm, d)
    with _ctx(v, i, ids) as cd:
        n_cut, n_below, n_above, info = cd.planes_count(nrm[:2], d[:2])
        assert n_above.tolist() == [nt, 0] and n_below.tolist() == [0, nt] and n_cut.tolist() == [0, 0], (n_cut, n_below, n_above)
        assert info.tri_tests == 0 and info.n_found == 0 and info.node_visits == 2 * -(-nt // plr.L)      # the root box, once a lane
        rows = cd.planes_cut_all(nrm[:2], d[:2], cap=64)
        assert rows[6] == 0 and rows[7] == OK and cd.planes_tested == 0
        for k in (2, 3):                                                    # through the mesh: most of it is counted whole
            cls = plr.classes_ref(v, i, planes[k:k + 1])
            info = _check_counts(cd, planes[k:k + 1], cls, f"{name}, plane {k}")
            want_cut = int((cls == plr.CUT).sum())
            print(f"{name} plane {k}: {want_cut} of {nt} cut, {info.tri_tests} plane_tri, {info.node_visits} boxes")
            assert want_cut <= info.tri_tests < nt and 0 < want_cut < nt, (want_cut, info.tri_tests, nt)


# ---------------------------------------------------------------- 4: closed loops from the device's rows
@pytest.mark.parametrize("name,normal,d,want_area,want_loops", plr.CLOSED_CASES)
def test_sections_of_closed_meshes_are_closed_loops(name, normal, d, want_area, want_loops):
    v, f, ids, _ = plr.mesh(name)
    plane = np.array([[*normal, d]])
    want = plr.planes_cut_all_ref(v, f, None, plane)
    with _ctx(v, f) as cd:
        got = _rows(cd, plane, name, cap=4096)
    plr.same_rows(got, want, name)
    assert plr.loops_closed(got.seg), name
    area = plr.area(got.seg, normal)
    assert area == plr.area(want.seg, normal) and (want_area is None or area == want_area), (area, want_area)
    assert want_loops is None or plr.n_loops(got.seg) == want_loops


# ---------------------------------------------------------------- 5: independence
def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def _unpermuted(w, perm):
    rows = w.rows.copy()
    rows[:, 0] = perm[rows[:, 0]]
    return plr.PlaneRows(*plr.wr.sort_rows(rows, *w[1:]))


def _check_all(cd, planes, want, cls, perm, what):
    cap = want.rows.shape[0] + 64
    plr.same_rows(_rows(cd, planes, what, cap), want, what)
    _check_counts(cd, planes, cls, what)
    plr.same_rows(_unpermuted(_rows(cd, planes[perm], what, cap), perm), want, what + ", planes permuted")
    _check_counts(cd, planes[perm], cls[perm], what + ", planes permuted")


def test_independent_of_frame_traversal_build_and_plane_order():
    name = "soup10k"
    v, i, ids, edge = plr.mesh(name)
    planes, cls = plr.planes(name, 200), plr.want_classes(name, 200)
    want = plr.want_rows(name, 200)
    perm = np.random.default_rng(4).permutation(planes.shape[0]).astype(np.uint32)
    with mi355cd.CollisionDetector(v, i) as cd:
        for frame in (mi355cd.CD_FRAME_REFERENCE, mi355cd.CD_FRAME_AUTO, mi355cd.CD_FRAME_CUSTOM):
            for trav in (0, 1, 3):
                for stagewise in (0, 1):
                    if stagewise and trav != 3:
                        continue
                    cd.set_option(mi355cd.CD_OPT_TRAVERSAL, trav)
                    cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, stagewise)
                    _frame(cd, frame)
                    cd.self_collide(cap=CAP)                               # the tree of this setting (the collision step builds it: a fused step)
                    _check_all(cd, planes, want, cls, perm, f"frame {frame} traversal {trav} stagewise {stagewise}")
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)
        cd.set_morton_frame(mi355cd.CD_FRAME_REFERENCE)
        cd.build_tree()                                                    # the staged build
        _check_all(cd, planes, want, cls, perm, "build_tree")


def test_independent_of_the_cell_table():
    name = "cloth100d"
    v, i, ids, edge = br.MESHES[name]
    planes = plr.make_planes(v, i, 64)
    cls = plr.classes_ref(v, i, planes)
    want = plr.rows_of(v, i, ids, planes, cls)
    perm = np.random.default_rng(5).permutation(planes.shape[0]).astype(np.uint32)
    with mi355cd.CollisionDetector(v, i) as cd:
        for table in (1, 0):
            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
            cd.self_collide(cap=CAP)
            _check_all(cd, planes, want, cls, perm, f"cell table {table}, fused step")
            cd.build_tree()
            _check_all(cd, planes, want, cls, perm, f"cell table {table}, build_tree")


# ---------------------------------------------------------------- 6: capacity, through the C interface
SENTINEL = 7


class _Raw:
    """A cd_planes_cut_all call through the C interface into sentinel-filled arrays of `room` rows."""

    def __init__(self, cd, room):
        r = max(room, 1)
        self.cd = cd
        self.fn = cd.lib.cd_planes_cut_all
        self.rows = np.full((r, 2), SENTINEL, dtype=np.uint32)
        self.vals = [np.full(r, SENTINEL, dtype=np.uint32), np.full((r, 2, 3), float(SENTINEL)), np.full((r, 2), SENTINEL, dtype=np.uint8),
                     np.full((r, 2), float(SENTINEL)), np.full(r, SENTINEL, dtype=np.uint8)]
        self.out = mi355cd.CdPlaneRows(*(a.ctypes.data for a in self.vals))
        self.n, self.tested = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)

    def call(self, items, cap, n=None, null=False):
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        n = items.shape[0] if n is None else n
        return self.fn(self.cd._ctx, vp(items), n, None if null else vp(self.rows), cap, C.byref(self.n), C.byref(self.tested), None if null else C.byref(self.out))

    def untouched_from(self, at):
        return all((a[at:] == SENTINEL).all() for a in [self.rows] + self.vals)

    def nothing_written(self):
        return self.untouched_from(0) and self.n.value == SENTINEL and self.tested.value == SENTINEL

    def written(self, count):
        return (self.rows[:count],) + tuple(a[:count] for a in self.vals)


def _distinct_members(got, want, what):
    """got's rows are distinct rows of want's set, with want's values."""
    g = plr.wr.sort_rows(*got)
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(32)) | r[:, 1].astype(np.uint64)
    kg, kw = key(g[0]), key(want.rows)
    assert np.unique(kg).size == kg.size, what
    at = np.minimum(np.searchsorted(kw, kg), kw.size - 1)
    assert np.array_equal(kw[at], kg), what
    plr.same_rows(g, plr.PlaneRows(*(a[at] for a in want)), what)


def test_overflow():
    name = "soup10k"
    v, i, ids, edge = plr.mesh(name)
    items, want = plr.planes(name, 64), plr.want_rows(name, 64)
    empty = items.copy(); empty[:, :3] = (0.0, 0.0, 1.0); empty[:, 3] = 100.0                      # far above the mesh: no rows
    total = want.rows.shape[0]
    assert total > 64
    with _ctx(v, i, ids) as cd:
        r = _Raw(cd, 0)                                                                             # the count-only call
        assert r.call(items, 0, null=True) == OVERFLOW and r.n.value == total and r.tested.value >= total
        assert r.call(empty, 0, null=True) == OK and r.n.value == 0
        r = _Raw(cd, total + 64)                                                                    # one row short
        assert r.call(items, total - 1) == OVERFLOW and r.n.value == total
        assert r.untouched_from(total - 1), "written at or past cap_rows"
        _distinct_members(r.written(total - 1), want, "cap = n_rows - 1")
        r = _Raw(cd, total + 64)                                                                    # a small prefix
        assert r.call(items, 65) == OVERFLOW and r.n.value == total and r.untouched_from(65)
        _distinct_members(r.written(65), want, "cap = 65")
        r = _Raw(cd, total + 64)                                                                    # exactly enough
        assert r.call(items, total) == OK and r.n.value == total and r.untouched_from(total)
        plr.same_rows(r.written(total), want, "cap = n_rows")
        r = _Raw(cd, total)                                                                         # rows only: out and n_tested NULL
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert r.fn(cd._ctx, vp(items), items.shape[0], vp(r.rows), total, C.byref(r.n), None, None) == OK
        assert np.array_equal(plr.wr.sort_rows(r.rows)[0], want.rows) and all((a == SENTINEL).all() for a in r.vals)


def test_candidate_buffer_grows_and_one_plane_calls_straddle_the_growth():
    """A soup whose every face straddles z = 1/2, and 700 planes z = d near it that cut every face: more candidates than the first
    allocation of the shards holds, whichever shard they go to."""
    nt = 2049
    v, i = si.box_soup(nt, 0.2, 0.0, 1.0, 7)
    v = v.copy()
    v[0::3, 2] = 0.25 * v[0::3, 2]                                          # every face's first vertex below 0.3, the others above 0.7
    v[1::3, 2] = 0.75 + 0.25 * v[1::3, 2]
    v[2::3, 2] = 0.75 + 0.25 * v[2::3, 2]
    m = 700
    assert m * nt > mi355cd.WITHIN_SHARD_FIRST * mi355cd.WITHIN_SHARDS
    big = mi355cd.pack_planes(np.tile([0.0, 0.0, 1.0], (m, 1)), np.linspace(0.4, 0.6, m))
    one_plane = np.array([[0.3, -0.5, 0.81, 0.25]])
    one = plr.planes_cut_all_ref(v, i, None, one_plane)
    assert 1 < one.rows.shape[0] < nt
    with _ctx(v, i) as cd:
        plr.same_rows(_rows(cd, one_plane, "one plane"), one, "one plane")
        got = cd.planes_cut_all(big[:, :3], big[:, 3], cap=m * nt)
        rows, n, rc = got[0], got[6], got[7]
        assert rc == OK and n == m * nt == rows.shape[0] and cd.planes_tested == m * nt, (rc, n, cd.planes_tested)
        key = np.sort(rows[:, 0].astype(np.int64) * nt + rows[:, 1])
        assert np.array_equal(key, np.arange(m * nt))                                               # every (plane, face) once
        assert np.array_equal(got[1], rows[:, 1])                                                   # the IDs: the face indices
        plr.same_rows(_rows(cd, one_plane, "one plane again"), one, "one plane again")
        n_cut, n_below, n_above, info = cd.planes_count(big[:, :3], big[:, 3])
        assert (n_cut == nt).all() and not n_below.any() and not n_above.any() and info.n_found == m


# ---------------------------------------------------------------- 7: the context, and errors
def test_leaves_the_context_as_it_was_and_errors_write_nothing():
    name = "soup10k"
    v, i, ids, edge = plr.mesh(name)
    planes, want, cls = plr.planes(name, 64), plr.want_rows(name, 64), plr.want_classes(name, 64)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    boxes = br.boxes(name)[:64]
    want_boxes = br.boxes_overlap_all_ref(v, i, ids, boxes)
    box_rows = lambda cd: br.BoxRows(*br.wr.sort_rows(*cd.boxes_overlap_all(boxes[:, 0::2], boxes[:, 1::2], cap=CAP)[:3]))

    def count_raw(cd, items, n=None):
        counts = [np.full(64, SENTINEL, dtype=np.uint32) for _ in range(3)]
        info = mi355cd.CdPlaneInfo(5, 5, 5)
        rc = cd.lib.cd_planes_count(cd._ctx, vp(items), items.shape[0] if n is None else n, *map(vp, counts), C.byref(info))
        clean = all((c == SENTINEL).all() for c in counts) and (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)
        return rc, clean

    with mi355cd.CollisionDetector(v, i) as cd:
        r = _Raw(cd, 256)                                                   # before a build
        assert r.call(planes, 256) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        assert count_raw(cd, planes) == (mi355cd.CD_ERR_ORDER, True)
        cd.self_collide(cap=CAP)
        before = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(), box_rows(cd))
        br.same_rows(before[2], want_boxes, "the box query before")
        plr.same_rows(_rows(cd, planes, name), want, name)
        _check_counts(cd, planes, cls, name)
        assert bytes(cd.stats()) == before[0]
        assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == before[1]
        br.same_rows(box_rows(cd), want_boxes, "the box query after")
        plr.same_rows(_rows(cd, planes, name), want, name + ", after the box query")

        for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (3, np.inf), (None, 0.0), (None, -0.0)):   # not finite; n = (0, 0, 0)
            x = planes.copy()
            if col is None:
                x[63, :3] = val                                            # the LAST plane: nothing may have been launched for the others
            else:
                x[63, col] = val
            r = _Raw(cd, 256)
            assert r.call(x, 256) == mi355cd.CD_ERR_ARG and r.nothing_written(), (col, val)
            assert count_raw(cd, x) == (mi355cd.CD_ERR_ARG, True), (col, val)
        r = _Raw(cd, 256)
        assert r.call(planes, 256, n=1 << 32) == mi355cd.CD_ERR_ARG and r.nothing_written()                             # (checked before the planes are read)
        assert r.fn(cd._ctx, None, 64, vp(r.rows), 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG                # NULL planes
        assert r.fn(cd._ctx, vp(planes), 64, None, 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG                # NULL rows with room asked for
        assert r.fn(cd._ctx, vp(planes), 64, vp(r.rows), 256, None, None, None) == mi355cd.CD_ERR_ARG and r.nothing_written()   # NULL n_rows
        assert r.call(planes, 256, n=0) == OK and r.n.value == 0 and r.untouched_from(0)                               # n = 0
        assert cd.lib.cd_planes_count(cd._ctx, vp(planes), 64, None, None, None, None) == mi355cd.CD_ERR_ARG           # NULL n_cut
        assert cd.lib.cd_planes_count(cd._ctx, None, 64, vp(np.zeros(64, dtype=np.uint32)), None, None, None) == mi355cd.CD_ERR_ARG
        assert count_raw(cd, planes, n=0)[0] == OK
        only_cut = np.full(64, SENTINEL, dtype=np.uint32)                   # the last two arrays and info may be NULL
        assert cd.lib.cd_planes_count(cd._ctx, vp(planes), 64, vp(only_cut), None, None, None) == OK
        assert np.array_equal(only_cut, plr.counts_of_classes(cls)[0])


def test_a_mesh_that_moves():
    s = mov.seq("jitter")
    planes0, planes1 = plr.make_planes(s.frames[0], s.vidx, 64), plr.make_planes(s.frames[1], s.vidx, 64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    with _ctx(s.frames[0], s.vidx) as cd:
        want0 = plr.planes_cut_all_ref(s.frames[0], s.vidx, None, planes0)
        plr.same_rows(_rows(cd, planes0, "frame 0"), want0, "frame 0")
        cd.update_vertices(s.frames[1])
        r = _Raw(cd, 256)                                                  # after update_vertices without a rebuild
        assert r.call(planes1, 256) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        counts = [np.full(64, SENTINEL, dtype=np.uint32) for _ in range(3)]
        assert cd.lib.cd_planes_count(cd._ctx, vp(planes1), 64, *map(vp, counts), None) == mi355cd.CD_ERR_ORDER and all((c == SENTINEL).all() for c in counts)
        cd.build_tree()
        cls1 = plr.classes_ref(s.frames[1], s.vidx, planes1)
        want1 = plr.rows_of(s.frames[1], s.vidx, None, planes1, cls1)
        same_planes = plr.planes_cut_all_ref(s.frames[1], s.vidx, None, planes0)
        assert same_planes.rows.shape != want0.rows.shape or not np.array_equal(same_planes.seg, want0.seg)             # the answer did change
        plr.same_rows(_rows(cd, planes1, "frame 1"), want1, "after update_vertices and a rebuild")
        plr.same_rows(_rows(cd, planes0, "frame 1, the planes of frame 0"), same_planes, "the rows follow the new vertices")
        _check_counts(cd, planes1, cls1, "after update_vertices and a rebuild")


# ---------------------------------------------------------------- 8: the fp32 range ends of the filter
@functools.lru_cache(maxsize=None)
def _scale_case(name):
    v, vidx, edge = si.meshes()[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    planes = plr.make_planes(vv, vidx, 128, seed=3)
    cls = plr.classes_ref(vv, vidx, planes)
    return vv, vidx, planes, cls, plr.rows_of(vv, vidx, None, planes, cls)


@pytest.mark.parametrize("k", (-300, -150, -126, 127, 128, 149, 300))
@pytest.mark.parametrize("name", ["dense", "centred"])
def test_fp32_range(name, k):
    """Mesh and d scaled by 2^k, past both fp32 ends (where the stored boxes hold +-inf, 0 and subnormals): the k = 0 rows with a and
    b scaled, and the k = 0 counts."""
    vv, vidx, planes, cls, want = _scale_case(name)
    pk = planes.copy()
    pk[:, 3] = si.scaled(pk[:, 3], k)
    with _ctx(si.scaled(vv, k), vidx) as cd:
        plr.same_rows(_rows(cd, pk, name), want._replace(seg=si.scaled(want.seg, k)), f"{name} 2^{k}")
        _check_counts(cd, pk, cls, f"{name} 2^{k}")


# ---------------------------------------------------------------- 9: the use
def test_slice_a_torus_into_layers():
    """What the query is for: a torus around z sliced by 32 parallel planes x = c.  Between the hole's edge and the outer rim a layer
    is one loop, through the hole it is two; the layer areas are the restatement's."""
    v, f = cm.torus()
    c = -1.24 + 0.08 * np.arange(32)
    two = np.abs(c) < 0.6197 - 0.015                                        # the faceted hole: between (R - r) cos(pi / 24) and R - r
    assert (two | (np.abs(c) > 0.625 + 0.015)).all() and (np.abs(c) < 1.36).all() and two.sum() == 16
    nrm = np.tile([1.0, 0.0, 0.0], (32, 1))
    planes = mi355cd.pack_planes(nrm, c)
    want = plr.planes_cut_all_ref(v, f, None, planes)
    with _ctx(v, f) as cd:
        got = _rows(cd, planes, "layers")
        n_cut, n_below, n_above, info = cd.planes_count(nrm, c)
    plr.same_rows(got, want, "layers")
    areas = []
    for k in range(32):
        mine = got.rows[:, 0] == k
        assert plr.loops_closed(got.seg[mine]) and mine.sum() == n_cut[k], k
        assert plr.n_loops(got.seg[mine]) == (2 if two[k] else 1), (k, c[k])
        areas.append(plr.area(got.seg[mine], nrm[k]))
        assert areas[-1] == plr.area(want.seg[want.rows[:, 0] == k], nrm[k]) and areas[-1] > 0.0
    assert (np.diff(n_below.astype(np.int64)) >= 0).all() and n_below[0] < n_below[-1]          # more of the torus lies below each next layer
    print("layer areas", np.round(areas, 4).tolist())
