"""The box queries on the device (cd_boxes_overlap_all, cd_boxes_count, cd_box_tri_points) against the restatements of
tests/box_ref.py -- all pairs, no box filter of any kind -- as sets of (item, face) and in every value of a row, and against each
other through the definitions that link them.  Every step has bounded size."""
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
import proximity_ref as pr
import scale_inputs as si

pytestmark = pytest.mark.gpu

CAP = 1 << 20
OK, OVERFLOW = mi355cd.CD_OK, mi355cd.CD_OVERFLOW


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _lo_hi(boxes):
    return boxes[:, 0::2], boxes[:, 1::2]


def _rows(cd, boxes, what, cap=CAP):
    """boxes_overlap_all's rows as a BoxRows sorted by (item, face); the call fitted its capacity."""
    got = cd.boxes_overlap_all(*_lo_hi(boxes), cap=cap)
    assert got[4] == OK and got[3] == got[0].shape[0] and cd.boxes_tested >= got[3], (what, got[3:], cd.boxes_tested)
    return br.BoxRows(*br.wr.sort_rows(*got[:3]))


def _check_counts(cd, boxes, want: br.BoxRows, what):
    """boxes_count against the per-item sums of `want`, plain and ANY.  -> the plain call's info"""
    n = boxes.shape[0]
    c, ci = br.counts_of(want, n)
    count, n_inside, info = cd.boxes_count(*_lo_hi(boxes))
    assert np.array_equal(count, c) and np.array_equal(n_inside, ci), (what, np.nonzero(count != c)[0][:4], np.nonzero(n_inside != ci)[0][:4])
    assert info.n_found == (c > 0).sum() and (info.node_visits >= n or (info.node_visits == 0 and info.tri_tests == n)), what   # (one triangle: no records)
    found, none, info_any = cd.boxes_count(*_lo_hi(boxes), any=True)
    assert none is None and np.array_equal(found, (c > 0).astype(np.uint32)) and info_any.n_found == info.n_found, what
    assert info_any.tri_tests <= info.tri_tests and info_any.node_visits <= info.node_visits, what
    return info


# ---------------------------------------------------------------- 1: the pin, and the values
def test_box_tri_points_is_the_restatement_bit_for_bit():
    for what, (boxes, tris) in (("integer", br.integer_family()), ("unit cube", br.random_family(0.0)), ("offset", br.random_family(br.OFFSET)),
                                ("near touching", br.near_touching_family())):
        want = br.box_tri_np(boxes, tris)
        got = mi355cd.box_tri_points(boxes, tris)
        for name, a, b in zip(("hit", "inside", "code"), got, want):
            assert np.array_equal(a, b), (what, name, np.nonzero(a != b)[0][:8])
        print(f"{what}: {boxes.shape[0]} cases, {int(want[0].sum())} hits, {int(want[1].sum())} inside, codes {np.bincount(want[2], minlength=14).tolist()}")
    hit, inside, code = br.box_tri_np(*br.near_touching_family())
    assert 10_000 < hit.sum() < 90_000 and (hit & ~inside).sum() > 10_000


@pytest.mark.parametrize("name", br.NAMES)
def test_rows_and_counts_are_the_restatements(name):
    """At 1, 63, 64, 65 and 1000 items: the restatement's set of (item, face) with its IDs and inside; count and n_inside are its
    per-item sums (so the rows grouped by item are boxes_count's answer); ANY is count > 0."""
    br.input_conditions(name)
    v, i, ids, edge = br.MESHES[name]
    boxes, want_all = br.boxes(name), br.want_rows(name)
    with _ctx(v, i, ids) as cd:
        for m in br.COUNTS:
            want = br.take_items(want_all, m)
            br.same_rows(_rows(cd, boxes[:m], f"{name} {m}"), want, f"{name}, {m} items")
            tested = cd.boxes_tested
            info = _check_counts(cd, boxes[:m], want, f"{name}, {m} items")
            if i.shape[0] == 1:
                assert tested == m and info.tri_tests == m and info.node_visits == 0         # no records: every box tests leaf 0
        print(f"{name}: {want_all.rows.shape[0]} rows, {int(want_all.inside.sum())} inside, {tested} box_tri in the rows call, {info.tri_tests} in the count call")


# ---------------------------------------------------------------- 2: the definitions that link the calls
@pytest.mark.parametrize("name", br.NAMES)
def test_root_box_counts_every_triangle_without_a_test(name):
    """cd_root_box's output is a valid item: count == n_inside == nt, and on a tree with records no box_tri runs for it -- the lane
    sees the tree inside the box and adds its leaves (this fails if contained subtrees are walked)."""
    v, i, ids, edge = br.MESHES[name]
    nt = i.shape[0]
    with _ctx(v, i, ids) as cd:
        root = cd.root_box().reshape(1, 6)
        assert np.array_equal(root[0], br.root_box(v, i))
        count, n_inside, info = cd.boxes_count(*_lo_hi(root))
        assert count[0] == nt == n_inside[0] and info.n_found == 1, (count, n_inside)
        assert info.tri_tests == (0 if nt > 1 else 1), info.tri_tests
        found, _, info = cd.boxes_count(*_lo_hi(root), any=True)
        assert found[0] == 1 and info.tri_tests == (0 if nt > 1 else 1)
        rows = _rows(cd, root, name)
        assert np.array_equal(rows.rows, np.stack([np.zeros(nt, dtype=np.uint32), np.arange(nt, dtype=np.uint32)], axis=1)) and rows.inside.all()
        # a box that holds all but the outermost vertices: most subtrees are counted whole, the rest is tested
        shrunk = root.copy()
        shrunk[0, 0::2] += 0.25 * np.minimum(edge, root[0, 1::2] - root[0, 0::2])
        want = br.boxes_overlap_all_ref(v, i, ids, shrunk)
        info = _check_counts(cd, shrunk, want, f"{name}, shrunk root box")
        br.same_rows(_rows(cd, shrunk, name), want, f"{name}, shrunk root box")
        if nt >= 5000:
            assert 2 * info.tri_tests < cd.boxes_tested, (info.tri_tests, want.rows.shape[0], cd.boxes_tested)


@pytest.mark.parametrize("name", ["soup10k", "cloth100", "duplicates"])
def test_point_box_on_a_vertex_returns_the_faces_around_it(name):
    v, i, ids, edge = br.MESHES[name]
    p = np.asarray(v, dtype=np.float64)[i.astype(np.int64)]                                  # [T, 3, 3]
    g = np.random.default_rng(8)
    at = p.reshape(-1, 3)[g.integers(0, 3 * i.shape[0], 200)]
    boxes = mi355cd.pack_boxes(at, at)
    want = br.boxes_overlap_all_ref(v, i, ids, boxes)
    with _ctx(v, i, ids) as cd:
        rows = _rows(cd, boxes, name)
        br.same_rows(rows, want, f"{name}, point boxes")
        _check_counts(cd, boxes, want, f"{name}, point boxes")
    most = 0
    for k in range(boxes.shape[0]):
        around = np.nonzero((p == at[k]).all(axis=2).any(axis=1))[0]
        mine = rows.rows[rows.rows[:, 0] == k, 1]
        assert around.size >= 1 and np.isin(around, mine).all(), (k, around, mine)
        most = max(most, around.size)
    assert most >= (6 if name == "cloth100" else 1)                                          # six faces share a vertex of the sheet
    assert not rows.inside[np.isin(rows.rows[:, 1], np.nonzero((p != p[:, :1]).any(axis=(1, 2)))[0])].any()   # a point holds no proper triangle


# ---------------------------------------------------------------- 3: independence
def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def _unpermuted(w, perm):
    rows = w.rows.copy()
    rows[:, 0] = perm[rows[:, 0]]
    return br.BoxRows(*br.wr.sort_rows(rows, *w[1:]))


def _check_all(cd, boxes, want, perm, what):
    br.same_rows(_rows(cd, boxes, what), want, what)
    _check_counts(cd, boxes, want, what)
    br.same_rows(_unpermuted(_rows(cd, boxes[perm], what), perm), want, what + ", boxes permuted")
    count, n_inside, _ = cd.boxes_count(*_lo_hi(boxes[perm]))
    c, ci = br.counts_of(want, boxes.shape[0])
    assert np.array_equal(count, c[perm]) and np.array_equal(n_inside, ci[perm]), what + ", boxes permuted"


def test_independent_of_frame_traversal_build_and_item_order():
    name = "soup10k"
    v, i, ids, edge = br.MESHES[name]
    boxes, want = br.boxes(name), br.want_rows(name)
    perm = np.random.default_rng(4).permutation(boxes.shape[0]).astype(np.uint32)
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
                    _check_all(cd, boxes, want, perm, f"frame {frame} traversal {trav} stagewise {stagewise}")
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)
        cd.set_morton_frame(mi355cd.CD_FRAME_REFERENCE)
        cd.build_tree()                                                    # the staged build
        _check_all(cd, boxes, want, perm, "build_tree")


def test_independent_of_the_cell_table():
    name = "cloth100d"
    v, i, ids, edge = br.MESHES[name]
    boxes = br.make_boxes(v, i, edge, 256)
    want = br.boxes_overlap_all_ref(v, i, ids, boxes)
    perm = np.random.default_rng(5).permutation(boxes.shape[0]).astype(np.uint32)
    with mi355cd.CollisionDetector(v, i) as cd:
        for table in (1, 0):
            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
            cd.self_collide(cap=CAP)
            _check_all(cd, boxes, want, perm, f"cell table {table}, fused step")
            cd.build_tree()
            _check_all(cd, boxes, want, perm, f"cell table {table}, build_tree")


# ---------------------------------------------------------------- 4: capacity, through the C interface
SENTINEL = 7


class _Raw:
    """A cd_boxes_overlap_all call through the C interface into sentinel-filled arrays of `room` rows."""

    def __init__(self, cd, room):
        self.cd = cd
        self.fn = cd.lib.cd_boxes_overlap_all
        self.rows = np.full((max(room, 1), 2), SENTINEL, dtype=np.uint32)
        self.vals = [np.full(max(room, 1), SENTINEL, dtype=np.uint32), np.full(max(room, 1), SENTINEL, dtype=np.uint8)]
        self.out = mi355cd.CdBoxRows(*(a.ctypes.data for a in self.vals))
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
        return (self.rows[:count], self.vals[0][:count], self.vals[1][:count].astype(bool))


def _distinct_members(got, want, what):
    """got's rows are distinct rows of want's set, with want's values."""
    g = br.wr.sort_rows(*got)
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(32)) | r[:, 1].astype(np.uint64)
    kg, kw = key(g[0]), key(want.rows)
    assert np.unique(kg).size == kg.size, what
    at = np.minimum(np.searchsorted(kw, kg), kw.size - 1)
    assert np.array_equal(kw[at], kg), what
    br.same_rows(g, br.BoxRows(*(a[at] for a in want)), what)


def test_overflow():
    name = "soup10k"
    v, i, ids, edge = br.MESHES[name]
    items, want = br.boxes(name), br.want_rows(name)
    empty = items.copy(); empty += 100.0                                                            # far from the mesh: no rows
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
        br.same_rows(r.written(total), want, "cap = n_rows")
        r = _Raw(cd, total)                                                                         # rows only: out and n_tested NULL
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert r.fn(cd._ctx, vp(items), items.shape[0], vp(r.rows), total, C.byref(r.n), None, None) == OK
        assert np.array_equal(br.wr.sort_rows(r.rows)[0], want.rows) and all((a == SENTINEL).all() for a in r.vals)


def test_candidate_buffer_grows_and_one_box_calls_straddle_the_growth():
    name = "soup10k"
    v, i, ids, edge = br.MESHES[name]
    nt = i.shape[0]
    root = br.root_box(v, i)
    big = np.ascontiguousarray(np.tile(root, (130, 1)))
    assert 130 * nt > mi355cd.WITHIN_SHARD_FIRST * mi355cd.WITHIN_SHARDS                             # more than the first allocation holds
    one_box = br.boxes(name)[2:3]                                                                   # three edges around a vertex
    one = br.boxes_overlap_all_ref(v, i, ids, one_box)
    assert one.rows.shape[0] > 1
    with _ctx(v, i, ids) as cd:
        br.same_rows(_rows(cd, one_box, "one box"), one, "one box")
        rows, oid, inside, n, rc = cd.boxes_overlap_all(*_lo_hi(big), cap=130 * nt)
        assert rc == OK and n == 130 * nt == rows.shape[0] and cd.boxes_tested == 130 * nt, (rc, n, cd.boxes_tested)
        assert inside.all()
        key = np.sort(rows[:, 0].astype(np.int64) * nt + rows[:, 1])
        assert np.array_equal(key, np.arange(130 * nt))                                             # every (item, face) once
        assert np.array_equal(oid, (np.arange(nt, dtype=np.uint32) if ids is None else ids)[rows[:, 1]])
        br.same_rows(_rows(cd, one_box, "one box again"), one, "one box again")
        br.same_rows(_rows(cd, br.boxes(name), "all boxes"), br.want_rows(name), "all boxes after the growth")
        count, n_inside, info = cd.boxes_count(*_lo_hi(big))
        assert (count == nt).all() and (n_inside == nt).all() and info.tri_tests == 0


# ---------------------------------------------------------------- 5: the context, and errors
def test_leaves_the_context_as_it_was_and_errors_write_nothing():
    name = "soup10k"
    v, i, ids, edge = br.MESHES[name]
    boxes, want = br.boxes(name), br.want_rows(name)
    b64 = np.ascontiguousarray(boxes[:64])
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def count_raw(cd, items, flags=0, n=None, with_inside=True):
        count, n_inside = np.full(64, SENTINEL, dtype=np.uint32), np.full(64, SENTINEL, dtype=np.uint32)
        info = mi355cd.CdBoxInfo(5, 5, 5)
        rc = cd.lib.cd_boxes_count(cd._ctx, vp(items), items.shape[0] if n is None else n, flags, vp(count), vp(n_inside) if with_inside else None, C.byref(info))
        clean = (count == SENTINEL).all() and (n_inside == SENTINEL).all() and (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)
        return rc, clean

    with mi355cd.CollisionDetector(v, i) as cd:
        r = _Raw(cd, 256)                                                   # before a build
        assert r.call(b64, 256) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        assert count_raw(cd, b64) == (mi355cd.CD_ERR_ORDER, True)
        for flags, with_inside in ((2, False), (-1, False), (3, False), (mi355cd.CD_BOX_ANY, True)):       # the flag rules come first
            assert count_raw(cd, b64, flags, with_inside=with_inside) == (mi355cd.CD_ERR_ARG, True), flags
        cd.self_collide(cap=CAP)
        before = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(), cd.find_proximity(0.004, cap=CAP))
        br.same_rows(_rows(cd, boxes, name), want, name)
        _check_counts(cd, boxes, want, name)
        assert bytes(cd.stats()) == before[0]
        assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == before[1]
        gp, gd = pr.sort_pairs(*cd.find_proximity(0.004, cap=CAP)[:2])
        wp, wd = pr.sort_pairs(*before[2][:2])
        assert gp.shape[0] > 0 and np.array_equal(gp, wp) and np.array_equal(gd.view(np.uint64), wd.view(np.uint64))
        br.same_rows(_rows(cd, boxes, name), want, name + ", after proximity")

        for col, val in ((0, np.nan), (1, np.nan), (2, np.inf), (3, np.inf), (4, -np.inf), (5, np.nan), (0, 1e9), (3, -1e9), (5, -1e9)):   # NaN, inf, lo > hi
            x = b64.copy(); x[63, col] = val                               # the LAST item: nothing may have been launched for the others
            r = _Raw(cd, 256)
            assert r.call(x, 256) == mi355cd.CD_ERR_ARG and r.nothing_written(), (col, val)
            assert count_raw(cd, x) == (mi355cd.CD_ERR_ARG, True), (col, val)
            assert count_raw(cd, x, mi355cd.CD_BOX_ANY, with_inside=False) == (mi355cd.CD_ERR_ARG, True), (col, val)
        r = _Raw(cd, 256)
        assert r.call(b64, 256, n=1 << 32) == mi355cd.CD_ERR_ARG and r.nothing_written()                                # (checked before the boxes are read)
        assert r.fn(cd._ctx, None, 64, vp(r.rows), 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG                # NULL items
        assert r.fn(cd._ctx, vp(b64), 64, None, 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG                   # NULL rows with room asked for
        assert r.fn(cd._ctx, vp(b64), 64, vp(r.rows), 256, None, None, None) == mi355cd.CD_ERR_ARG and r.nothing_written()   # NULL n_rows
        assert r.call(b64, 256, n=0) == OK and r.n.value == 0 and r.untouched_from(0)                                  # n = 0
        assert cd.lib.cd_boxes_count(cd._ctx, vp(b64), 64, 0, None, None, None) == mi355cd.CD_ERR_ARG                  # NULL count
        assert cd.lib.cd_boxes_count(cd._ctx, None, 64, 0, vp(np.zeros(64, dtype=np.uint32)), None, None) == mi355cd.CD_ERR_ARG
        assert count_raw(cd, b64, n=0)[0] == OK
        flat = b64.copy(); flat[:, 1::2] = flat[:, 0::2]                   # lo == hi is a value, not an error
        assert _Raw(cd, 256).call(flat, 256) == OK

    s = mov.seq("jitter")
    boxes0, boxes1 = br.make_boxes(s.frames[0], s.vidx, s.edge, 256), br.make_boxes(s.frames[1], s.vidx, s.edge, 256)
    with _ctx(s.frames[0], s.vidx) as cd:
        want0 = br.boxes_overlap_all_ref(s.frames[0], s.vidx, None, boxes0)
        br.same_rows(_rows(cd, boxes0, "frame 0"), want0, "frame 0")
        cd.update_vertices(s.frames[1])
        r = _Raw(cd, 256)                                                  # after update_vertices without a rebuild
        assert r.call(np.ascontiguousarray(boxes1[:64]), 256) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        assert count_raw(cd, np.ascontiguousarray(boxes1[:64])) == (mi355cd.CD_ERR_ORDER, True)
        cd.build_tree()
        want1 = br.boxes_overlap_all_ref(s.frames[1], s.vidx, None, boxes1)
        assert want1.rows.shape != want0.rows.shape or not np.array_equal(want1.rows, want0.rows)                      # the answer did change
        br.same_rows(_rows(cd, boxes1, "frame 1"), want1, "after update_vertices and a rebuild")
        _check_counts(cd, boxes1, want1, "after update_vertices and a rebuild")
        assert cd.boxes_count(*_lo_hi(cd.root_box().reshape(1, 6)))[0][0] == s.nt


# ---------------------------------------------------------------- 6: the fp32 range ends, and a translated mesh
SCALE_MESHES = si.meshes()
NSCALE = 512
BAND = tuple(k for k in si.SCALES if abs(k) <= 300) + (-300, 300)             # box_tri's band (csrc/cd_math.h): ray_tri's


@functools.lru_cache(maxsize=None)
def _scale_case(name):
    v, vidx, edge = SCALE_MESHES[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    boxes = br.make_boxes(vv, vidx, edge, NSCALE, seed=3)
    return vv, vidx, boxes, br.boxes_overlap_all_ref(vv, vidx, None, boxes)


@pytest.mark.parametrize("k", BAND)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """Mesh and boxes scaled by 2^k, past both fp32 ends: the k = 0 rows, IDs, inside and counts."""
    vv, vidx, boxes, want = _scale_case(name)
    c, ci = br.counts_of(want, NSCALE)
    assert (c == 0).sum() >= NSCALE // 8 and (c >= 2).sum() >= NSCALE // 8 and c[br.ROOT_AT] == vidx.shape[0] and 0 < ci.sum() < c.sum()
    bs = si.scaled(boxes, k)
    with _ctx(si.scaled(vv, k), vidx) as cd:
        br.same_rows(_rows(cd, bs, name), want, f"{name} 2^{k}")
        _check_counts(cd, bs, want, f"{name} 2^{k}")
    if k in si.EDGES and k != 0:
        br.same_rows(want, br.boxes_overlap_all_ref(si.scaled(vv, k), vidx, None, bs), f"{name} 2^{k}, the restatement on the scaled inputs")


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_mesh_gives_the_restatement(name):
    vv, vidx, _, _ = _scale_case(name)
    edge = SCALE_MESHES[name][2]
    vt = vv + (2.0 ** 20 + 0.37)
    boxes = br.make_boxes(vt, vidx, edge, NSCALE, seed=5)
    want = br.boxes_overlap_all_ref(vt, vidx, None, boxes)
    c, _ = br.counts_of(want, NSCALE)
    print(f"{name} translated: {want.rows.shape[0]} rows, {int((c == 0).sum())} of {NSCALE} boxes with none, {int((c >= 2).sum())} with several")
    assert (c == 0).sum() >= NSCALE // 8 and (c >= 2).sum() >= NSCALE // 8
    with _ctx(vt, vidx) as cd:
        br.same_rows(_rows(cd, boxes, name), want, f"{name} translated")
        _check_counts(cd, boxes, want, f"{name} translated")


# ---------------------------------------------------------------- 7: the use
def test_voxelise_a_closed_mesh():
    """What the query is for: a torus on a 16^3 grid, one box a voxel.  The occupied set and the per-voxel counts are the
    restatement's; a face in a voxel's wall belongs to both voxels."""
    v, f = cm.torus()
    m = 16
    lo, hi = v.min(axis=0) - 0.01, v.max(axis=0) + 0.01
    g = np.stack(np.meshgrid(*(np.arange(m),) * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    vlo = lo + (hi - lo) * (g / m)
    vhi = lo + (hi - lo) * ((g + 1) / m)
    boxes = mi355cd.pack_boxes(vlo, vhi)
    want_count, want_inside = br.boxes_count_ref(v, f, boxes)
    with _ctx(v, f) as cd:
        occupied, _, info_any = cd.boxes_count(vlo, vhi, any=True)
        count, n_inside, info = cd.boxes_count(vlo, vhi)
        rows = _rows(cd, boxes, "voxels")
    assert np.array_equal(count, want_count) and np.array_equal(n_inside, want_inside)
    assert np.array_equal(occupied.astype(bool), want_count > 0)
    c, ci = br.counts_of(rows, m ** 3)
    assert np.array_equal(c, want_count) and np.array_equal(ci, want_inside)
    print(f"torus, {f.shape[0]} faces on {m}^3 voxels: {int(occupied.sum())} occupied, {int(count.sum())} rows, {info.tri_tests} box_tri (ANY: {info_any.tri_tests})")
    assert 100 < occupied.sum() < m ** 3 - 100 and count.sum() > f.shape[0] and info_any.tri_tests < info.tri_tests
