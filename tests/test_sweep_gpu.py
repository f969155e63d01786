"""The swept-point queries on the device (cd_pt_advance_points, cd_sweep_points_all, cd_sweep_points) against the restatement of
tests/sweep_ref.py -- which uses no tree and no box filter beyond the gate -- as sets of (item, face) and bit for bit in every value of
a row, and against the device's own point and ray queries.  Every step has bounded size."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import mi355_synth as synth
import mi355cd
import oracle
import point_ref as ptr
import scale_inputs as si
import sweep_ref as sr
import within_ref as wr

pytestmark = pytest.mark.gpu

CAP = 1 << 20
NAMES = wr.SMALL + ["cloth100"]
OK, OVERFLOW = mi355cd.CD_OK, mi355cd.CD_OVERFLOW


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _sweep(cd, it, x1, what, skip=None, cap=CAP):
    """sweep_points_all's rows as a SweepRows sorted by (item, face); the call fitted its capacity."""
    got = cd.sweep_points_all(it[:, 0:3], it[:, 3:6], it[:, 6], verts_end=x1, skip_vertex=skip, cap=cap)
    assert got[9] == OK and got[8] == got[0].shape[0], (what, got[8:])
    info = cd.sweep_info
    assert info.n_candidates >= info.n_tested >= got[8] and info.n_evals >= info.n_tested, what
    return sr.SweepRows(*wr.sort_rows(*got[:8]))


def _same_tuple(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        if b.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        assert np.array_equal(a, b), (what, k)


def _counts(cd):
    return (cd.sweep_info.n_tested, cd.sweep_info.n_evals, cd.sweep_info.n_unresolved)


# ---------------------------------------------------------------- 1: the pin
@functools.lru_cache(maxsize=None)
def _pin():
    inputs = sr.pin_inputs(5800, seed=1)                                       # 10 classes of 5800 and 2 of 725: 59 450 pairs
    it, t = np.concatenate([v[0] for v in inputs.values()]), np.concatenate([v[1] for v in inputs.values()])
    o = np.random.default_rng(2).permutation(it.shape[0])                      # (the classes mixed: every wave meets every branch)
    it, t = np.ascontiguousarray(it[o]), np.ascontiguousarray(t[o])
    return it, t, sr.pt_advance_np(it, t)


def test_pt_advance_is_the_restatement_bit_for_bit():
    it, t, want = _pin()
    sr.pin_conditions(it, t, want)
    _same_tuple(mi355cd.pt_advance_points(it, t), want, "pin")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_pt_advance_grid_edge(n):
    it, t, want = _pin()
    _same_tuple(mi355cd.pt_advance_points(it[:n], t[:n]), type(want)(*(a[:n] for a in want)), f"pin, n = {n}")


# ---------------------------------------------------------------- 2: the row sets
@functools.lru_cache(maxsize=None)
def _case(name):
    """Items wr.points(name) moved by about an edge, x1 a jittered copy of the vertices, dist a quarter edge; the restatement's rows."""
    v, i, ids, edge = wr.MESHES[name]
    v = np.asarray(v, dtype=np.float64)
    g = np.random.default_rng(11)
    p0 = wr.points(name)
    it = mi355cd.pack_sweeps(p0, p0 + g.normal(size=p0.shape) * 0.6 * edge, 0.25 * edge)
    x1 = v + g.normal(size=v.shape) * 0.25 * edge
    want, counts = sr.sweep_rows_ref(v, x1, i, ids, it, counts=True)
    return v, x1, it, want, counts


@pytest.mark.parametrize("name", NAMES)
def test_row_sets_are_the_restatement(name):
    _, i, ids, edge = wr.MESHES[name]
    v, x1, it, want, counts = _case(name)
    n = it.shape[0]
    per = np.bincount(want.rows[:, 0].astype(np.int64), minlength=n)
    print(f"{name}: {want.rows.shape[0]} rows, {int((per == 0).sum())} of {n} items with none, {int((per >= 2).sum())} with several, counts {counts}")
    assert counts[2] == 0                                                       # the motion leaves nothing unresolved
    if i.shape[0] > 1:
        assert (per == 0).sum() >= n // 8 and want.rows.shape[0] >= n // 16 and ((want.toi > 0) & (want.toi < 1)).sum() >= 4
    with _ctx(v, i, ids) as cd:
        wr.same_rows(_sweep(cd, it, x1, name), want, name)
        assert _counts(cd) == counts, (name, _counts(cd), counts)
        assert i.shape[0] > 1 or cd.sweep_info.n_candidates == n              # one triangle: no records, every item meets leaf 0
        for m in (1, 63, 64, 65):                                               # the grid edge of the descent
            sub = sr.SweepRows(*(a[want.rows[:, 0] < m] for a in want))
            wr.same_rows(_sweep(cd, it[:m], x1, f"{name}, {m} items"), sub, f"{name}, {m} items")


def test_unresolved_rows_are_the_restatements():
    """Constructed: points that run along a face at 1.5 dist for some 2000 dist are left unresolved after 1024 evaluations."""
    it, t = sr.pin_class("unresolved", 8, np.random.default_rng(4))
    v = np.ascontiguousarray(t[:, :3].reshape(-1, 3))
    i = np.arange(24, dtype=np.uint32).reshape(8, 3)
    want, counts = sr.sweep_rows_ref(v, None, i, None, it, counts=True)
    assert counts[2] >= 8 and np.all(want.dist[want.rows[:, 0] == want.rows[:, 1]] > it[:, 6])
    with _ctx(v, i) as cd:
        wr.same_rows(_sweep(cd, it, None, "unresolved"), want, "unresolved")
        assert _counts(cd) == counts
        first = cd.sweep_points(it[:, 0:3], it[:, 3:6], it[:, 6])
        _same_tuple(first[:8], sr.first_of(want, 8), "unresolved, first contact")


# ---------------------------------------------------------------- 3: first contact
def _first(cd, it, x1, skip=None):
    got = cd.sweep_points(it[:, 0:3], it[:, 3:6], it[:, 6], verts_end=x1, skip_vertex=skip)
    assert got[8].n_found == int((got[0] != mi355cd.SWEEP_NONE).sum())
    return got


@pytest.mark.parametrize("name", NAMES)
def test_first_contact_is_the_smallest_row_of_the_devices_own_rows(name):
    _, i, ids, edge = wr.MESHES[name]
    v, x1, it, want, counts = _case(name)
    n = it.shape[0]
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, x1, name)
        got = _first(cd, it, x1)
        _same_tuple(got[:8], sr.first_of(rows, n), name)
        assert np.array_equal(np.bincount(rows.rows[:, 0].astype(np.int64), minlength=n) == 0, got[0] == mi355cd.SWEEP_NONE)
        assert got[8].tri_tests <= cd.sweep_info.n_evals                        # the cut-off only saves evaluations
        for m in (1, 63, 64, 65):
            _same_tuple(_first(cd, it[:m], x1)[:8], tuple(a[:m] for a in got[:8]), f"{name}, {m} items")


def _grid(n):
    """An integer-grid sheet of n x n quads in z = 0, two triangles a quad."""
    x, y = np.meshgrid(np.arange(n + 1.0), np.arange(n + 1.0), indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1)
    k = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    f = np.concatenate([np.stack([k, k + n + 1, k + n + 2], axis=1), np.stack([k, k + n + 2, k + 1], axis=1)])
    return v, f.astype(np.uint32)


def test_ties_at_equal_toi_go_to_the_smaller_id_then_face_index():
    """Points a quarter above the vertices and edge midpoints of an integer grid, dist a half: every incident face reports at toi = 0 with
    the same dist; IDs that repeat leave the face index to decide."""
    v, f = _grid(9)
    g = np.random.default_rng(6)
    ids = g.integers(0, 6, f.shape[0]).astype(np.uint32)                      # (few IDs: many ties go on to the face index)
    mids = 0.5 * (v[f[:, 0]] + v[f[:, 2]])                                      # the diagonals' midpoints: two faces share each
    p0 = np.concatenate([v, mids[: f.shape[0] // 2]]) + np.array([0.0, 0.0, 0.25])
    it = mi355cd.pack_sweeps(p0, p0 - np.array([0.0, 0.0, 0.5]), 0.5)
    n = it.shape[0]
    with _ctx(v, f, ids) as cd:
        rows = _sweep(cd, it, None, "grid")
        got = _first(cd, it, None)
    assert np.all(rows.toi == 0.0) and np.all(got[2] == 0.0) and np.all(got[0] != mi355cd.SWEEP_NONE)
    face, bid = got[0].astype(np.int64), got[1]
    by_id = by_face = 0
    for k in range(n):
        at = np.nonzero(rows.rows[:, 0] == k)[0]
        best = at[rows.dist[at] == rows.dist[at].min()]                         # (toi ties throughout: dist is not part of the key)
        key = min((int(rows.ids[r]), int(rows.rows[r, 1])) for r in at)
        assert (int(bid[k]), int(face[k])) == key, k
        by_id += len({int(rows.ids[r]) for r in at}) > 1
        by_face += sum(int(rows.ids[r]) == key[0] for r in at) > 1
        assert best.size >= 1
    assert by_id > 50 and by_face > 30, (by_id, by_face)
    _same_tuple(got[:8], sr.first_of(rows, n), "grid")


# ---------------------------------------------------------------- 4: consistency with the static queries
@pytest.mark.parametrize("name", ["soup10k", "cloth100", "n1", "n65"])
def test_no_motion_is_points_within(name):
    v, i, ids, edge = wr.MESHES[name]
    pts = wr.points(name)
    it = mi355cd.pack_sweeps(pts, pts, edge)
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, None, name)
        pw = cd.points_within(pts, edge, cap=CAP)
    assert pw[8] == OK and np.all(rows.toi == 0.0)
    static = wr.PointRows(*wr.sort_rows(*pw[:7]))
    wr.same_rows((rows.rows, rows.ids, rows.dist, rows.closest, rows.uv, rows.feature, rows.side), static, name)
    wr.same_rows((rows.rows, rows.ids, rows.dist, rows.closest, rows.uv, rows.feature, rows.side), wr.want_points(name, 1.0), name + ", restated")


@pytest.mark.parametrize("name", ["soup10k", "cloth100"])
def test_rows_at_toi_zero_are_points_within_on_x0(name):
    _, i, ids, edge = wr.MESHES[name]
    v, x1, it, want, counts = _case(name)
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, x1, name)
        pw = cd.points_within(it[:, 0:3], it[:, 6], cap=CAP)
    z = rows.toi == 0.0
    assert z.sum() > 20 and (~z).sum() > 20
    static = wr.PointRows(*wr.sort_rows(*pw[:7]))
    wr.same_rows(tuple(a[z] for a in (rows.rows, rows.ids, rows.dist, rows.closest, rows.uv, rows.feature, rows.side)), static, name)


@pytest.mark.parametrize("name", ["soup10k", "cloth100"])
def test_every_ray_hit_on_the_segment_has_a_row_no_later(name):
    """A static mesh and a small dist: wherever the segment p0 -> p1 crosses a triangle (cast_rays_all over [0, 1]) the sweep has a row
    of that (item, face) with toi <= the ray's t (the guarantee: at t the point is far closer than h)."""
    v, i, ids, edge = wr.MESHES[name]
    g = np.random.default_rng(13)
    p0 = wr.points(name)
    p1 = p0 + g.normal(size=p0.shape) * edge
    it = mi355cd.pack_sweeps(p0, p1, 0.05 * edge)
    with _ctx(v, i, ids) as cd:
        rows = _sweep(cd, it, None, name)
        hits = cd.cast_rays_all(p0, p1 - p0, 1.0, cap=CAP)
    assert hits[6] == OK and hits[5] > 30, hits[5:]
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(32)) | r[:, 1].astype(np.uint64)
    kr, kh = key(rows.rows), key(hits[0])
    at = np.minimum(np.searchsorted(kr, kh), kr.size - 1)
    assert np.array_equal(kr[at], kh), "a crossing without a row"
    assert np.all(rows.toi[at] <= hits[2])
    print(f"{name}: {hits[5]} crossings, {rows.rows.shape[0]} rows")


def test_tunnelling_through_a_thin_sheet_is_reported():
    v, f = _grid(8)
    g = np.random.default_rng(3)
    xy = g.uniform(0.5, 7.5, (200, 2))
    p0 = np.concatenate([xy, np.full((200, 1), 1.0)], axis=1)
    p1 = np.concatenate([xy + g.uniform(-0.4, 0.4, (200, 2)), np.full((200, 1), -1.0)], axis=1)
    with _ctx(v, f) as cd:
        for p in (p0, p1):
            assert cd.points_within(p, 0.01, cap=CAP)[7] == 0                  # nothing at either end
        it = mi355cd.pack_sweeps(p0, p1, 0.01)
        rows = _sweep(cd, it, None, "sheet")
        got = _first(cd, it, None)
    assert np.array_equal(np.unique(rows.rows[:, 0]), np.arange(200))
    assert np.all((rows.toi > 0.0) & (rows.toi < 1.0)) and np.all(rows.dist <= 0.01)
    assert np.all((got[2] >= 0.495 - 1e-12) & (got[2] <= 0.4975 + 1e-12))      # z = 1 - 2 t: within dist from t = 0.495 on, within h from 0.4975 on


# ---------------------------------------------------------------- 5: skip_vertex
def test_skip_vertex_on_a_cloths_own_vertices():
    v, f = synth.cloth_pair(24)
    v = np.asarray(v, dtype=np.float64)
    f = np.asarray(f)
    nv = v.shape[0]
    edge = 2.88 / 24
    x1 = v + np.random.default_rng(8).normal(size=v.shape) * 0.2 * edge
    it = mi355cd.pack_sweeps(v, x1, 0.2 * edge)
    skip = np.arange(nv, dtype=np.uint32)
    want, counts = sr.sweep_rows_ref(v, x1, f, None, it, skip=skip, counts=True)
    plain_want = sr.sweep_rows_ref(v, x1, f, None, it)
    assert counts[2] == 0 and want.rows.shape[0] > 100
    with _ctx(v, f) as cd:
        rows = _sweep(cd, it, x1, "cloth, skip", skip=skip)
        assert _counts(cd) == counts
        plain = _sweep(cd, it, x1, "cloth, no skip")
        first = _first(cd, it, x1, skip=skip)
        some = skip.copy(); some[::2] = mi355cd.SWEEP_NONE                       # every second item without a filter
        mixed = _sweep(cd, it, x1, "cloth, every second skip", skip=some)
    wr.same_rows(rows, want, "cloth, skip")
    wr.same_rows(plain, plain_want, "cloth, no skip")
    assert not (f[rows.rows[:, 1]] == rows.rows[:, 0:1]).any()
    inc = (f[plain.rows[:, 1]] == plain.rows[:, 0:1]).any(axis=1)
    assert inc.sum() == 3 * f.shape[0] and np.all(plain.toi[inc] == 0.0)         # without the skip every incident face is a row at toi 0
    wr.same_rows(sr.SweepRows(*(a[~inc] for a in plain)), want, "cloth, the rest")
    keep = ~inc | (plain.rows[:, 0] % 2 == 0)
    wr.same_rows(mixed, sr.SweepRows(*(a[keep] for a in plain)), "cloth, every second skip")
    _same_tuple(first[:8], sr.first_of(rows, nv), "cloth, first contact with skip")


# ---------------------------------------------------------------- 6: independence
def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def test_independent_of_frame_traversal_build_cell_table_and_item_order():
    name = "soup10k"
    _, i, ids, edge = wr.MESHES[name]
    v, x1, it, want, counts = _case(name)
    n = it.shape[0]
    perm = np.random.default_rng(4).permutation(n).astype(np.uint32)
    first_want = sr.first_of(want, n)

    def check(cd, what):
        wr.same_rows(_sweep(cd, it, x1, what), want, what)
        assert _counts(cd) == counts, what
        w = _sweep(cd, it[perm], x1, what + ", permuted")
        rows = w.rows.copy(); rows[:, 0] = perm[rows[:, 0]]
        wr.same_rows(wr.sort_rows(rows, *w[1:]), want, what + ", permuted")
        _same_tuple(_first(cd, it, x1)[:8], first_want, what)

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
        still = _sweep(cd, it, None, "verts_end None")                     # a mesh that does not move: NULL, or its own vertices
        assert still.rows.shape[0] > 50 and not np.array_equal(still.rows, want.rows)
        wr.same_rows(_sweep(cd, it, v, "verts_end = the vertices"), still, "verts_end None against the vertices themselves")
        _same_tuple(_first(cd, it, v)[:8], _first(cd, it, None)[:8], "first contact, verts_end None against the vertices themselves")


# ---------------------------------------------------------------- 7: overflow and growth, through the C interface
SENTINEL = 7
FIELDS = (("ids", np.uint32, ()), ("toi", np.float64, ()), ("dist", np.float64, ()), ("closest", np.float64, (3,)), ("uv", np.float64, (2,)),
          ("feature", np.uint8, ()), ("side", np.uint8, ()))


class _Raw:
    """A cd_sweep_points_all call through the C interface into sentinel-filled arrays of `room` rows."""

    def __init__(self, cd, room):
        self.cd = cd
        self.rows = np.full((max(room, 1), 2), SENTINEL, dtype=np.uint32)
        self.vals = [np.full((max(room, 1),) + shape, SENTINEL, dtype=dt) for _, dt, shape in FIELDS]
        self.out = mi355cd.CdSweepRows(*(a.ctypes.data for a in self.vals))
        self.n, self.info = C.c_uint64(SENTINEL), mi355cd.CdCcdInfo(SENTINEL, SENTINEL, SENTINEL, SENTINEL)

    def call(self, items, cap, x1=None, skip=None, n=None, null=False):
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        n = items.shape[0] if n is None else n
        return self.cd.lib.cd_sweep_points_all(self.cd._ctx, vp(x1), vp(items), n, vp(skip), None if null else vp(self.rows), cap, C.byref(self.n),
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
    _, i, ids, edge = wr.MESHES[name]
    v, x1, it, want, counts = _case(name)
    total = want.rows.shape[0]
    assert total > 130
    far = it.copy(); far[:, 0:6] += 100.0
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
        assert cd.lib.cd_sweep_points_all(cd._ctx, vp(x1), vp(it), it.shape[0], None, vp(r.rows), total, C.byref(r.n), None, None) == OK
        assert np.array_equal(wr.sort_rows(r.rows)[0], want.rows) and all((a == SENTINEL).all() for a in r.vals)


def test_candidate_buffer_grows_and_shrinking_calls_still_work():
    name = "soup10k"
    _, i, ids, edge = wr.MESHES[name]
    v, x1, it, want, counts = _case(name)
    nt = i.shape[0]
    p = np.ascontiguousarray(np.concatenate([it[:, 0:3], it[:, 0:3], it[:48, 0:3]], axis=0))
    assert p.shape[0] == 2048 and 2048 * nt >= 2 * mi355cd.WITHIN_SHARD_FIRST * mi355cd.WITHIN_SHARDS       # twice the first allocation, and more
    one = sr.SweepRows(*(a[want.rows[:, 0] < 1] for a in want))
    with _ctx(v, i, ids) as cd:
        wr.same_rows(_sweep(cd, it[:1], x1, "one item"), one, "one item")
        # resting points with a dist beyond the whole scene, the mesh at rest: every triangle is a candidate and a row, one evaluation each
        rows, *_, n, rc = cd.sweep_points_all(p, p, 1.0e4, cap=0)
        assert rc == OVERFLOW and rows.shape[0] == 0 and n == 2048 * nt, (rc, n)
        assert cd.sweep_info.n_candidates == cd.sweep_info.n_tested == cd.sweep_info.n_evals == 2048 * nt and cd.sweep_info.n_unresolved == 0
        wr.same_rows(_sweep(cd, it[:1], x1, "one item again"), one, "one item again")
        wr.same_rows(_sweep(cd, it, x1, "all items"), want, "all items after the growth")


# ---------------------------------------------------------------- 8: the context, errors, a mesh that moves
def test_leaves_the_context_as_it_was_and_errors_write_nothing():
    name = "soup10k"
    _, i, ids, edge = wr.MESHES[name]
    v, x1, it, want, counts = _case(name)
    it64 = np.ascontiguousarray(it[:64])
    with mi355cd.CollisionDetector(v, i) as cd:
        r = _Raw(cd, 256)                                                   # before a build
        assert r.call(it64, 256, x1) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        cd.self_collide(cap=CAP)
        ccd = cd.find_ccd(x1, 0.1 * edge, cap=CAP)
        assert ccd[3] > 0
        before = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(), cd.debug_swept(), cd.points_within(it[:, 0:3], edge, cap=CAP))
        wr.same_rows(_sweep(cd, it, x1, name), want, name)
        _first(cd, it, x1)
        other = v + 0.37 * edge                                             # another x1: the sweep's own swept records change, the CCD pass's do not
        assert _sweep(cd, it, other, name + ", another x1").rows.shape[0] > 0
        assert bytes(cd.stats()) == before[0]
        assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == before[1]
        after = cd.debug_swept()
        assert before[2][0].shape[0] == i.shape[0] and all(np.array_equal(a, b) for a, b in zip(before[2][:3], after[:3])) and before[2][3:] == after[3:]
        _same_tuple(wr.sort_rows(*cd.points_within(it[:, 0:3], edge, cap=CAP)[:7]), wr.sort_rows(*before[3][:7]), "points_within after the sweeps")
        again = cd.find_ccd(x1, 0.1 * edge, cap=CAP)
        assert again[3] == ccd[3] and np.array_equal(np.sort(again[0].view(np.uint64).ravel()), np.sort(ccd[0].view(np.uint64).ravel()))

        def bad(items, what, n=None, x1=x1):
            r = _Raw(cd, 256)
            assert r.call(items, 256, x1, n=n) == mi355cd.CD_ERR_ARG and r.nothing_written(), what
            face = np.full(64, SENTINEL, dtype=np.uint32)
            toi = np.full(64, float(SENTINEL))
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            rc = cd.lib.cd_sweep_points(cd._ctx, vp(x1), vp(items), items.shape[0] if n is None else n, None, 0, vp(face), None, vp(toi), None, None, None, None, None, None)
            assert rc == mi355cd.CD_ERR_ARG and (face == SENTINEL).all() and (toi == SENTINEL).all(), what

        for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (5, np.inf), (6, np.nan), (6, 0.0), (6, -1.0), (6, np.inf)):
            x = it64.copy(); x[63, col] = val                               # the LAST item: nothing may have been launched for the others
            bad(x, (col, val))
        bad(it64, "n = 2^32 + 1", n=(1 << 32) + 1)                          # (checked before the 64 items are read)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        r = _Raw(cd, 256)
        assert cd.lib.cd_sweep_points_all(cd._ctx, None, None, 64, None, vp(r.rows), 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG        # NULL items
        assert cd.lib.cd_sweep_points_all(cd._ctx, None, vp(it64), 64, None, None, 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG           # NULL rows with room asked for
        assert cd.lib.cd_sweep_points_all(cd._ctx, None, vp(it64), 64, None, vp(r.rows), 256, None, None, None) == mi355cd.CD_ERR_ARG and r.nothing_written()   # NULL n_rows
        assert r.call(it64, 256, n=0) == OK and r.n.value == 0 and r.untouched_from(0)                                                          # n = 0
        face = np.full(64, SENTINEL, dtype=np.uint32)
        assert cd.lib.cd_sweep_points(cd._ctx, None, vp(it64), 64, None, 1, vp(face), None, None, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG   # flags
        assert cd.lib.cd_sweep_points(cd._ctx, None, vp(it64), 64, None, 0, None, None, None, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG       # NULL face
        assert (face == SENTINEL).all()

        g = np.random.default_rng(9)
        moved = v + g.normal(0.0, 0.5 * edge, v.shape)
        cd.update_vertices(moved)
        r = _Raw(cd, 256)                                                   # after update_vertices without a rebuild
        assert r.call(it64, 256, x1) == mi355cd.CD_ERR_ORDER and r.nothing_written()
        cd.build_tree()
        new = sr.sweep_rows_ref(moved, x1, i, None, it)
        assert new.rows.shape != want.rows.shape or not np.array_equal(new.rows, want.rows)      # the answer did change
        wr.same_rows(_sweep(cd, it, x1, "moved"), new, "after update_vertices and a rebuild")
        _same_tuple(_first(cd, it, x1)[:8], sr.first_of(new, it.shape[0]), "first contact after update_vertices and a rebuild")


# ---------------------------------------------------------------- 9: the fp32 range ends, and a translated mesh
SCALE_MESHES = si.meshes()
NSCALE = 512


@functools.lru_cache(maxsize=None)
def _scale_case(name):
    """512 points of the mesh moved by N(0, 0.6 edge) a coordinate, dist a quarter edge, the mesh moving to scale_inputs.motion: the
    restatement's rows and counts at k = 0."""
    v, vidx, edge = SCALE_MESHES[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    p0 = ptr.mesh_points(vv, vidx, NSCALE, seed=3, edge=edge)
    it = mi355cd.pack_sweeps(p0, p0 + np.random.default_rng(21).normal(size=p0.shape) * 0.6 * edge, 0.25 * edge)
    x1 = si.motion(vv, edge)
    want, counts = sr.sweep_rows_ref(vv, x1, vidx, None, it, counts=True)
    return vv, vidx, x1, it, want, counts


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """Mesh, end positions and all seven columns of the items scaled by 2^k, past both fp32 ends (the band of tests/scale_inputs.py):
    the k = 0 rows, IDs, toi bits, u, v, feature and side, dist and closest times 2^k exactly, and the k = 0 counts; at the scales of
    scale_inputs.EDGES also the restatement on the scaled inputs themselves; first contact: first_of of those rows.  The descent and
    the first-contact kernel filter in fp32 with a pad of their own, 2 dist + 2 dist 2^-20 + M 2^-20 rounded up: +inf at the upper end
    of the band, a subnormal or 0 at the lower."""
    vv, vidx, x1, it, want, counts = _scale_case(name)
    per = np.bincount(want.rows[:, 0].astype(np.int64), minlength=NSCALE)
    inside = int(((want.toi > 0) & (want.toi < 1)).sum())
    assert (per == 0).sum() >= 64 and (per >= 2).sum() >= 32 and inside >= 4 and counts[2] == 0, ((per == 0).sum(), (per >= 2).sum(), inside, counts)
    what = f"{name} 2^{k}"
    ws = want._replace(dist=si.scaled(want.dist, k), closest=si.scaled(want.closest, k))
    vs, xs, its = si.scaled(vv, k), si.scaled(x1, k), si.scaled(it, k)
    with _ctx(vs, vidx) as cd:
        rows = _sweep(cd, its, xs, what)
        wr.same_rows(rows, ws, what)
        assert _counts(cd) == counts, (what, _counts(cd), counts)
        if k in si.EDGES:
            direct, direct_counts = sr.sweep_rows_ref(vs, xs, vidx, None, its, counts=True)
            wr.same_rows(rows, direct, what + ", the restatement on the scaled inputs")
            assert _counts(cd) == direct_counts, (what, _counts(cd), direct_counts)
        _same_tuple(_first(cd, its, xs)[:8], sr.first_of(ws, NSCALE), what + ", first contact")


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_mesh_gives_the_restatement(name):
    """Mesh, end positions, p0 and p1 translated by 2^20 + 0.37: M is 2^20 while the motion is a fraction of an edge, so the pad's
    M 2^-20 term (about 1) decides which candidates pass the fp32 filters."""
    vv, vidx, x1, it, _, _ = _scale_case(name)
    off = 2.0 ** 20 + 0.37
    vt, xt, itt = vv + off, x1 + off, it.copy()
    itt[:, 0:6] += off
    want, counts = sr.sweep_rows_ref(vt, xt, vidx, None, itt, counts=True)
    per = np.bincount(want.rows[:, 0].astype(np.int64), minlength=NSCALE)
    print(f"{name} translated: {want.rows.shape[0]} rows, {int((per == 0).sum())} of {NSCALE} items with none, {int((per >= 2).sum())} with several, counts {counts}")
    assert (per == 0).sum() >= 64 and (per >= 2).sum() >= 32
    with _ctx(vt, vidx) as cd:
        wr.same_rows(_sweep(cd, itt, xt, name), want, f"{name} translated")
        assert _counts(cd) == counts, (name, _counts(cd), counts)
        _same_tuple(_first(cd, itt, xt)[:8], sr.first_of(want, NSCALE), f"{name} translated, first contact")
