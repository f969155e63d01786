"""The all-results item queries on the device (cd_points_within, cd_cast_rays_all) against the all-pairs restatement of
tests/within_ref.py -- which uses no box filter of any kind -- as sets of (item, face) and bit for bit in every value of a row, and
against the device's own single-answer calls.  Every step has bounded size."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import mi355_synth as synth
import mi355cd
import oracle
import point_ref as ptr
import proximity_ref as pr
import ray_ref as rr
import scale_inputs as si
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


def _points(cd, pts, rmax, what, cap=CAP):
    """points_within's rows as a PointRows sorted by (item, face); the call fitted its capacity."""
    got = cd.points_within(pts, rmax, cap=cap)
    assert got[8] == OK and got[7] == got[0].shape[0] and cd.within_tested >= got[7], (what, got[7:], cd.within_tested)
    return wr.PointRows(*wr.sort_rows(*got[:7]))


def _rays(cd, rays, what, cap=CAP):
    got = cd.cast_rays_all(rays[:, 0:3], rays[:, 3:6], rays[:, 6], cap=cap)
    assert got[6] == OK and got[5] == got[0].shape[0] and cd.rays_all_tested >= got[5], (what, got[5:], cd.rays_all_tested)
    return wr.RayRows(*wr.sort_rows(*got[:5]))


def _same_tuple(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        if b.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        assert np.array_equal(a, b), (what, k)


# ---------------------------------------------------------------- 1, 2: the row sets, and their minima against the single-answer calls
@pytest.mark.parametrize("name", NAMES)
def test_row_sets_are_the_restatements(name):
    """Points at radius edge and 3 edge and rays: the restatement's set of (item, face), and every value of every row bit for bit."""
    wr.input_conditions(name)
    v, i, ids, edge = wr.MESHES[name]
    pts, rays = wr.points(name), wr.rays(name)
    assert pts.shape[0] == wr.n_items(name) == rays.shape[0]
    with _ctx(v, i, ids) as cd:
        for factor in (1.0, 3.0):
            want = wr.want_points(name, factor)
            wr.same_rows(_points(cd, pts, factor * edge, name), want, f"{name}, points within {factor} edge")
            print(f"{name}: {want.rows.shape[0]} rows within {factor} edge, {cd.within_tested} pt_tri")
            assert i.shape[0] > 1 or cd.within_tested == pts.shape[0]           # one triangle: no records, every point tests leaf 0
        want = wr.want_rays(name)
        wr.same_rows(_rays(cd, rays, name), want, f"{name}, rays")
        print(f"{name}: {want.rows.shape[0]} hits, {cd.rays_all_tested} ray_tri")


@pytest.mark.parametrize("name", NAMES)
def test_the_smallest_row_of_an_item_is_the_single_answer_calls(name):
    """By definition: per item the row with the smallest (dist or t, ID, face) is closest_points' / cast_rays' answer of the DEVICE, bit
    for bit, and the items with no row are its 0xFFFFFFFF items."""
    v, i, ids, edge = wr.MESHES[name]
    pts, rays = wr.points(name), wr.rays(name)
    n = pts.shape[0]
    with _ctx(v, i, ids) as cd:
        for factor in (1.0, 3.0):
            rows = _points(cd, pts, factor * edge, name)
            single = cd.closest_points(pts, factor * edge)[:7]
            _same_tuple(wr.closest_of(rows, n), single, f"{name}, {factor} edge")
            assert np.array_equal(wr.rows_per_item(rows, n) == 0, single[0] == mi355cd.POINT_NONE)
        rows = _rays(cd, rays, name)
        single = cd.cast_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6])[:5]
        _same_tuple(wr.first_hit_of(rows, n), single, f"{name}, rays")
        assert np.array_equal(wr.rows_per_item(rows, n) == 0, single[0] == mi355cd.RAY_MISS)


# ---------------------------------------------------------------- 3: independence
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
    v, i, ids, edge = wr.MESHES[name]
    pts, rays = wr.points(name), wr.rays(name)
    want_p, want_r = wr.want_points(name, 3.0), wr.want_rays(name)
    perm = np.random.default_rng(4).permutation(pts.shape[0]).astype(np.uint32)

    def check(cd, what):
        wr.same_rows(_points(cd, pts, 3 * edge, what), want_p, what)
        wr.same_rows(_rays(cd, rays, what), want_r, what)
        wr.same_rows(_unpermuted(_points(cd, pts[perm], 3 * edge, what), perm), want_p, what + ", points permuted")
        wr.same_rows(_unpermuted(_rays(cd, rays[perm], what), perm), want_r, what + ", rays permuted")

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


# ---------------------------------------------------------------- 4: overflow, through the C interface
SENTINEL = 7


class _Raw:
    """A call through the C interface into sentinel-filled arrays of `room` rows."""
    POINT = (("ids", np.uint32, ()), ("dist", np.float64, ()), ("closest", np.float64, (3,)), ("uv", np.float64, (2,)), ("feature", np.uint8, ()), ("side", np.uint8, ()))
    RAY = (("ids", np.uint32, ()), ("t", np.float64, ()), ("uv", np.float64, (2,)), ("side", np.uint8, ()))

    def __init__(self, cd, kind, room):
        self.cd, self.kind, self.room = cd, kind, room
        self.fn = cd.lib.cd_points_within if kind == "points" else cd.lib.cd_cast_rays_all
        self.rows = np.full((max(room, 1), 2), SENTINEL, dtype=np.uint32)
        self.vals = [np.full((max(room, 1),) + shape, SENTINEL, dtype=dt) for _, dt, shape in (self.POINT if kind == "points" else self.RAY)]
        self.out = (mi355cd.CdPointRows if kind == "points" else mi355cd.CdRayRows)(*(a.ctypes.data for a in self.vals))
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
    g = wr.sort_rows(*got)
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(32)) | r[:, 1].astype(np.uint64)
    kg, kw = key(g[0]), key(want.rows)
    assert np.unique(kg).size == kg.size, what
    at = np.minimum(np.searchsorted(kw, kg), kw.size - 1)
    assert np.array_equal(kw[at], kg), what
    wr.same_rows(g, type(want)(*(a[at] for a in want)), what)


@pytest.mark.parametrize("kind", ["points", "rays"])
def test_overflow(kind):
    name = "soup10k"
    v, i, ids, edge = wr.MESHES[name]
    if kind == "points":
        items, want = mi355cd.pack_points(wr.points(name), 3 * edge), wr.want_points(name, 3.0)
        empty = mi355cd.pack_points(wr.points(name) + 100.0, 0.0)                                   # far from the mesh, radius 0: no rows
    else:
        items, want = wr.rays(name), wr.want_rays(name)
        empty = wr.rays(name).copy(); empty[:, 0:3] += 100.0; empty[:, 6] = 0.0                     # far from the mesh, tmax 0
    total = want.rows.shape[0]
    assert total > 64
    with _ctx(v, i, ids) as cd:
        r = _Raw(cd, kind, 0)                                                                       # the count-only call
        assert r.call(items, 0, null=True) == OVERFLOW and r.n.value == total and r.tested.value >= total
        assert r.call(empty, 0, null=True) == OK and r.n.value == 0
        r = _Raw(cd, kind, total + 64)                                                              # one row short
        assert r.call(items, total - 1) == OVERFLOW and r.n.value == total
        assert r.untouched_from(total - 1), "written at or past cap_rows"
        _distinct_members(r.written(total - 1), want, f"{kind}, cap = n_rows - 1")
        r = _Raw(cd, kind, total + 64)                                                              # a small prefix
        assert r.call(items, 65) == OVERFLOW and r.n.value == total and r.untouched_from(65)
        _distinct_members(r.written(65), want, f"{kind}, cap = 65")
        r = _Raw(cd, kind, total + 64)                                                              # exactly enough
        assert r.call(items, total) == OK and r.n.value == total and r.untouched_from(total)
        wr.same_rows(r.written(total), want, f"{kind}, cap = n_rows")
        r = _Raw(cd, kind, total)                                                                   # rows only: out and n_tested NULL
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert r.fn(cd._ctx, vp(items), items.shape[0], vp(r.rows), total, C.byref(r.n), None, None) == OK
        assert np.array_equal(wr.sort_rows(r.rows)[0], want.rows) and all((a == SENTINEL).all() for a in r.vals)


# ---------------------------------------------------------------- 5, 6: infinite bounds, and the candidate buffer's growth
def test_infinite_radius_returns_every_triangle():
    v, i, ids, edge = wr.MESHES["n65"]
    pts = wr.points("n65")[:130]
    with _ctx(v, i, ids) as cd:
        rows = _points(cd, pts, np.inf, "n65")
        assert rows.rows.shape[0] == 130 * 65 and cd.within_tested == 130 * 65
        assert np.array_equal(rows.rows, np.stack(np.divmod(np.arange(130 * 65, dtype=np.uint32), np.uint32(65)), axis=1))
        wr.same_rows(rows, wr.points_within_ref(v, i, ids, pts, np.inf), "n65, rmax = +inf")


def test_candidate_buffer_grows_and_shrinking_calls_still_work():
    name = "soup10k"
    v, i, ids, edge = wr.MESHES[name]
    nt = i.shape[0]
    pts = wr.points(name)
    big = np.ascontiguousarray(np.concatenate([pts, pts, pts[:48]], axis=0))
    assert big.shape[0] == 2048 and 2048 * nt >= 2 * mi355cd.WITHIN_SHARD_FIRST * mi355cd.WITHIN_SHARDS      # twice the first allocation, and more
    one = wr.points_within_ref(v, i, ids, pts[:1], 3 * edge)
    with _ctx(v, i, ids) as cd:
        wr.same_rows(_points(cd, pts[:1], 3 * edge, "one point"), one, "one point")
        rows, *_, n, rc = cd.points_within(big, np.inf, cap=0)
        assert rc == OVERFLOW and rows.shape[0] == 0 and n == 2048 * nt and cd.within_tested == 2048 * nt, (rc, n, cd.within_tested)
        wr.same_rows(_points(cd, pts[:1], 3 * edge, "one point again"), one, "one point again")
        wr.same_rows(_points(cd, pts, 3 * edge, "all points"), wr.want_points(name, 3.0), "all points after the growth")


# ---------------------------------------------------------------- 7: the context, and errors
def test_leaves_the_context_as_it_was_and_errors_write_nothing():
    name = "soup10k"
    v, i, ids, edge = wr.MESHES[name]
    pts, rays = wr.points(name), wr.rays(name)
    p4 = mi355cd.pack_points(pts[:64], 3 * edge)
    r7 = np.ascontiguousarray(rays[:64])
    with mi355cd.CollisionDetector(v, i) as cd:
        for kind, items in (("points", p4), ("rays", r7)):                 # before a build
            r = _Raw(cd, kind, 256)
            assert r.call(items, 256) == mi355cd.CD_ERR_ORDER and r.nothing_written(), kind
        cd.self_collide(cap=CAP)
        before = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(), cd.find_proximity(0.004, cap=CAP))
        wr.same_rows(_points(cd, pts, 3 * edge, name), wr.want_points(name, 3.0), name)
        wr.same_rows(_rays(cd, rays, name), wr.want_rays(name), name)
        assert bytes(cd.stats()) == before[0]
        assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == before[1]
        gp, gd = pr.sort_pairs(*cd.find_proximity(0.004, cap=CAP)[:2])
        wp, wd = pr.sort_pairs(*before[2][:2])
        assert gp.shape[0] > 0 and np.array_equal(gp, wp) and np.array_equal(_bits(gd), _bits(wd))
        wr.same_rows(_points(cd, pts, 3 * edge, name), wr.want_points(name, 3.0), name + ", after proximity")

        def bad(kind, items, what, n=None):
            r = _Raw(cd, kind, 256)
            assert r.call(items, 256, n=n) == mi355cd.CD_ERR_ARG and r.nothing_written(), what

        for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (3, -1.0), (3, -np.inf)):
            x = p4.copy(); x[63, col] = val                               # the LAST item: nothing may have been launched for the others
            bad("points", x, ("point", col, val))
        for col, val in ((0, np.nan), (4, np.inf), (6, np.nan), (6, -1.0)):
            x = r7.copy(); x[63, col] = val
            bad("rays", x, ("ray", col, val))
        x = r7.copy(); x[63, 3:6] = 0.0
        bad("rays", x, "zero direction")
        bad("points", p4, "n = 2^32", n=1 << 32)                          # (checked before the 64 points are read)
        bad("rays", r7, "n = 2^32", n=1 << 32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        r = _Raw(cd, "points", 256)
        assert r.fn(cd._ctx, None, 64, vp(r.rows), 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG               # NULL items
        assert r.fn(cd._ctx, vp(p4), 64, None, 256, C.byref(r.n), None, None) == mi355cd.CD_ERR_ARG                   # NULL rows with room asked for
        assert r.fn(cd._ctx, vp(p4), 64, vp(r.rows), 256, None, None, None) == mi355cd.CD_ERR_ARG and r.nothing_written()   # NULL n_rows
        assert r.call(p4, 256, n=0) == OK and r.n.value == 0 and r.untouched_from(0)                                  # n = 0
        assert r.fn(cd._ctx, None, 0, None, 0, C.byref(r.n), None, None) == OK and r.n.value == 0
        zero = p4.copy(); zero[:, 3] = 0.0                                 # rmax = 0 is a value, not an error
        assert _Raw(cd, "points", 256).call(zero, 256) == OK

        moved = np.asarray(v) + 0.001
        cd.update_vertices(moved)
        for kind, items in (("points", p4), ("rays", r7)):                 # after update_vertices without a rebuild
            r = _Raw(cd, kind, 256)
            assert r.call(items, 256) == mi355cd.CD_ERR_ORDER and r.nothing_written(), kind
        cd.build_tree()
        wr.same_rows(_points(cd, pts[:64], 3 * edge, "moved"), wr.points_within_ref(moved, i, ids, pts[:64], 3 * edge), "after update_vertices and a rebuild")


# ---------------------------------------------------------------- 8: the fp32 range ends, and a translated mesh
SCALE_MESHES = si.meshes()
NSCALE = 512


def _scale_radii(vv, vidx, pts, edge, seed):
    rm = ptr.radii(ptr.closest_points_ref(vv, vidx, None, pts)[2], edge, seed=seed)
    rm[::16] = np.inf                                                           # some without a radius: every triangle is a row
    return rm


@functools.lru_cache(maxsize=None)
def _scale_case(name):
    v, vidx, edge = SCALE_MESHES[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    pts = ptr.mesh_points(vv, vidx, NSCALE, seed=3, edge=edge)
    rm = _scale_radii(vv, vidx, pts, edge, 4)
    return vv, vidx, pts, rm, wr.points_within_ref(vv, vidx, None, pts, rm)


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """Mesh, points and radii scaled by 2^k, past both fp32 ends (the band of tests/scale_inputs.py): the k = 0 rows, IDs, u, v,
    feature, side, and dist and closest times 2^k exactly."""
    vv, vidx, pts, rm, want = _scale_case(name)
    ws = want._replace(dist=si.scaled(want.dist, k), closest=si.scaled(want.closest, k))
    with _ctx(si.scaled(vv, k), vidx) as cd:
        wr.same_rows(_points(cd, si.scaled(pts, k), si.scaled(rm, k), name), ws, f"{name} 2^{k}")
    c = wr.rows_per_item(want, NSCALE)
    assert (c == 0).sum() >= NSCALE // 8 and (c >= 2).sum() >= NSCALE // 16 and (c[::16] == vidx.shape[0]).all()


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_mesh_gives_the_restatement(name):
    vv, vidx, _, _, _ = _scale_case(name)
    edge = SCALE_MESHES[name][2]
    vt = vv + (2.0 ** 20 + 0.37)
    pts = ptr.mesh_points(vt, vidx, NSCALE, seed=5, edge=edge)
    rm = _scale_radii(vt, vidx, pts, edge, 6)
    want = wr.points_within_ref(vt, vidx, None, pts, rm)
    with _ctx(vt, vidx) as cd:
        wr.same_rows(_points(cd, pts, rm, name), want, f"{name} translated")
    print(f"{name} translated: {want.rows.shape[0]} rows, {int((wr.rows_per_item(want, NSCALE) == 0).sum())} of {NSCALE} points with none")


@functools.lru_cache(maxsize=None)
def _ray_scale_case(name):
    v, vidx, edge = SCALE_MESHES[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    rays = rr.mesh_rays(vv, vidx, NSCALE, seed=3)
    return vv, vidx, rays, wr.cast_rays_all_ref(vv, vidx, None, rays)


BAND = tuple(k for k in si.SCALES if abs(k) <= 300) + (-300, 300)             # tests/test_rays_gpu.py's: the band include/mi355cd.h states for ray_tri


@pytest.mark.parametrize("k", BAND)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_rays_fp32_range(name, k):
    """cd_cast_rays_all with mesh, origins and directions scaled by 2^k, past both fp32 ends (tmax is a parameter value and stays): the
    k = 0 rows, IDs, t bits, u, v and side; at the scales of scale_inputs.EDGES also the restatement on the scaled inputs themselves."""
    vv, vidx, rays, want = _ray_scale_case(name)
    c = wr.rows_per_item(want, NSCALE)
    assert (c == 0).sum() >= 64 and (c >= 2).sum() >= 32, ((c == 0).sum(), (c >= 2).sum())
    rs = rays.copy()
    rs[:, 0:6] = si.scaled(rays[:, 0:6], k)
    with _ctx(si.scaled(vv, k), vidx) as cd:
        rows = _rays(cd, rs, name)
    wr.same_rows(rows, want, f"{name} 2^{k}")
    if k in si.EDGES:
        wr.same_rows(rows, wr.cast_rays_all_ref(si.scaled(vv, k), vidx, None, rs), f"{name} 2^{k}, the restatement on the scaled inputs")


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_rays_on_a_translated_mesh_give_the_restatement(name):
    vv, vidx, _, _ = _ray_scale_case(name)
    vt = vv + (2.0 ** 20 + 0.37)
    rt = rr.mesh_rays(vt, vidx, NSCALE, seed=5)
    want = wr.cast_rays_all_ref(vt, vidx, None, rt)
    c = wr.rows_per_item(want, NSCALE)
    print(f"{name} translated: {want.rows.shape[0]} hits, {int((c == 0).sum())} of {NSCALE} rays with none, {int((c >= 2).sum())} with several")
    assert (c == 0).sum() >= 64 and (c >= 2).sum() >= 32
    with _ctx(vt, vidx) as cd:
        wr.same_rows(_rays(cd, rt, name), want, f"{name} translated")


# ---------------------------------------------------------------- 9: a mesh that moves
def test_rows_follow_a_mesh_that_moves():
    """update_vertices and a rebuild through the stage-wise and the fused path: the rows of the new positions, not the old tree's."""
    name = "custom_ids"
    v, i, ids, edge = wr.MESHES[name]
    pts, rays = wr.points(name), wr.rays(name)
    g = np.random.default_rng(9)
    v0 = np.asarray(v, dtype=np.float64)
    with _ctx(v0, i, ids) as cd:
        wr.same_rows(_points(cd, pts, 3 * edge, name), wr.want_points(name, 3.0), "frame 0")
        prev = wr.want_points(name, 3.0).rows
        for f, stagewise in ((1, 1), (2, 0)):
            vf = v0 + g.normal(0.0, 0.5 * edge, v0.shape)
            cd.update_vertices(vf)
            cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, stagewise)
            cd.self_collide(cap=CAP)
            want = wr.points_within_ref(vf, i, ids, pts, 3 * edge)
            assert want.rows.shape != prev.shape or not np.array_equal(want.rows, prev)              # the answer did change
            prev = want.rows
            wr.same_rows(_points(cd, pts, 3 * edge, name), want, f"frame {f}, stagewise {stagewise}: points")
            wr.same_rows(_rays(cd, rays, name), wr.cast_rays_all_ref(vf, i, ids, rays), f"frame {f}, stagewise {stagewise}: rays")
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)


# ---------------------------------------------------------------- 10: the use
def test_vertex_face_proximity_between_two_cloth_sheets():
    """What the query is for: every vertex of one sheet of cloth_pair(100) against the other sheet's triangles within 1.5 edges."""
    v, i = synth.cloth_pair(100)
    v = np.asarray(v, dtype=np.float64)
    i = np.asarray(i)
    half = i.shape[0] // 2
    sheets = []
    for f in (i[:half], i[half:]):
        used = np.unique(f)
        sheets.append((np.ascontiguousarray(v[used]), np.searchsorted(used, f).astype(np.uint32)))
    (va, fa), (vb, fb) = sheets
    h = 1.5 * 2.88 / 100
    want = wr.points_within_ref(vb, fb, None, va, h)
    with _ctx(va, fa) as a, _ctx(vb, fb) as b:
        rows = _points(b, a.verts, h, "sheet a's vertices against sheet b")
        wr.same_rows(rows, want, "sheet a's vertices against sheet b")
        single = b.closest_points(a.verts, h)[:7]
        _same_tuple(wr.closest_of(rows, va.shape[0]), single, "per-vertex minimum")
    c = wr.rows_per_item(want, va.shape[0])
    print(f"{va.shape[0]} vertices, {want.rows.shape[0]} vertex-face rows, {c.min()} .. {c.max()} a vertex, {b.within_tested} pt_tri")
    assert c.max() > 1
