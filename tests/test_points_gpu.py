"""Closest-point queries on the device (cd_pt_tri_points, cd_closest_points) against the numpy restatement and the all-pairs minimum
of tests/point_ref.py -- which uses no box filter of any kind -- face, ID and the bits of dist, q, u, v, feature, side.  Every step
has bounded size."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import ccd_ref as cr
import mi355_synth as synth
import mi355cd
import oracle
import point_ref as ptr
import proximity_ref as pr
import query_meshes as qm
import scale_inputs as si

pytestmark = pytest.mark.gpu

CAP = 1 << 20
NPTS = 2048
NPTS_LARGE = 512                                                                # cloth300 has 360 000 triangles: all pairs on the CPU
NONE = 0xFFFFFFFF


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _same(got, want, what):
    face, ids, dist, q, uv, feat, side = got[:7]
    wf, wi, wd, wq, wuv, wfe, ws = want
    bad = np.nonzero((face != wf) | (ids != wi) | (_bits(dist) != _bits(wd)) | (_bits(q) != _bits(wq)).any(axis=1) | (_bits(uv) != _bits(wuv)).any(axis=1)
                     | (feat != wfe) | (side != ws))[0]
    assert bad.size == 0, (what, bad.size, bad[:5], face[bad[:5]], wf[bad[:5]], dist[bad[:5]], wd[bad[:5]], feat[bad[:5]], wfe[bad[:5]])
    if len(got) > 7:
        assert got[7].n_found == int((wf != NONE).sum()), what


def test_predicate_pin():
    """pt_tri on the device == the numpy restatement, bit for bit, on 2^20 pairs of every class."""
    total = 0
    for name, (pts, tris) in ptr.pair_classes(1 << 17, seed=11).items():
        dist, q, uv, feat, side = mi355cd.pt_tri_points(pts, tris)
        wd, wq, wu, wv, wf, ws = ptr.pt_tri_np(pts, tris)
        for got, want, what in ((dist, wd, "dist"), (q[:, 0], wq[:, 0], "qx"), (q[:, 1], wq[:, 1], "qy"), (q[:, 2], wq[:, 2], "qz"), (uv[:, 0], wu, "u"), (uv[:, 1], wv, "v")):
            bad = np.nonzero(_bits(got) != _bits(want))[0]
            assert bad.size == 0, (name, what, bad.size, got[bad[:3]], want[bad[:3]])
        assert np.array_equal(feat, wf), (name, int((feat != wf).sum()))
        assert np.array_equal(side, ws), name
        total += pts.shape[0]
        print(f"{name}: features {np.bincount(wf, minlength=7).tolist()}")
        assert name != "random" or (np.bincount(wf, minlength=7) > 0).all()    # every feature occurs
    assert total >= 1 << 20
    r = ptr.pair_classes(1 << 10, seed=12)
    pts, tris = r["random"]                                                     # outputs other than dist may be NULL
    dist = np.zeros(pts.shape[0])
    rc = mi355cd.load_library().cd_pt_tri_points(np.ascontiguousarray(pts).ctypes.data_as(C.c_void_p), np.ascontiguousarray(tris).ctypes.data_as(C.c_void_p),
                                                 pts.shape[0], dist.ctypes.data_as(C.c_void_p), None, None, None, None)
    assert rc == mi355cd.CD_OK and np.array_equal(_bits(dist), _bits(ptr.pt_tri_np(pts, tris)[0]))


MESHES = {m[0]: m[1:] for m in qm._meshes()}
SMALL = [name for name, m in MESHES.items() if m[1].shape[0] <= 10_000]


@functools.lru_cache(maxsize=None)
def _points(name, n=NPTS):
    v, i, ids, edge = MESHES[name]
    return ptr.mesh_points(v, i, n, seed=len(name) + i.shape[0], edge=edge)


@functools.lru_cache(maxsize=None)
def _want(name, n=NPTS):
    v, i, ids, edge = MESHES[name]
    return ptr.closest_points_ref(v, i, ids, _points(name, n))


@functools.lru_cache(maxsize=None)
def _radii(name, n=NPTS):
    return ptr.radii(_want(name, n)[2], MESHES[name][3], seed=7)


@functools.lru_cache(maxsize=None)
def _want_r(name, n=NPTS):
    v, i, ids, edge = MESHES[name]
    return ptr.closest_points_ref(v, i, ids, _points(name, n), _radii(name, n))


def _check_mesh(name, n):
    v, i, ids, edge = MESHES[name]
    want, want_r = _want(name, n), _want_r(name, n)
    with _ctx(v, i, ids) as cd:
        got = cd.closest_points(_points(name, n))
        _same(got, want, name)
        got_r = cd.closest_points(_points(name, n), _radii(name, n))
        _same(got_r, want_r, name + ", finite radii")
    info = got[7]
    assert (want[0] != NONE).all()                                              # rmax = +inf: every point has a nearest triangle
    nf = int((want_r[0] != NONE).sum())
    print(f"{name}: {info.node_visits / n:.1f} boxes and {info.tri_tests / n:.2f} pt_tri a point; finite radii: {nf} of {n} find a triangle, "
          f"{got_r[7].node_visits / n:.1f} boxes and {got_r[7].tri_tests / n:.2f} pt_tri")
    assert n // 4 <= nf <= n - n // 8, (name, nf)                               # a good share finds nothing, a good share something
    assert (want_r[0][2::4] != NONE).all()                                      # rmax == the nearest distance: closed
    return info


@pytest.mark.parametrize("name", SMALL)
def test_closest_points_on_small_meshes(name):
    assert {"comb", "duplicates", "custom_ids", "n1", "n2", "n3", "n63", "n64", "n65"} <= set(SMALL)
    info = _check_mesh(name, NPTS)
    nt = MESHES[name][1].shape[0]
    assert info.tri_tests >= NPTS and (nt == 1 or info.node_visits > 0)
    if nt == 1:
        assert info.tri_tests == NPTS and info.node_visits == 0


@pytest.mark.parametrize("name", ["cloth300", "soup100k"])
def test_closest_points_on_large_meshes_against_all_pairs(name):
    _check_mesh(name, NPTS_LARGE)


def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def test_independent_of_frame_traversal_build_and_point_order():
    name = "soup10k"
    v, i, ids, edge = MESHES[name]
    pts, want = _points(name), _want(name)
    perm = np.random.default_rng(4).permutation(NPTS)
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
                    what = f"frame {frame} traversal {trav} stagewise {stagewise}"
                    _same(cd.closest_points(pts), want, what)
                    g = cd.closest_points(pts[perm])
                    _same(g[:7], tuple(w[perm] for w in want), what + ", points permuted")
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)
        cd.set_morton_frame(mi355cd.CD_FRAME_REFERENCE)
        cd.build_tree()                                                    # the staged build (morton_sort, build_hierarchy, refit_boxes inside)
        _same(cd.closest_points(pts), want, "build_tree")
    name = "cloth100d"                                                     # full doubles: the cell table matters
    v, i, ids, edge = MESHES[name]
    pts, want = _points(name), _want(name)
    with mi355cd.CollisionDetector(v, i) as cd:
        for table in (0, 1):
            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
            cd.self_collide(cap=CAP)
            _same(cd.closest_points(pts), want, f"cell table {table}")


@pytest.mark.parametrize("name", ["soup10k", "cloth100", "duplicates", "comb", "n1", "n2", "n65"])
def test_any_within_is_defined_where_it_is_defined(name):
    v, i, ids, edge = MESHES[name]
    pts, rm, want = _points(name), _radii(name), _want_r(name)
    tris = np.asarray(v, dtype=np.float64)[np.asarray(i).astype(np.int64)]
    with _ctx(v, i, ids) as cd:
        face, info = cd.closest_points(pts, rm, any_within=True)
        assert np.array_equal(face != NONE, want[0] != NONE), name        # WHETHER there is one
        k = np.nonzero(face != NONE)[0]
        assert (face[k] < i.shape[0]).all()
        assert (ptr.pt_tri_np(pts[k], tris[face[k]])[0] <= rm[k]).all(), name      # the triangle returned is within rmax; WHICH one is not defined
        assert info.n_found == k.size
        face_inf, info_inf = cd.closest_points(pts, any_within=True)      # rmax = +inf: the seed alone answers
        assert (face_inf != NONE).all() and info_inf.tri_tests == NPTS
        lib, p4 = cd.lib, mi355cd.pack_points(pts, rm)
        buf = np.zeros(NPTS, dtype=np.float64)
        rc = lib.cd_closest_points(cd._ctx, p4.ctypes.data_as(C.c_void_p), NPTS, mi355cd.CD_POINT_ANY, face.ctypes.data_as(C.c_void_p), None,
                                   buf.ctypes.data_as(C.c_void_p), None, None, None, None, None)
        assert rc == mi355cd.CD_ERR_ARG and not buf.any()                  # an output other than face with CD_POINT_ANY


SCALE_MESHES = si.meshes()


@functools.lru_cache(maxsize=None)
def _scale_case(name):
    v, vidx, edge = SCALE_MESHES[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    pts = ptr.mesh_points(vv, vidx, NPTS, seed=3, edge=edge)
    inf = ptr.closest_points_ref(vv, vidx, None, pts)
    rm = ptr.radii(inf[2], edge, seed=4)
    rm[::2] = np.inf                                                            # half without a radius
    return vv, vidx, pts, rm, ptr.closest_points_ref(vv, vidx, None, pts, rm)


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """Mesh, points and radii scaled by 2^k, past both fp32 ends (the band of tests/scale_inputs.py, proximity's): the k = 0 faces, IDs,
    u, v, feature, side, and dist and q times 2^k exactly."""
    vv, vidx, pts, rm, want = _scale_case(name)
    ws = (want[0], want[1], si.scaled(want[2], k), si.scaled(want[3], k)) + want[4:]
    with _ctx(si.scaled(vv, k), vidx) as cd:
        _same(cd.closest_points(si.scaled(pts, k), si.scaled(rm, k)), ws, f"{name} 2^{k}")
    nf = int((want[0] != NONE).sum())
    assert NPTS // 2 < nf < NPTS


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_mesh_gives_the_restatement(name):
    vv, vidx, _, _, _ = _scale_case(name)
    edge = SCALE_MESHES[name][2]
    off = 2.0 ** 20 + 0.37
    vt = vv + off
    pts = ptr.mesh_points(vt, vidx, NPTS, seed=5, edge=edge)
    inf = ptr.closest_points_ref(vt, vidx, None, pts)
    rm = ptr.radii(inf[2], edge, seed=6)
    want = ptr.closest_points_ref(vt, vidx, None, pts, rm)
    with _ctx(vt, vidx) as cd:
        _same(cd.closest_points(pts), inf, f"{name} translated")
        _same(cd.closest_points(pts, rm), want, f"{name} translated, finite radii")
    print(f"{name} translated: {int((want[0] != NONE).sum())} of {NPTS} within their radius")


def test_leaves_the_context_as_it_was():
    """Modelled on test_rays_gpu.py's test of the same name: statistics, the last pair list, a captured step, the proximity and CCD
    results, the ray results; then proximity, CCD and ray calls interleaved with point calls."""
    import ray_ref as rr
    v, i = synth.soup(20000, e=0.02, seed=21)
    x1 = np.asarray(v) + np.random.default_rng(1).normal(0.0, 0.005, np.shape(v))
    pts = ptr.mesh_points(v, i, NPTS, seed=8, edge=0.02)
    want = ptr.closest_points_ref(v, i, None, pts)
    rays = rr.mesh_rays(v, i, 1024, seed=8)
    cast = lambda cd: cd.cast_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6])[:5]
    with mi355cd.CollisionDetector(v, i) as cd:
        cd.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)                      # what a captured step needs
        cd.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
        cd.set_option(mi355cd.CD_OPT_GRAPH, 1)
        ref = oracle.pipeline(cd.verts, cd.vidx)
        for _ in range(3):                                                 # capture, then replays
            cd.self_collide(cap=CAP)
        p, n, rc = cd.self_collide(cap=CAP)
        assert cd.stats().traverse_launches == 0, "the self step does not replay: nothing here would be tested"
        before = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(), cd.collision_triangles()[0],
                  cd.find_proximity(0.004, cap=CAP), cd.find_ccd(x1, 0.004, cap=CAP), cast(cd))
        hint0 = cd.debug_get(mi355cd.CD_DBG_GET_ORDER_STATE)
        _same(cd.closest_points(pts), want, "closest")
        cd.closest_points(pts, 0.01, any_within=True)
        st0, sp0, tri0, px0, cc0, ry0 = before
        assert bytes(cd.stats()) == st0
        assert cd.debug_get(mi355cd.CD_DBG_GET_ORDER_STATE) == hint0
        assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == sp0
        assert np.array_equal(cd.collision_triangles()[0], tri0)
        for rnd in range(2):                                               # interleaved: each still gives its earlier result
            gp, gd = pr.sort_pairs(*cd.find_proximity(0.004, cap=CAP)[:2])
            wp, wd = pr.sort_pairs(px0[0], px0[1])
            assert np.array_equal(gp, wp) and np.array_equal(_bits(gd), _bits(wd))
            _same(cd.closest_points(pts), want, f"closest after proximity {rnd}")
            g = cr.sort_pairs(*cd.find_ccd(x1, 0.004, cap=CAP)[:3])
            w = cr.sort_pairs(*cc0[:3])
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(g, w))
            _same(cd.closest_points(pts), want, f"closest after ccd {rnd}")
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(cast(cd), ry0))
            _same(cd.closest_points(pts), want, f"closest after rays {rnd}")
        rep0 = cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
        p, n, rc = cd.self_collide(cap=CAP)                                # the next self step still replays, and matches the oracle
        assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + 1 and cd.stats().traverse_launches == 0
        assert rc == mi355cd.CD_OK and np.array_equal(oracle.pair_set(p), oracle.pair_set(ref["pairs"]))
        _same(cd.closest_points(pts), want, "closest after a replayed step")


def test_order_and_argument_errors_write_nothing():
    v, i, ids, edge = MESHES["soup10k"]
    pts = mi355cd.pack_points(_points("soup10k")[:64])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    with mi355cd.CollisionDetector(v, i) as cd:
        lib = cd.lib
        outs = lambda: (np.full(64, 7, np.uint32), np.full(64, 7, np.uint32), np.full(64, 7.0), np.full((64, 3), 7.0), np.full((64, 2), 7.0),
                        np.full(64, 7, np.uint8), np.full(64, 7, np.uint8))
        def call(r, n=64, flags=0, o=None):
            o = outs() if o is None else o
            rc = lib.cd_closest_points(cd._ctx, vp(r) if r is not None else None, n, flags, *(vp(x) for x in o), None)
            return rc, o
        untouched = lambda o: all((x == 7).all() for x in o)
        rc, o = call(pts)
        assert rc == mi355cd.CD_ERR_ORDER and untouched(o)                 # before a build
        cd.build_tree()
        assert call(pts)[0] == mi355cd.CD_OK
        for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (3, -1.0), (3, -np.inf)):
            bad = pts.copy(); bad[63, col] = val                           # the LAST point: nothing may have been launched for the others
            rc, o = call(bad)
            assert rc == mi355cd.CD_ERR_ARG and untouched(o), (col, val)
        assert call(None)[0] == mi355cd.CD_ERR_ARG
        assert lib.cd_closest_points(cd._ctx, vp(pts), 64, 0, None, None, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG
        assert call(pts, flags=2)[0] == mi355cd.CD_ERR_ARG
        rc, o = call(pts, flags=mi355cd.CD_POINT_ANY)
        assert rc == mi355cd.CD_ERR_ARG and untouched(o)
        assert lib.cd_closest_points(None, vp(pts), 64, 0, vp(o[0]), None, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG
        assert call(None, n=0)[0] == mi355cd.CD_OK                         # n = 0
        rc, o = call(pts, n=0)
        assert rc == mi355cd.CD_OK and untouched(o)
        face = np.zeros(64, np.uint32)                                     # every output except face may be NULL
        assert lib.cd_closest_points(cd._ctx, vp(pts), 64, 0, vp(face), None, None, None, None, None, None, None) == mi355cd.CD_OK
        assert np.array_equal(face, _want("soup10k")[0][:64])
        zero_r = pts.copy(); zero_r[:, 3] = 0.0                            # rmax = 0 and +inf are values, not errors
        assert call(zero_r)[0] == mi355cd.CD_OK
        cd.update_vertices(np.asarray(v) + 0.001)
        rc, o = call(pts)
        assert rc == mi355cd.CD_ERR_ORDER and untouched(o)                 # after update_vertices without a rebuild
        cd.build_tree()
        rc, o = call(pts)
        assert rc == mi355cd.CD_OK
        _same(o, ptr.closest_points_ref(np.asarray(v) + 0.001, i, ids, pts[:, :3]), "after update_vertices and a rebuild")   # the moved mesh's answers, not the old tree's


def test_buffers_grow_from_one_point_to_a_million_and_back():
    v, i, ids, edge = MESHES["soup10k"]
    pts, want = _points("soup10k"), _want("soup10k")
    big = np.ascontiguousarray(np.tile(pts, ((1 << 20) // NPTS, 1)))
    with _ctx(v, i) as cd:
        _same(cd.closest_points(pts[:1])[:7], tuple(w[:1] for w in want), "1 point")
        g = cd.closest_points(big)
        assert g[7].n_found == 1 << 20
        for rep in (0, 1, (1 << 20) // NPTS - 1):
            _same(tuple(x[rep * NPTS:(rep + 1) * NPTS] for x in g[:7]), want, f"2^20 points, copy {rep}")
        _same(cd.closest_points(pts[:1])[:7], tuple(w[:1] for w in want), "1 point again")
        _same(cd.closest_points(pts[:65])[:7], tuple(w[:65] for w in want), "65 points")
        _same(cd.closest_points(pts), want, "all points")


def test_the_walk_prunes():
    """The guard against the degenerate walk (a condition, not a performance target): on soup100k, 2^14 points drawn on the surface and
    displaced by at most one mean edge length must cost no more than nt / 100 pt_tri evaluations a point.  Any walk that prunes stays
    orders of magnitude below; one that tests half the tree before it has a bound does not."""
    v, i, ids, edge = MESHES["soup100k"]
    v = np.asarray(v, dtype=np.float64)
    tris = v[np.asarray(i).astype(np.int64)]
    nt, n = tris.shape[0], 1 << 14
    g = np.random.default_rng(2)
    t = tris[g.integers(0, nt, n)]
    a, b = ptr._bary_in(g, n)
    mean_edge = float(np.mean([np.linalg.norm(tris[:, (k + 1) % 3] - tris[:, k], axis=1).mean() for k in range(3)]))
    d = g.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = t[:, 0] + a[:, None] * (t[:, 1] - t[:, 0]) + b[:, None] * (t[:, 2] - t[:, 0]) + d * (mean_edge * g.random(n))[:, None]
    with _ctx(v, i) as cd:
        got = cd.closest_points(pts)
    info = got[7]
    print(f"soup100k, {n} points within {mean_edge:.4f} of the surface: {info.node_visits / n:.1f} boxes and {info.tri_tests / n:.2f} pt_tri a point "
          f"(the guard: {nt / 100:.0f})")
    assert info.n_found == n and (got[2] <= mean_edge * (1 + 1e-9)).all()
    assert info.tri_tests <= n * nt // 100


@pytest.mark.parametrize("n", [2, 3, 65])
def test_a_walk_that_must_visit_every_node(n):
    """n coincident triangles, each on vertices of its own, default IDs: all boxes of the tree are one box, so a point that enters
    one subtree enters all.  Nearest-triangle queries above the interior with rmax = +inf: the seed descent looks at both children
    of D nodes (ties to the left: the same path, of depth D, for every point) and tests its leaf; the walk's bound is then the
    common distance, the box test is closed at it, so the walk visits every node but the root once -- 2 n - 2 boxes, the most a
    walk over a tree makes -- and tests all n triangles, the seed leaf a second time.  Every point reports the smallest ID."""
    v = np.tile(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (n, 1))
    i = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    g = np.linspace(0.125, 0.375, 8)
    pts = np.array([[x, y, 0.5] for x in g for y in g])
    p = pts.shape[0]
    with _ctx(v, i) as cd:
        got = cd.closest_points(pts)
    face, ids, dist, info = got[0], got[1], got[2], got[7]
    print(f"{n} coincident triangles, {p} points: {info.node_visits / p:.1f} boxes and {info.tri_tests / p:.2f} pt_tri a point")
    assert (face == 0).all() and (ids == 0).all() and (dist == 0.5).all() and info.n_found == p
    assert info.tri_tests == p * (n + 1)
    seed = info.node_visits - p * (2 * n - 2)                                   # 2 D boxes a point
    assert seed % (2 * p) == 0 and 1 <= seed // (2 * p) <= n - 1, (info.node_visits, seed)
    assert n != 2 or seed == 2 * p


def test_project_one_cloth_sheet_onto_the_other():
    """The usage the query is for: every vertex of one sheet of cloth_pair(100) projected onto the other sheet's mesh (two contexts,
    one per sheet), against the restatement."""
    v, i = synth.cloth_pair(100)
    v = np.asarray(v, dtype=np.float64)
    i = np.asarray(i)
    half = i.shape[0] // 2
    sheets = []
    for f in (i[:half], i[half:]):
        used = np.unique(f)
        assert used.size < v.shape[0]                                           # the sheets share no vertex
        sheets.append((np.ascontiguousarray(v[used]), np.searchsorted(used, f).astype(np.uint32)))
    (va, fa), (vb, fb) = sheets
    assert not set(np.unique(i[:half])) & set(np.unique(i[half:]))
    want = ptr.closest_points_ref(vb, fb, None, va)
    with _ctx(va, fa) as a, _ctx(vb, fb) as b:
        got = b.closest_points(a.verts)                                         # a's vertices onto b
        _same(got, want, "sheet a onto sheet b")
        back = a.closest_points(got[3])                                         # the projections lie on b; from there back to a
        _same(back, ptr.closest_points_ref(va, fa, None, got[3]), "the projections back onto sheet a")
    tb = vb[fb.astype(np.int64)][got[0]]
    assert np.array_equal(_bits(ptr.point_from_uv(got[4][:, 0], got[4][:, 1], tb)), _bits(got[3]))     # closest IS the point (face, uv) names
    gap = got[2]
    print(f"{va.shape[0]} vertices projected: distance {gap.min():.4f} .. {gap.max():.4f}, features {np.bincount(got[5], minlength=7).tolist()}")
    assert gap.max() < 0.5
