"""Ray queries on the device (cd_ray_tri_points, cd_cast_rays) against the numpy restatement and the all-pairs closest hit of
tests/ray_ref.py -- which uses no box filter of any kind -- face, ID and the bits of t, u, v.  Every step has bounded size."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import ccd_ref as cr
import mi355_synth as synth
import mi355cd
import oracle
import proximity_ref as pr
import query_meshes as qm
import ray_ref as rr
import scale_inputs as si

pytestmark = pytest.mark.gpu

CAP = 1 << 20
NRAYS = 4096
MISS = 0xFFFFFFFF
BAND = tuple(k for k in si.SCALES if abs(k) <= 300) + (-300, 300)             # the band include/mi355cd.h states for ray_tri


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _cast(cd, rays, any_hit=False):
    return cd.cast_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6], any_hit=any_hit)


def _same(got, want, what):
    face, ids, t, uv, side = got[:5]
    wf, wi, wt, wuv, ws = want
    bad = np.nonzero((face != wf) | (ids != wi) | (_bits(t) != _bits(wt)) | (_bits(uv) != _bits(wuv)).any(axis=1) | (side != ws))[0]
    assert bad.size == 0, (what, bad.size, bad[:5], face[bad[:5]], wf[bad[:5]], t[bad[:5]], wt[bad[:5]])
    if len(got) > 5:
        assert got[5].n_hits == int((wf != MISS).sum()), what


def test_predicate_pin():
    """ray_tri on the device == the numpy restatement, bit for bit, on 2^20 pairs of every class (zero direction components,
    tmax = 0 and tmax = +inf among them)."""
    total = 0
    for name, (rays, tris) in rr.pair_classes(1 << 17, seed=11).items():
        hit, t, uv, side = mi355cd.ray_tri_points(rays, tris)
        wh, wt, wu, wv, ws = rr.ray_tri_np(rays, tris)
        assert np.array_equal(hit, wh), (name, int((hit != wh).sum()))
        for got, want, what in ((t, wt, "t"), (uv[:, 0], wu, "u"), (uv[:, 1], wv, "v")):
            bad = np.nonzero(_bits(got) != _bits(want))[0]
            assert bad.size == 0, (name, what, bad.size, got[bad[:3]], want[bad[:3]])
        assert np.array_equal(side, ws), name
        total += rays.shape[0]
        print(f"{name}: {int(hit.sum())} hits of {rays.shape[0]}")
        assert name in ("degenerate", "in_plane") or hit.sum() > rays.shape[0] // 16, name
    assert total >= 1 << 20
    r = rr.pair_classes(1 << 10, seed=12)
    assert (r["axis"][0][:, 3:6] == 0.0).any() and (r["on_triangle"][0][:, 6] == 0.0).any() and np.isinf(r["random"][0][:, 6]).any()
    # outputs other than hit may be NULL
    rays, tris = r["random"]
    hit = np.zeros(rays.shape[0], dtype=np.uint8)
    rc = mi355cd.load_library().cd_ray_tri_points(rays.ctypes.data_as(C.c_void_p), np.ascontiguousarray(tris).ctypes.data_as(C.c_void_p), rays.shape[0],
                                                  hit.ctypes.data_as(C.c_void_p), None, None, None)
    assert rc == mi355cd.CD_OK and np.array_equal(hit.astype(bool), rr.ray_tri_np(rays, tris)[0])


MESHES = {m[0]: m[1:] for m in qm._meshes()}
SMALL = [name for name, m in MESHES.items() if m[1].shape[0] <= 10_000]


@functools.lru_cache(maxsize=None)
def _rays(name):
    v, i, ids, edge = MESHES[name]
    return rr.mesh_rays(v, i, NRAYS, seed=len(name) + i.shape[0])


@functools.lru_cache(maxsize=None)
def _want(name):
    v, i, ids, edge = MESHES[name]
    return rr.cast_rays_ref(v, i, ids, _rays(name))


@pytest.mark.parametrize("name", SMALL)
def test_closest_hit_on_small_meshes(name):
    v, i, ids, edge = MESHES[name]
    assert {"comb", "duplicates", "custom_ids", "n1", "n2", "n3", "n63", "n64", "n65"} <= set(SMALL)
    want = _want(name)
    with _ctx(v, i, ids) as cd:
        got = _cast(cd, _rays(name))
        _same(got, want, name)
        info = got[5]
        assert info.tri_tests >= info.n_hits and (i.shape[0] == 1 or info.node_visits > 0)
        if i.shape[0] == 1:
            assert info.tri_tests == NRAYS and info.node_visits == 0
    nh = int((want[0] != MISS).sum())
    print(f"{name}: {nh} of {NRAYS} rays hit, {info.node_visits / NRAYS:.1f} boxes and {info.tri_tests / NRAYS:.2f} ray_tri a ray")
    assert nh > NRAYS // 8 or i.shape[0] < 4, (name, nh)


@pytest.mark.parametrize("name", ["cloth300", "soup100k"])
def test_closest_hit_on_large_meshes_against_all_pairs(name):
    v, i, ids, edge = MESHES[name]
    with _ctx(v, i, ids) as cd:
        got = _cast(cd, _rays(name))
    _same(got, _want(name), name)
    assert int((got[0] != MISS).sum()) > NRAYS // 8


@pytest.mark.parametrize("n", [2, 3, 65])
def test_a_walk_that_must_visit_every_node(n):
    """n coincident triangles, each on vertices of its own, default IDs: all boxes of the tree are one box, so a ray that enters one
    subtree enters all.  Closest-hit rays straight down through the interior: every triangle is hit at the same t, the box test is
    closed at t_best, so every ray tests all n triangles, visits every node but the root once -- 2 n - 2 boxes, the most a walk over
    a tree makes -- and reports the smallest ID."""
    v = np.tile(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (n, 1))
    i = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    g = np.linspace(0.125, 0.375, 8)
    o = np.array([[x, y, 1.0] for x in g for y in g])
    r = o.shape[0]
    with _ctx(v, i) as cd:
        face, ids, t, uv, side, info = cd.cast_rays(o, np.tile([0.0, 0.0, -1.0], (r, 1)))
    print(f"{n} coincident triangles, {r} rays: {info.node_visits / r:.1f} boxes and {info.tri_tests / r:.2f} ray_tri a ray")
    assert (face == 0).all() and (ids == 0).all() and (t == 1.0).all() and info.n_hits == r
    assert info.tri_tests == r * n
    assert info.node_visits == r * (2 * n - 2)


def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def test_independent_of_frame_traversal_build_and_ray_order():
    name = "soup10k"
    v, i, ids, edge = MESHES[name]
    rays, want = _rays(name), _want(name)
    perm = np.random.default_rng(4).permutation(NRAYS)
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
                    _same(_cast(cd, rays), want, what)
                    g = _cast(cd, rays[perm])
                    _same(g[:5], tuple(w[perm] for w in want), what + ", rays permuted")
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)
        cd.set_morton_frame(mi355cd.CD_FRAME_REFERENCE)
        cd.build_tree()                                                    # the staged build (morton_sort, build_hierarchy, refit_boxes inside)
        _same(_cast(cd, rays), want, "build_tree")
    name = "cloth100d"                                                     # full doubles: the cell table matters
    v, i, ids, edge = MESHES[name]
    rays, want = _rays(name), _want(name)
    with mi355cd.CollisionDetector(v, i) as cd:
        for table in (0, 1):
            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
            cd.self_collide(cap=CAP)
            _same(_cast(cd, rays), want, f"cell table {table}")


@pytest.mark.parametrize("name", ["soup10k", "cloth100", "duplicates", "comb", "n1", "n2", "n65"])
def test_any_hit_is_defined_where_it_is_defined(name):
    v, i, ids, edge = MESHES[name]
    rays, want = _rays(name), _want(name)
    tris = np.asarray(v, dtype=np.float64)[np.asarray(i).astype(np.int64)]
    with _ctx(v, i, ids) as cd:
        face, info = _cast(cd, rays, any_hit=True)
        assert np.array_equal(face != MISS, want[0] != MISS), name        # WHETHER there is a hit
        k = np.nonzero(face != MISS)[0]
        assert (face[k] < i.shape[0]).all()
        assert rr.ray_tri_np(rays[k], tris[face[k]])[0].all(), name        # the triangle returned is one ray_tri hits; WHICH one is not defined
        assert info.n_hits == k.size
        lib, r = cd.lib, np.ascontiguousarray(rays)
        buf = np.zeros(NRAYS, dtype=np.float64)
        rc = lib.cd_cast_rays(cd._ctx, r.ctypes.data_as(C.c_void_p), NRAYS, mi355cd.CD_RAY_ANY, face.ctypes.data_as(C.c_void_p), None,
                              buf.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc == mi355cd.CD_ERR_ARG and not buf.any()                  # an output other than face with CD_RAY_ANY


SCALE_MESHES = si.meshes()


@functools.lru_cache(maxsize=None)
def _scale_case(name):
    v, vidx, edge = SCALE_MESHES[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    rays = rr.mesh_rays(vv, vidx, NRAYS, seed=3)
    return vv, vidx, rays, rr.cast_rays_ref(vv, vidx, None, rays)


@pytest.mark.parametrize("k", BAND)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """Mesh and rays scaled by 2^k, past both fp32 ends: the k = 0 faces, IDs, u, v, side and t (t is scale-free when o and d scale
    together; tmax is a parameter value and stays)."""
    vv, vidx, rays, want = _scale_case(name)
    rs = rays.copy()
    rs[:, 0:6] = si.scaled(rays[:, 0:6], k)
    with _ctx(si.scaled(vv, k), vidx) as cd:
        _same(_cast(cd, rs), want, f"{name} 2^{k}")
    assert int((want[0] != MISS).sum()) > NRAYS // 8


@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_translated_mesh_gives_the_restatement(name):
    vv, vidx, rays, _ = _scale_case(name)
    off = 2.0 ** 20 + 0.37
    vt = vv + off
    rt = rr.mesh_rays(vt, vidx, NRAYS, seed=5)
    want = rr.cast_rays_ref(vt, vidx, None, rt)
    with _ctx(vt, vidx) as cd:
        _same(_cast(cd, rt), want, f"{name} translated")
    print(f"{name} translated: {int((want[0] != MISS).sum())} hits")


def test_leaves_the_context_as_it_was():
    """Modelled on test_between_gpu.py::test_leaves_both_contexts_as_they_were: statistics, the last pair list, a captured step,
    the proximity and CCD results; then proximity and CCD calls interleaved with ray calls."""
    v, i = synth.soup(20000, e=0.02, seed=21)
    x1 = np.asarray(v) + np.random.default_rng(1).normal(0.0, 0.005, np.shape(v))
    rays = rr.mesh_rays(v, i, NRAYS, seed=8)
    want = rr.cast_rays_ref(v, i, None, rays)
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
                  cd.find_proximity(0.004, cap=CAP), cd.find_ccd(x1, 0.004, cap=CAP))
        hint0 = cd.debug_get(mi355cd.CD_DBG_GET_ORDER_STATE)
        _same(_cast(cd, rays), want, "closest")
        _cast(cd, rays, any_hit=True)
        st0, sp0, tri0, px0, cc0 = before
        assert bytes(cd.stats()) == st0
        assert cd.debug_get(mi355cd.CD_DBG_GET_ORDER_STATE) == hint0
        assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == sp0
        assert np.array_equal(cd.collision_triangles()[0], tri0)
        for rnd in range(2):                                               # interleaved: each still gives its earlier result
            gp, gd = pr.sort_pairs(*cd.find_proximity(0.004, cap=CAP)[:2])
            wp, wd = pr.sort_pairs(px0[0], px0[1])
            assert np.array_equal(gp, wp) and np.array_equal(_bits(gd), _bits(wd))
            _same(_cast(cd, rays), want, f"closest after proximity {rnd}")
            g = cr.sort_pairs(*cd.find_ccd(x1, 0.004, cap=CAP)[:3])
            w = cr.sort_pairs(*cc0[:3])
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(g, w))
            _same(_cast(cd, rays), want, f"closest after ccd {rnd}")
        rep0 = cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
        p, n, rc = cd.self_collide(cap=CAP)                                # the next self step still replays, and matches the oracle
        assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + 1 and cd.stats().traverse_launches == 0
        assert rc == mi355cd.CD_OK and np.array_equal(oracle.pair_set(p), oracle.pair_set(ref["pairs"]))
        _same(_cast(cd, rays), want, "closest after a replayed step")


def test_order_and_argument_errors_write_nothing():
    v, i, ids, edge = MESHES["soup10k"]
    rays = np.ascontiguousarray(_rays("soup10k")[:64])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    with mi355cd.CollisionDetector(v, i) as cd:
        lib = cd.lib
        outs = lambda: (np.full(64, 7, np.uint32), np.full(64, 7, np.uint32), np.full(64, 7.0), np.full((64, 2), 7.0), np.full(64, 7, np.uint8))
        def call(r, n=64, flags=0, o=None):
            o = outs() if o is None else o
            rc = lib.cd_cast_rays(cd._ctx, vp(r) if r is not None else None, n, flags, *(vp(x) for x in o), None)
            return rc, o
        untouched = lambda o: all((x == 7).all() for x in o)
        rc, o = call(rays)
        assert rc == mi355cd.CD_ERR_ORDER and untouched(o)                 # before a build
        cd.build_tree()
        assert call(rays)[0] == mi355cd.CD_OK
        for col, val in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (4, np.inf), (6, np.nan), (6, -1.0), (6, -np.inf)):
            bad = rays.copy(); bad[63, col] = val                          # the LAST ray: nothing may have been launched for the others
            rc, o = call(bad)
            assert rc == mi355cd.CD_ERR_ARG and untouched(o), (col, val)
        bad = rays.copy(); bad[5, 3:6] = 0.0
        rc, o = call(bad)
        assert rc == mi355cd.CD_ERR_ARG and untouched(o)
        bad = rays.copy(); bad[5, 3:6] = [0.0, -0.0, 0.0]
        assert call(bad)[0] == mi355cd.CD_ERR_ARG
        assert call(None)[0] == mi355cd.CD_ERR_ARG
        assert lib.cd_cast_rays(cd._ctx, vp(rays), 64, 0, None, None, None, None, None, None) == mi355cd.CD_ERR_ARG
        assert call(rays, flags=2)[0] == mi355cd.CD_ERR_ARG
        rc, o = call(rays, flags=mi355cd.CD_RAY_ANY)
        assert rc == mi355cd.CD_ERR_ARG and untouched(o)
        assert lib.cd_cast_rays(None, vp(rays), 64, 0, vp(o[0]), None, None, None, None, None) == mi355cd.CD_ERR_ARG
        assert call(None, n=0)[0] == mi355cd.CD_OK                         # n = 0
        rc, o = call(rays, n=0)
        assert rc == mi355cd.CD_OK and untouched(o)
        face = np.zeros(64, np.uint32)                                     # every output except face may be NULL
        assert lib.cd_cast_rays(cd._ctx, vp(rays), 64, 0, vp(face), None, None, None, None, None) == mi355cd.CD_OK
        assert np.array_equal(face, _want("soup10k")[0][:64])
        zero_t = rays.copy(); zero_t[:, 6] = 0.0                           # tmax = 0 and +inf are values, not errors
        assert call(zero_t)[0] == mi355cd.CD_OK
        cd.update_vertices(np.asarray(v) + 0.001)
        rc, o = call(rays)
        assert rc == mi355cd.CD_ERR_ORDER and untouched(o)                 # after update_vertices without a rebuild
        cd.build_tree()
        rc, o = call(rays)
        assert rc == mi355cd.CD_OK
        _same(o, rr.cast_rays_ref(np.asarray(v) + 0.001, i, ids, rays), "after update_vertices and a rebuild")   # the moved mesh's answers, not the old tree's


def test_buffers_grow_from_one_ray_to_a_million_and_back():
    v, i, ids, edge = MESHES["soup10k"]
    rays, want = _rays("soup10k"), _want("soup10k")
    big = np.ascontiguousarray(np.tile(rays, ((1 << 20) // NRAYS, 1)))
    with _ctx(v, i) as cd:
        _same(_cast(cd, rays[:1])[:5], tuple(w[:1] for w in want), "1 ray")
        g = _cast(cd, big)
        assert g[5].n_hits == ((1 << 20) // NRAYS) * int((want[0] != MISS).sum())
        for rep in (0, 1, (1 << 20) // NRAYS - 1):
            _same(tuple(x[rep * NRAYS:(rep + 1) * NRAYS] for x in g[:5]), want, f"2^20 rays, copy {rep}")
        _same(_cast(cd, rays[:1])[:5], tuple(w[:1] for w in want), "1 ray again")
        _same(_cast(cd, rays[:65])[:5], tuple(w[:65] for w in want), "65 rays")
        _same(_cast(cd, rays), want, "4096 rays")


def test_depth_frame():
    """A 256 x 256 pinhole camera over cloth_pair(100): the depth image (t per pixel) and everything else, pixel for pixel."""
    v, i = synth.cloth_pair(100)
    rays = rr.pinhole(eye=[1.5, 2.5, 0.75], target=[1.5, -0.1, 0.75], up=[0.0, 0.0, 1.0], fov_deg=70.0, res=256)
    want = rr.cast_rays_ref(v, i, None, rays)
    with _ctx(v, i) as cd:
        got = _cast(cd, rays)
    _same(got, want, "depth frame")
    depth = got[2].reshape(256, 256)
    hit = np.isfinite(depth)
    print(f"depth frame: {int(hit.sum())} of {256 * 256} pixels see the cloth, depth {depth[hit].min():.3f} .. {depth[hit].max():.3f} (in units of |d|)")
    assert hit[96:160, 96:160].all() and not hit.all()                    # the cloth fills the middle and leaves a border
