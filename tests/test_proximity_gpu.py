"""Self-proximity on the device (cd_find_proximity / cd_self_proximity / cd_tri_distance_points) against the CPU
restatement (tests/proximity_ref.py): the pair set AND every distance bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import contact_inputs
import mi355_synth as synth
import mi355cd
import oracle
import proximity_ref as pr
from query_meshes import _comb, _meshes  # noqa: F401  (the CCD and swept-tree tests take them from here too)

pytestmark = pytest.mark.gpu


def _bits(d):
    return np.asarray(d, dtype=np.float64).view(np.uint64)


def _same(got, want):
    gp, gd = pr.sort_pairs(got[0], got[1])
    wp, wd = want
    assert gp.shape == wp.shape, (gp.shape, wp.shape)
    assert np.array_equal(gp, wp)
    assert np.array_equal(_bits(gd), _bits(wd))


def _extra_pairs(n, seed):
    g = np.random.default_rng(seed)
    out = []
    a = g.uniform(-1, 1, (n, 6, 3)); a[:, 3:] += g.uniform(-1.5, 1.5, (n, 1, 3)); out.append(a)
    d = g.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = np.zeros((n, 6, 3)); o = g.normal(size=(n, 3)) * 1e-3
    b[:, 1] = d; b[:, 2] = 0.5 * d + g.normal(size=(n, 3)) * 0.3
    b[:, 3] = o + 0.2 * d; b[:, 4] = o + 0.2 * d + d + g.normal(size=(n, 3)) * 1e-9; b[:, 5] = o + d + g.normal(size=(n, 3)) * 0.3
    out.append(b)
    c = g.uniform(-1, 1, (n, 6, 3)); c[:, :, 2] = 0.25; c[:, 3:, 0] += g.uniform(0, 3, (n, 1)); out.append(c)
    dg = a.copy(); k = n // 3
    dg[:k, 1] = dg[:k, 0]; dg[k:2 * k, 2] = dg[k:2 * k, 0] + 0.37 * (dg[k:2 * k, 1] - dg[k:2 * k, 0])
    dg[2 * k:, 4] = dg[2 * k:, 3]; dg[2 * k:, 5] = dg[2 * k:, 3]; out.append(dg)
    out.append(a * 1e100); out.append(a * 1e-100); out.append(a.astype(np.float32).astype(np.float64))
    return np.concatenate(out)


def test_tri_distance_pin():
    t, _ = contact_inputs.tri_pairs()
    t = np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1, 6, 3), _extra_pairs(40000, 3)])
    assert t.shape[0] >= 1_000_000
    got = mi355cd.tri_distance_points(t)
    want = pr.tri_distance_np(t)
    assert np.all(np.isfinite(got))
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("name,verts,vidx,ids,edge", list(_meshes()), ids=lambda x: x if isinstance(x, str) else "")
def test_proximity_matches_restatement(name, verts, vidx, ids, edge):
    big = name in ("soup100k", "cloth300", "cloth300d")
    dists = [0.0, edge / 10] + ([] if big else [edge])
    with mi355cd.CollisionDetector(verts, vidx, ids) as cd:
        for k, d in enumerate(dists):
            want = pr.proximity_pairs(verts, vidx, ids, d)
            if k == 0:
                got = cd.self_proximity(d, cap=max(1, 2 * want[0].shape[0]))
            else:
                got = cd.find_proximity(d, cap=max(1, 2 * want[0].shape[0]))
            assert got[3] == mi355cd.CD_OK and got[2] == want[0].shape[0], (name, d, got[2], want[0].shape[0])
            _same(got, want)
            got = cd.self_proximity(d, cap=max(1, 2 * want[0].shape[0]))
            _same(got, want)
        if vidx.shape[0] >= 64:                                          # a cap that overflows
            d = edge / 2
            full = cd.find_proximity(d, cap=1 << 22)
            assert full[3] == mi355cd.CD_OK
            cap = max(1, full[2] // 3)
            part = cd.find_proximity(d, cap=cap)
            assert part[3] == mi355cd.CD_OVERFLOW and part[2] == full[2] and part[0].shape[0] == cap
            fs = set(map(tuple, full[0].tolist()))
            assert all(tuple(p) in fs for p in part[0].tolist())


@pytest.fixture(scope="module")
def cloth1m():
    return synth.cloth_pair(500)


def test_invariants_on_1m_cloth(cloth1m):
    verts, vidx = cloth1m
    dists = [0.0, 0.0005, 0.001, 0.003]
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cpairs, cn, crc = cd.self_collide(cap=1 << 22)
        assert crc == mi355cd.CD_OK
        sets, results = [], []
        for d in dists:
            p, dd, n, rc = cd.find_proximity(d, cap=1 << 24)
            assert rc == mi355cd.CD_OK and n == p.shape[0]
            assert np.all(dd <= d)
            assert np.all(p[:, 0] <= p[:, 1])
            s = oracle.pair_set(p)
            assert np.unique(s).shape[0] == s.shape[0]                     # each pair once
            sets.append(s); results.append((p, dd))
        assert np.all(np.isin(oracle.pair_set(cpairs), sets[0]))          # proximity(0) contains every collision
        for a, b in zip(sets, sets[1:]):
            assert np.all(np.isin(a, b))                                   # monotone in dist
        # every returned distance is the pinned function's on that pair (A = the smaller ID)
        p, dd = results[2]
        sel = p[np.random.default_rng(0).choice(p.shape[0], min(200_000, p.shape[0]), replace=False)]
        tv = verts[vidx.astype(np.int64)]
        keys = (p[:, 0].astype(np.uint64) << np.uint64(32)) | p[:, 1].astype(np.uint64)
        order = np.argsort(keys); ps = keys[order]; ds = dd[order]
        key = (sel[:, 0].astype(np.uint64) << np.uint64(32)) | sel[:, 1].astype(np.uint64)
        want = ds[np.searchsorted(ps, key)]
        got = mi355cd.tri_distance_points(np.concatenate([tv[sel[:, 0]], tv[sel[:, 1]]], axis=1))
        assert np.array_equal(_bits(got), _bits(want))
        # the restatement on every pair touching 2 000 random query triangles
        q = np.random.default_rng(5).choice(vidx.shape[0], 2000, replace=False)
        for k, d in enumerate(dists):
            wp, wd = pr.proximity_pairs(verts, vidx, None, d, queries=q)
            p, dd = results[k]
            touch = np.isin(p[:, 0], q) | np.isin(p[:, 1], q)
            _same((p[touch], dd[touch]), (wp, wd))
        # the same set whatever the traversal, the frame and the build
        ref = {d: sets[k] for k, d in enumerate(dists)}
        for setup in ("trav0", "trav1", "auto", "stagewise"):
            if setup == "trav0":
                cd.set_option(mi355cd.CD_OPT_TRAVERSAL, 0)
            elif setup == "trav1":
                cd.set_option(mi355cd.CD_OPT_TRAVERSAL, 1)
            elif setup == "auto":
                cd.set_option(mi355cd.CD_OPT_TRAVERSAL, 3); cd.set_morton_frame(mi355cd.CD_FRAME_AUTO)
            else:
                cd.set_morton_frame(mi355cd.CD_FRAME_REFERENCE); cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 1)
            for d in (0.0, 0.003):
                p, dd, n, rc = cd.self_proximity(d, cap=1 << 24)
                assert rc == mi355cd.CD_OK and np.array_equal(oracle.pair_set(p), ref[d]), (setup, d)


def test_degenerate_pair_far_apart():
    """A point triangle and a segment triangle far apart: the 17-axis test says "contact" (every axis between them is zero), but
    their boxes are disjoint, so they are not in contact: tri_distance is their Euclidean distance and no small dist reports them."""
    verts = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [12, 0, 5], [12, 10, 5], [12, 5, 5],
                      [30, 30, 30], [31, 30, 30], [30, 31, 30]], dtype=np.float64)
    vidx = np.arange(9, dtype=np.uint32).reshape(3, 3)
    tri = np.concatenate([verts[vidx[0]], verts[vidx[1]]])[None]
    assert mi355cd.tri_contact_points(tri)[0] == 1
    assert mi355cd.tri_distance_points(tri)[0] == 13.0
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        for d in (0.0, 1.0, 12.9):
            p, dd, n, rc = cd.self_proximity(d)
            assert rc == mi355cd.CD_OK and n == 0, (d, p)
        p, dd, n, rc = cd.find_proximity(13.0)
        assert rc == mi355cd.CD_OK and p.tolist() == [[0, 1]] and dd.tolist() == [13.0]


def test_cell_table_does_not_change_the_result():
    verts, vidx = synth.cloth_pair(100, round_f32=False)
    out = []
    for table in (1, 0):
        with mi355cd.CollisionDetector(verts, vidx) as cd:
            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
            p, dd, n, rc = cd.self_proximity(0.01)
            out.append(pr.sort_pairs(p, dd))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))


def test_order_errors():
    verts, vidx = synth.soup(2000, e=0.05, seed=2)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        with pytest.raises(mi355cd.CdError) as e:
            cd.find_proximity(0.01)
        assert e.value.rc == mi355cd.CD_ERR_ORDER
        cd.build_tree()
        assert cd.find_proximity(0.01)[3] == mi355cd.CD_OK
        cd.update_vertices(verts)
        with pytest.raises(mi355cd.CdError) as e:
            cd.find_proximity(0.01)
        assert e.value.rc == mi355cd.CD_ERR_ORDER


@pytest.mark.parametrize("graph", [0, 1])
def test_collision_results_unchanged(graph):
    verts, vidx = synth.soup(20000, e=0.05, seed=3)
    ref = oracle.pipeline(verts, vidx)
    want = oracle.pair_set(ref["pairs"])
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        if graph:
            cd.set_option(mi355cd.CD_OPT_GRAPH, 1)
            cd.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)
            cd.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
        for _ in range(3):
            pairs, n, rc = cd.self_collide(cap=1 << 16)
        assert rc == 0 and np.array_equal(oracle.pair_set(pairs), want)
        if graph:                                                          # the step has been captured once and is being replayed
            caps0, reps0 = cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES), cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
            assert caps0 >= 1 and reps0 >= 1
        st0 = cd.stats()
        sp0 = cd.sorted_pairs(cap=1 << 16)
        ct0 = cd.collision_triangles(cap=1 << 17)
        pp = cd.find_proximity(0.01)
        assert pp[3] == 0 and pp[2] > n
        pp = cd.self_proximity(0.01)
        assert pp[3] == 0
        st1 = cd.stats()
        for f, _ in mi355cd.CdStats._fields_:
            assert getattr(st0, f) == getattr(st1, f), f
        sp1 = cd.sorted_pairs(cap=1 << 16)
        ct1 = cd.collision_triangles(cap=1 << 17)
        assert np.array_equal(sp0[0], sp1[0]) and sp0[1] == sp1[1]
        assert np.array_equal(ct0[0], ct1[0])
        for _ in range(3):
            pairs, n, rc = cd.self_collide(cap=1 << 16)
            assert rc == 0 and np.array_equal(oracle.pair_set(pairs), want)
        assert cd.stats().pairs_tested == ref["stats"].pairs_tested
        if graph:                                                          # the captured step survived: replayed again, never recaptured
            assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES) == caps0
            assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == reps0 + 3
            assert cd.stats().traverse_launches == 0
