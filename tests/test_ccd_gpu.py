"""Continuous collision queries on the device (cd_find_ccd / cd_self_ccd / cd_ccd_points) against the CPU restatement
(tests/ccd_ref.py): the pair set, every time of contact and every distance bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ccd_ref as cr
import mi355_synth as synth
import mi355cd
import oracle
import proximity_ref as pr
from test_proximity_gpu import _meshes

pytestmark = pytest.mark.gpu


def _bits(d):
    return np.asarray(d, dtype=np.float64).view(np.uint64)


def _same(got, want):
    gp, gt, gd = cr.sort_pairs(got[0], got[1], got[2])
    wp, wt, wd = want
    assert gp.shape == wp.shape, (gp.shape, wp.shape)
    assert np.array_equal(gp, wp)
    assert np.array_equal(_bits(gt), _bits(wt))
    assert np.array_equal(_bits(gd), _bits(wd))


def _pin_pairs(seed=17):
    """2^18 moving pairs: most take a few evaluations; 16 384 fast tumbling pairs spread over 1 .. CCD_MAX_EVALS, some unresolved."""
    g = np.random.default_rng(seed)
    n_easy, n_hard = (1 << 18) - 16384, 16384
    a = g.uniform(-1, 1, (n_easy, 3, 3)); b = g.uniform(-1, 1, (n_easy, 3, 3))
    off = g.normal(size=(n_easy, 1, 3)); off *= g.uniform(0.5, 3.0, (n_easy, 1, 1)) / np.linalg.norm(off, axis=2, keepdims=True)
    easy = np.concatenate([a, b + off, a + g.normal(size=(n_easy, 1, 3)) * 0.2, b - off + g.normal(size=(n_easy, 3, 3)) * 0.05], axis=1)
    k = n_easy // 8
    easy[:k, 6:] = easy[:k, :6]                                           # no motion
    easy[k:2 * k, [1, 7]] = easy[k:2 * k, [0, 6]]                          # degenerate
    a = g.uniform(-0.05, 0.05, (n_hard, 3, 3)); b = g.uniform(-0.05, 0.05, (n_hard, 3, 3)) + np.array([0.4, 0.0, 0.0])
    spin = 10.0 ** g.uniform(-1.5, 1.5, (n_hard, 1, 1))
    hard = np.concatenate([a, b, a + g.normal(size=(n_hard, 3, 3)) * spin, b + g.normal(size=(n_hard, 3, 3)) * spin], axis=1)
    return np.concatenate([easy, hard])


def test_ccd_points_pin():
    tri = _pin_pairs()
    assert tri.shape[0] >= 1 << 18
    for dist in (0.01,):
        got = mi355cd.ccd_points(tri, dist)
        want = cr.advance_np(tri, dist)
        for gg, ww, name in zip(got, want, ("toi", "d", "evals")):
            if name == "evals":
                bad = np.nonzero(gg != ww)[0]
            else:
                bad = np.nonzero(_bits(gg) != _bits(ww))[0]
            assert bad.size == 0, (name, bad.size, bad[:5], gg[bad[:5]], ww[bad[:5]])
        ev = got[2]
        assert ev.min() == 1 and ev.max() == cr.MAX_EVALS
        assert np.unique(ev).size > 200
        unres = np.isfinite(got[0]) & (got[1] > dist)
        assert unres.sum() > 0 and np.all(ev[unres] == cr.MAX_EVALS)


def _move(verts, edge, seed):
    g = np.random.default_rng(seed)
    return verts + g.normal(size=verts.shape) * edge * 0.3 + g.normal(size=(1, 3)) * edge


@pytest.mark.parametrize("name,verts,vidx,ids,edge", [m for m in _meshes() if m[0] not in ("soup100k", "cloth300", "cloth300d")],
                         ids=lambda x: x if isinstance(x, str) else "")
def test_ccd_matches_restatement(name, verts, vidx, ids, edge):
    x1 = _move(verts, edge, 3)
    with mi355cd.CollisionDetector(verts, vidx, ids) as cd:
        for k, d in enumerate((edge / 10, edge / 2)):
            want, (tested, evals) = cr.ccd_pairs(verts, x1, vidx, ids, d, counts=True)
            cap = max(1, 2 * want[0].shape[0])
            got = cd.self_ccd(x1, d, cap=cap) if k == 0 else cd.find_ccd(x1, d, cap=cap)
            assert got[4] == mi355cd.CD_OK and got[3] == want[0].shape[0], (name, d, got[3], want[0].shape[0])
            _same(got, want)
            info = cd.ccd_info
            assert info.n_tested == tested and info.n_evals == evals, (info.n_tested, tested, info.n_evals, evals)
            assert info.n_candidates >= tested
            _same(cd.find_ccd(x1, d, cap=cap), want)


def test_tunnelling():
    """Two small triangles pass through each other inside the step: apart at both ends, so neither the collision path nor
    proximity sees them; continuous collision reports the pair with a time strictly inside the step."""
    a = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    b = np.array([[0.2, 0.2, 1.0], [0.6, 0.2, 1.0], [0.2, 0.6, 1.2]])
    verts = np.concatenate([a, b]); vidx = np.arange(6, dtype=np.uint32).reshape(2, 3)
    x1 = verts.copy(); x1[3:, 2] -= 2.5
    dist = 0.01
    for v in (verts, x1):
        with mi355cd.CollisionDetector(v, vidx) as cd:
            assert cd.self_collide()[1] == 0
            assert cd.self_proximity(dist)[2] == 0
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        p, toi, dd, n, rc = cd.find_ccd(x1, dist)
        assert rc == mi355cd.CD_OK and p.tolist() == [[0, 1]]
        assert 0.0 < toi[0] < 1.0 and dd[0] <= dist
        assert (1.0 - dist) / 2.5 <= toi[0] <= (1.0 - dist / 2) / 2.5
        _same((p, toi, dd), cr.ccd_pairs(verts, x1, vidx, None, dist))


@pytest.fixture(scope="module")
def cloth1m():
    return synth.cloth_pair(500)


def _key(p):
    return oracle.pair_set(p)


def test_invariants_on_1m_cloth(cloth1m):
    verts, vidx = cloth1m
    dist = 0.001
    x1 = synth.cloth_motion(verts, approach=0.5, wave=0.5)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        p, toi, dd, n, rc = cd.find_ccd(x1, dist, cap=1 << 24)
        assert rc == mi355cd.CD_OK and n == p.shape[0] and n > 0
        assert np.all((toi >= 0.0) & (toi <= 1.0))
        s = _key(p)
        assert np.unique(s).shape[0] == s.shape[0]
        # toi == 0: exactly proximity on x0, with the same distances
        pp, pd, pn, prc = cd.find_proximity(dist, cap=1 << 24)
        sp, sd = pr.sort_pairs(pp, pd)
        z = toi == 0.0
        _same((p[z], toi[z], dd[z]), (sp, np.zeros(sp.shape[0]), sd))
        # x1 == x0: identical to proximity
        q, qt, qd, qn, qrc = cd.find_ccd(verts, dist, cap=1 << 24)
        _same((q, qt, qd), (sp, np.zeros(sp.shape[0]), sd))
        # the restatement on every pair touching 2 000 random query triangles
        qsel = np.random.default_rng(5).choice(vidx.shape[0], 2000, replace=False)
        want = cr.ccd_pairs(verts, x1, vidx, None, dist, queries=qsel)
        touch = np.isin(p[:, 0], qsel) | np.isin(p[:, 1], qsel)
        _same((p[touch], toi[touch], dd[touch]), want)
        # the same set whatever the traversal, the frame and the build
        for setup in ("trav0", "trav1", "auto", "stagewise"):
            if setup == "trav0":
                cd.set_option(mi355cd.CD_OPT_TRAVERSAL, 0)
            elif setup == "trav1":
                cd.set_option(mi355cd.CD_OPT_TRAVERSAL, 1)
            elif setup == "auto":
                cd.set_option(mi355cd.CD_OPT_TRAVERSAL, 3); cd.set_morton_frame(mi355cd.CD_FRAME_AUTO)
            else:
                cd.set_morton_frame(mi355cd.CD_FRAME_REFERENCE); cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 1)
            got = cd.self_ccd(x1, dist, cap=1 << 24)
            assert got[4] == mi355cd.CD_OK and np.array_equal(_key(got[0]), s), setup
            _same(got[:3], cr.sort_pairs(p, toi, dd))
    # every proximity pair at the end state is reported
    with mi355cd.CollisionDetector(x1, vidx) as cd1:
        ep = cd1.self_proximity(dist, cap=1 << 24)
        assert ep[3] == mi355cd.CD_OK
        assert np.all(np.isin(_key(ep[0]), s))


def test_broad_phase_stays_local(cloth1m):
    verts, vidx = cloth1m
    dist = 0.001
    x1 = synth.cloth_motion(verts, approach=0.5, wave=0.5)
    x1t = synth.cloth_motion(verts, approach=0.5, wave=0.5, throw=True)
    k = np.nonzero(np.any(x1t != x1, axis=1))[0]
    assert k.size == 1
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        base = cd.find_ccd(x1, dist, cap=1 << 24)
        c0 = cd.ccd_info.n_candidates
        thrown = cd.find_ccd(x1t, dist, cap=1 << 24)
        c1 = cd.ccd_info.n_candidates
        assert base[4] == thrown[4] == mi355cd.CD_OK
    tris = np.nonzero(np.any(vidx == k[0], axis=1))[0]
    _, (gate, _) = cr.ccd_pairs(verts, x1t, vidx, None, dist, queries=tris, counts=True)
    assert gate > 0
    assert c1 - c0 <= 4 * gate + 1000, (c0, c1, gate)


def test_errors():
    verts, vidx = synth.soup(2000, e=0.05, seed=2)
    x1 = verts + 0.01
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        with pytest.raises(mi355cd.CdError) as e:
            cd.find_ccd(x1, 0.01)
        assert e.value.rc == mi355cd.CD_ERR_ORDER
        cd.build_tree()
        for bad in (0.0, -0.01, float("nan"), float("inf")):
            with pytest.raises(mi355cd.CdError) as e:
                cd.find_ccd(x1, bad)
            assert e.value.rc == mi355cd.CD_ERR_ARG
        n = C.c_uint64(0)
        assert cd.lib.cd_find_ccd(cd._ctx, None, 0.01, None, None, None, 0, C.byref(n), None) == mi355cd.CD_ERR_ARG
        full = cd.find_ccd(x1, 0.02, cap=1 << 22)
        assert full[4] == mi355cd.CD_OK and full[3] > 10
        cap = full[3] // 3
        part = cd.find_ccd(x1, 0.02, cap=cap)
        assert part[4] == mi355cd.CD_OVERFLOW and part[3] == full[3] and part[0].shape[0] == cap
        fs = set(map(tuple, full[0].tolist()))
        assert all(tuple(q) in fs for q in part[0].tolist())
        assert cd.lib.cd_find_ccd(cd._ctx, x1.ctypes.data, 0.02, None, None, None, 0, C.byref(n), None) == mi355cd.CD_OVERFLOW
        assert n.value == full[3]
        cd.update_vertices(verts)
        with pytest.raises(mi355cd.CdError) as e:
            cd.find_ccd(x1, 0.01)
        assert e.value.rc == mi355cd.CD_ERR_ORDER


@pytest.mark.parametrize("graph", [0, 1])
def test_side_effects(graph):
    verts, vidx = synth.soup(20000, e=0.05, seed=3)
    x1 = _move(verts, 0.05, 4)
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
        if graph:
            caps0, reps0 = cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES), cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
            assert caps0 >= 1 and reps0 >= 1
        st0 = cd.stats()
        sp0 = cd.sorted_pairs(cap=1 << 16)
        ct0 = cd.collision_triangles(cap=1 << 17)
        px0 = pr.sort_pairs(*cd.find_proximity(0.01)[:2])
        cc = cd.find_ccd(x1, 0.01)
        assert cc[4] == 0 and cc[3] > 0
        cc = cd.self_ccd(x1, 0.01)
        assert cc[4] == 0
        st1 = cd.stats()
        for f, _ in mi355cd.CdStats._fields_:
            assert getattr(st0, f) == getattr(st1, f), f
        sp1 = cd.sorted_pairs(cap=1 << 16)
        ct1 = cd.collision_triangles(cap=1 << 17)
        assert np.array_equal(sp0[0], sp1[0]) and sp0[1] == sp1[1]
        assert np.array_equal(ct0[0], ct1[0])
        px1 = pr.sort_pairs(*cd.find_proximity(0.01)[:2])
        assert np.array_equal(px0[0], px1[0]) and np.array_equal(_bits(px0[1]), _bits(px1[1]))
        px2 = pr.sort_pairs(*cd.self_proximity(0.01)[:2])                  # rebuilt from the context's vertices: still x0
        assert np.array_equal(px0[0], px2[0]) and np.array_equal(_bits(px0[1]), _bits(px2[1]))
        for _ in range(3):
            pairs, n, rc = cd.self_collide(cap=1 << 16)
            assert rc == 0 and np.array_equal(oracle.pair_set(pairs), want)
        assert cd.stats().pairs_tested == ref["stats"].pairs_tested
        if graph:
            assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES) == caps0
            assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == reps0 + 3
