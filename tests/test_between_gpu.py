"""Queries between two meshes on the device (cd_find_collisions_between, cd_find_proximity_between, cd_find_ccd_between) against the
CPU restatement (tests/between_ref.py) and against the pinned self path on the merged mesh: pair sets and the bits of every distance
and toi."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import between_ref as br
import ccd_ref as cr
import mi355_synth as synth
import mi355cd
import oracle
import proximity_ref as pr
import scale_inputs as si

pytestmark = pytest.mark.gpu

CAP = 1 << 20


def _bits(d):
    return np.asarray(d, dtype=np.float64).view(np.uint64)


def _ctx(v, i, ids=None):
    cd = mi355cd.CollisionDetector(v, i, ids)
    cd.build_tree()
    return cd


def _same_contact(got, want, what):
    p, n, rc = got
    wp = want
    assert rc == mi355cd.CD_OK and n == wp.shape[0], (what, n, wp.shape[0])
    assert np.array_equal(oracle.pair_set(p), oracle.pair_set(wp)), what


def _same_prox(got, want, what):
    gp, gd = pr.sort_pairs(got[0], got[1])
    wp, wd = want
    assert got[3] == mi355cd.CD_OK and got[2] == wp.shape[0], (what, got[2], wp.shape[0])
    assert np.array_equal(gp, wp), what
    bad = np.nonzero(_bits(gd) != _bits(wd))[0]
    assert bad.size == 0, (what, bad.size, gd[bad[:3]], wd[bad[:3]])


def _same_ccd(got, want, what):
    gp, gt, gd = cr.sort_pairs(got[0], got[1], got[2])
    wp, wt, wd = want
    assert got[4] == mi355cd.CD_OK and got[3] == wp.shape[0], (what, got[3], wp.shape[0])
    assert np.array_equal(gp, wp), what
    assert np.array_equal(_bits(gt), _bits(wt)), what
    assert np.array_equal(_bits(gd), _bits(wd)), what


def _cases():
    out = {}
    for na, nb, e, seed in ((1, 1, 0.5, 1), (1, 400, 0.15, 2), (400, 1, 0.15, 3), (2, 600, 0.12, 4), (700, 900, 0.06, 5), (1500, 500, 0.05, 6)):
        v, i = br.soup(na + nb, e, seed)
        out[f"soup_{na}_{nb}_s{seed}"] = br.split(v, i, na)
    va, ia = br.soup(300, 0.05, 7, 0.0, 1.0)
    vb, ib = br.soup(300, 0.05, 8, 3.0, 4.0)
    out["disjoint"] = (va, ia, vb, ib)
    out["shared_positions"] = br.shared_positions(200, 9)
    v, i = br.with_degenerate(*br.soup(900, 0.1, 10), seed=10)
    out["degenerate"] = br.split(v, i, 400)
    return out


CASES = _cases()
DISTS = (0.0, 0.01, 0.08)
CCD_DIST = 0.01


@functools.lru_cache(maxsize=None)
def _want(name, swap=False):
    va, ia, vb, ib = CASES[name]
    if swap:
        va, ia, vb, ib = vb, ib, va, ia
    x1a, x1b = br.motion(va, 0.03, 11), br.motion(vb, 0.03, 12)
    contact = br.contact_pairs(va, ia, vb, ib)
    prox = {d: br.proximity_pairs(va, ia, vb, ib, d) for d in DISTS}
    ccd = {m: br.ccd_pairs(va, ia, vb, ib, CCD_DIST, x1a if m in ("both", "a") else None, x1b if m == "both" else None)
           for m in ("both", "a", "none")}
    prox_x1 = br.proximity_pairs(x1a, ia, x1b, ib, CCD_DIST)
    return dict(x1a=x1a, x1b=x1b, contact=contact, prox=prox, ccd=ccd, prox_x1=prox_x1)


def _check_all(a, b, w, what, x1a, x1b):
    p, n, rc = a.find_collisions_between(b, cap=CAP)
    _same_contact((p, n, rc), w["contact"][0], f"{what} contact")
    assert a.between_tested == w["contact"][1], (what, a.between_tested, w["contact"][1])
    for d in DISTS:
        _same_prox(a.find_proximity_between(b, d, cap=CAP), w["prox"][d], f"{what} proximity {d}")
    for m in ("both", "a", "none"):
        got = a.find_ccd_between(b, CCD_DIST, x1a if m in ("both", "a") else None, x1b if m == "both" else None, cap=CAP)
        _same_ccd(got, w["ccd"][m], f"{what} ccd {m}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_restatement(name):
    va, ia, vb, ib = CASES[name]
    w = _want(name)
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        _check_all(a, b, w, name, w["x1a"], w["x1b"])
        # consistency between the queries: proximity(0) holds every contact pair, at 0
        pc = oracle.pair_set(a.find_collisions_between(b, cap=CAP)[0])
        p0, d0, _, _ = a.find_proximity_between(b, 0.0, cap=CAP)
        s0 = oracle.pair_set(p0)
        assert np.isin(pc, s0).all() and np.all(d0 == 0.0), name
        # CCD pairs at toi 0 are proximity on x0 with the same distances; every proximity pair on x1 is in the CCD result
        cp, ct, cd, _, _ = a.find_ccd_between(b, CCD_DIST, w["x1a"], w["x1b"], cap=CAP)
        z = ct == 0.0
        _same_prox((cp[z], cd[z], int(z.sum()), mi355cd.CD_OK), w["prox"][CCD_DIST], f"{name} ccd toi 0")
    with _ctx(w["x1a"], ia) as a1, _ctx(w["x1b"], ib) as b1:
        p1, d1, n1, _ = a1.find_proximity_between(b1, CCD_DIST, cap=CAP)
        _same_prox((p1, d1, n1, mi355cd.CD_OK), w["prox_x1"], f"{name} proximity on x1")
        assert np.isin(oracle.pair_set(p1), oracle.pair_set(cp)).all(), name


@pytest.mark.parametrize("name", ["soup_2_600_s4", "soup_1500_500_s6", "shared_positions", "degenerate"])
def test_roles_swapped(name):
    va, ia, vb, ib = CASES[name]
    w = _want(name, swap=True)
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        _check_all(b, a, w, f"{name} swapped", w["x1a"], w["x1b"])


def test_cloth_pair_1m_against_self_path():
    """The two sheets of cloth_pair(500) as two contexts, b's IDs offset by nA: contact equals the cross pairs of cd_self_collide on the
    merged mesh, proximity at 0.0005 those of cd_find_proximity, distance bits included."""
    verts, vidx = synth.cloth_pair(500)
    nt, half = vidx.shape[0], verts.shape[0] // 2
    na = nt // 2
    assert vidx[:na].max() < half and vidx[na:].min() >= half
    va, ia, vb, ib = verts[:half], vidx[:na], verts[half:], (vidx[na:] - half).astype(np.uint32)
    idb = np.arange(nt - na, dtype=np.uint32) + na
    with mi355cd.CollisionDetector(verts, vidx) as m:
        sp, sn, rc = m.self_collide(cap=1 << 22)
        assert rc == mi355cd.CD_OK
        mp, md, mn, rc = m.find_proximity(0.0005, cap=1 << 21)
        assert rc == mi355cd.CD_OK
    sel = (sp[:, 0] < na) != (sp[:, 1] < na)
    want_c = np.sort(sp[sel], axis=1)
    mp, md = pr.sort_pairs(mp, md)
    sel = (mp[:, 0] < na) & (mp[:, 1] >= na)
    want_p = (mp[sel], md[sel])
    with _ctx(va, ia) as a, _ctx(vb, ib, idb) as b:
        _same_contact(a.find_collisions_between(b, cap=1 << 22), want_c, "cloth contact")
        assert want_c.shape[0] > 10000
        _same_prox(a.find_proximity_between(b, 0.0005, cap=1 << 21), want_p, "cloth proximity")


def _frame(cd, mode):
    if mode == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(mode, np.array([-0.3, -0.2, -0.25]), np.array([1.7, 1.5, 1.6]))
    else:
        cd.set_morton_frame(mode)


def test_independent_of_frames_traversal_and_cell_table():
    name = "soup_1500_500_s6"
    va, ia, vb, ib = CASES[name]
    w = _want(name)
    frames = (mi355cd.CD_FRAME_REFERENCE, mi355cd.CD_FRAME_AUTO, mi355cd.CD_FRAME_CUSTOM)
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:
        k = 0
        for fa in frames:
            for fb in frames:
                for trav in (0, 1, 3):
                    for table in (0, 1):
                        if (k := k + 1) % 3 and not (trav == 3 and table == 1):
                            continue                            # a third of the product, and every frame pair in the default setting
                        for cd, f in ((a, fa), (b, fb)):
                            cd.set_option(mi355cd.CD_OPT_TRAVERSAL, trav)
                            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
                            _frame(cd, f)
                            cd.self_collide(cap=CAP)                   # the tree of this setting (the collision step builds it)
                        _check_all(a, b, w, f"frames {fa}/{fb} traversal {trav} table {table}", w["x1a"], w["x1b"])


def test_leaves_both_contexts_as_they_were():
    va, ia = br.soup(20000, 0.02, 21)
    vb, ib = br.soup(20000, 0.02, 22)
    x1a, x1b = br.motion(va, 0.005, 1), br.motion(vb, 0.005, 2)
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:
        for cd in (a, b):                                    # what a captured step needs (graph_eligible)
            cd.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)
            cd.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
            cd.set_option(mi355cd.CD_OPT_GRAPH, 1)
        refs = {id(cd): oracle.pipeline(cd.verts, cd.vidx) for cd in (a, b)}
        for _ in range(3):                                   # capture, then replays
            for cd in (a, b):
                cd.self_collide(cap=CAP)
        before = {}
        for cd in (a, b):
            p, n, rc = cd.self_collide(cap=CAP)
            assert cd.stats().traverse_launches == 0, "the self step does not replay: nothing here would be tested"
            before[id(cd)] = (bytes(cd.stats()), oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes(),
                              cd.collision_triangles()[0], cd.find_proximity(0.004, cap=CAP), cd.find_ccd(x1a if cd is a else x1b, 0.004, cap=CAP))
        a.find_collisions_between(b, cap=CAP)
        a.find_proximity_between(b, 0.004, cap=CAP)
        a.find_ccd_between(b, 0.004, x1a, x1b, cap=CAP)
        b.find_ccd_between(a, 0.004, None, x1a, cap=CAP)
        for cd in (a, b):
            st0, sp0, tri0, px0, cc0 = before[id(cd)]
            assert bytes(cd.stats()) == st0
            assert oracle.pair_set(cd.sorted_pairs(cap=CAP)[0]).tobytes() == sp0
            assert np.array_equal(cd.collision_triangles()[0], tri0)
            _same_prox(cd.find_proximity(0.004, cap=CAP), pr.sort_pairs(px0[0], px0[1]), "proximity after the between calls")   # (rows unordered)
            _same_ccd(cd.find_ccd(x1a if cd is a else x1b, 0.004, cap=CAP), cr.sort_pairs(*cc0[:3]), "ccd after the between calls")
        for cd in (a, b):                                    # the next self step still replays, and matches the oracle
            rep0 = cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
            p, n, rc = cd.self_collide(cap=CAP)
            assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + 1 and cd.stats().traverse_launches == 0
            r = refs[id(cd)]
            assert rc == mi355cd.CD_OK and np.array_equal(oracle.pair_set(p), oracle.pair_set(r["pairs"]))


SCALE_MESHES = si.meshes()


@functools.lru_cache(maxsize=None)
def _scale_want(name):
    v, vidx, edge = SCALE_MESHES[name]
    k = vidx.shape[0] // 2
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    x1 = si.motion(vv, edge)
    ia, ib = vidx[:k], vidx[k:]
    # the split keeps the vertex array whole on both sides (unused vertices are allowed): indices stay as they are
    prox = {d: br.proximity_pairs(vv, ia, vv, ib, d) for d in (0.0, edge / 4)}
    ccd = br.ccd_pairs(vv, ia, vv, ib, edge / 4, x1, None)
    contact = br.contact_pairs(vv, ia, vv, ib)
    return vv, x1, ia, ib, edge, prox, ccd, contact


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """The tests/scale_inputs.py meshes split in two and scaled by 2^k: the same pairs, distances and toi bits times 2^k (toi unchanged)."""
    vv, x1, ia, ib, edge, prox, ccd, contact = _scale_want(name)
    v, y1 = si.scaled(vv, k), si.scaled(x1, k)
    with _ctx(v, ia) as a, _ctx(v, ib) as b:
        for d, (wp, wd) in prox.items():
            _same_prox(a.find_proximity_between(b, np.ldexp(d, k), cap=CAP), (wp, np.ldexp(wd, k)), f"{name} k={k} proximity {d}")
        cp, ct, cd = ccd
        _same_ccd(a.find_ccd_between(b, np.ldexp(edge / 4, k), y1, None, cap=CAP), (cp, ct, np.ldexp(cd, k)), f"{name} k={k} ccd")
        if -200 <= k <= 200:                                  # (the contact predicate is the reference's: unscaled products)
            _same_contact(a.find_collisions_between(b, cap=CAP), contact[0], f"{name} k={k} contact")


def test_overflow_keeps_the_cap_and_a_canary():
    name = "soup_700_900_s5"
    va, ia, vb, ib = CASES[name]
    wp, wd = _want(name)["prox"][0.08]
    n_true = wp.shape[0]
    assert n_true > 100
    cap = n_true // 3
    lib = mi355cd.load_library()
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        pairs = np.full((cap + 8, 2), 0xDEADBEEF, dtype=np.uint32)
        dists = np.full(cap + 8, -7.0)
        n, t = C.c_uint64(0), C.c_uint64(0)
        rc = lib.cd_find_proximity_between(a._ctx, b._ctx, 0.08, pairs.ctypes.data_as(C.c_void_p), dists.ctypes.data_as(C.c_void_p), cap,
                                           C.byref(n), C.byref(t))
        assert rc == mi355cd.CD_OVERFLOW and n.value == n_true
        assert np.all(pairs[cap:] == 0xDEADBEEF) and np.all(dists[cap:] == -7.0)
        got = oracle.pair_set(pairs[:cap])
        assert np.unique(got).shape[0] == cap and np.isin(got, oracle.pair_set(wp)).all()
        p, nn, rc = a.find_collisions_between(b, cap=1)
        wc = _want(name)["contact"][0].shape[0]
        assert (rc == mi355cd.CD_OVERFLOW) == (wc > 1) and nn == wc
        p, tt, dd, nn, rc = a.find_ccd_between(b, CCD_DIST, _want(name)["x1a"], _want(name)["x1b"], cap=2)
        assert rc == mi355cd.CD_OVERFLOW and nn == _want(name)["ccd"]["both"][0].shape[0] and p.shape[0] == 2


def test_candidate_shards_grow():
    """Two coincident dense meshes at a large dist: every a x b pair is a candidate, far more than the first candidate buffer holds."""
    va, ia = br.soup(800, 0.05, 31, 0.0, 0.2)
    vb, ib = va.copy(), ia.copy()
    d = 0.5
    want = br.proximity_pairs(va, ia, vb, ib, d)
    assert want[0].shape[0] == 800 * 800
    wc = br.ccd_pairs(va, ia, vb, ib, d, br.motion(va, 0.02, 1), None)
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        _same_prox(a.find_proximity_between(b, d, cap=1 << 20), want, "growth proximity")
        _same_ccd(a.find_ccd_between(b, d, br.motion(va, 0.02, 1), None, cap=1 << 20), wc, "growth ccd")
        _same_contact(a.find_collisions_between(b, cap=1 << 20), br.contact_pairs(va, ia, vb, ib)[0], "growth contact")


def test_errors():
    va, ia, vb, ib = CASES["soup_700_900_s5"]
    lib = mi355cd.load_library()
    n, t = C.c_uint64(0), C.c_uint64(0)
    info = mi355cd.CdCcdInfo()
    with _ctx(va, ia) as a, _ctx(vb, ib) as b:
        E = mi355cd.CD_ERR_ARG
        assert lib.cd_find_collisions_between(a._ctx, a._ctx, None, 0, C.byref(n), C.byref(t)) == E
        assert lib.cd_find_proximity_between(a._ctx, a._ctx, 0.1, None, None, 0, C.byref(n), C.byref(t)) == E
        assert lib.cd_find_ccd_between(a._ctx, None, a._ctx, None, 0.1, None, None, None, 0, C.byref(n), C.byref(info)) == E
        assert lib.cd_find_collisions_between(a._ctx, None, None, 0, C.byref(n), C.byref(t)) == E
        assert lib.cd_find_collisions_between(None, b._ctx, None, 0, C.byref(n), C.byref(t)) == E
        for d in (float("nan"), -1e-3, float("inf")):
            assert lib.cd_find_proximity_between(a._ctx, b._ctx, d, None, None, 0, C.byref(n), C.byref(t)) == E, d
            assert lib.cd_find_ccd_between(a._ctx, None, b._ctx, None, d, None, None, None, 0, C.byref(n), C.byref(info)) == E, d
        assert lib.cd_find_ccd_between(a._ctx, None, b._ctx, None, 0.0, None, None, None, 0, C.byref(n), C.byref(info)) == E
        with pytest.raises(ValueError):
            a.find_ccd_between(b, 0.01, np.zeros((va.shape[0] + 1, 3)))
        with pytest.raises(ValueError):
            a.find_ccd_between(b, 0.01, None, np.zeros((vb.shape[0], 2)))
        b.update_vertices(vb)                               # the tree of b is outdated
        for cd1, cd2 in ((a, b), (b, a)):
            assert lib.cd_find_collisions_between(cd1._ctx, cd2._ctx, None, 0, C.byref(n), C.byref(t)) == mi355cd.CD_ERR_ORDER
            assert lib.cd_find_proximity_between(cd1._ctx, cd2._ctx, 0.1, None, None, 0, C.byref(n), C.byref(t)) == mi355cd.CD_ERR_ORDER
            assert lib.cd_find_ccd_between(cd1._ctx, None, cd2._ctx, None, 0.1, None, None, None, 0, C.byref(n), C.byref(info)) == mi355cd.CD_ERR_ORDER
        b.build_tree()
        assert lib.cd_find_collisions_between(a._ctx, b._ctx, None, 0, C.byref(n), C.byref(t)) in (mi355cd.CD_OK, mi355cd.CD_OVERFLOW)
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:      # never built
        assert lib.cd_find_collisions_between(a._ctx, b._ctx, None, 0, C.byref(n), C.byref(t)) == mi355cd.CD_ERR_ORDER
        a.build_tree()
        assert lib.cd_find_proximity_between(a._ctx, b._ctx, 0.1, None, None, 0, C.byref(n), C.byref(t)) == mi355cd.CD_ERR_ORDER
