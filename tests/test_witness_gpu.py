"""The witness of the pair queries on the device (cd_tri_witness_points, cd_find_proximity_witness, cd_find_proximity_between_witness,
cd_find_ccd_witness, cd_find_ccd_between_witness) against the CPU restatement (tests/witness_ref.py): every point, barycentric and
feature bit for bit, the plain calls' results unchanged, and the calls' capacity, growth, state and error rules."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import between_ref as br
import mi355cd
import witness_ref as wr

pytestmark = pytest.mark.gpu


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _rows(pairs, toi, dists, wit) -> wr.Rows:
    """A witness call's result as Rows sorted by (face_a, face_b)."""
    return wr.Rows(*wr.sort_rows(wit.faces, pairs, toi, dists, wit.points, wit.bary, wit.feature))


def _same_rows(got: wr.Rows, want: wr.Rows, what):
    assert got.faces.shape == want.faces.shape, (what, got.faces.shape, want.faces.shape)
    assert np.array_equal(got.faces, want.faces), what
    assert np.array_equal(got.pairs, want.pairs), what
    if want.toi is not None:
        assert np.array_equal(_bits(got.toi), _bits(want.toi)), what
    assert np.array_equal(_bits(got.dists), _bits(want.dists)), what
    assert np.array_equal(got.feature, want.feature), (what, np.nonzero((got.feature != want.feature).any(axis=1))[0][:5])
    assert np.array_equal(_bits(got.bary), _bits(want.bary)), what
    assert np.array_equal(_bits(got.points), _bits(want.points)), what


def _same_as_plain(got, plain, what):
    """(pairs, [toi,] dists, n, rc) of a witness call and of the plain call, as sorted lists."""
    k = len(plain) - 2
    assert got[k] == plain[k] and got[k + 1] == plain[k + 1] == mi355cd.CD_OK, what
    for g, p in zip(wr.sort_by_ids(*got[:k]), wr.sort_by_ids(*plain[:k])):
        assert np.array_equal(g, p), what


# ---------------------------------------------------------------- the pin
def _pin(tri):
    dist, points, bary, feature = mi355cd.tri_witness_points(tri)
    want = wr.tri_witness_np(tri)
    assert np.array_equal(_bits(dist), _bits(want.dist))
    assert np.array_equal(feature, want.feature), np.nonzero((feature != want.feature).any(axis=1))[0][:5]
    assert np.array_equal(_bits(bary), _bits(want.bary))
    assert np.array_equal(_bits(points), _bits(want.points))
    assert np.array_equal(_bits(dist), _bits(mi355cd.tri_distance_points(tri)))
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_tri_witness_pin_small(n):
    _pin(wr.pin_inputs(n))


def test_tri_witness_pin_large():
    tri = wr.pin_inputs(7 * 28672)                                              # 200 704 pairs, every set of pin_sets
    want = _pin(tri)
    assert set(np.unique(want.win).tolist()) == set(range(-1, 33))              # every term wins somewhere, and some pairs have no witness
    lib = mi355cd.load_library()                                                # every output except dist may be NULL
    t = np.ascontiguousarray(tri[:300].reshape(-1, 18))
    d = np.zeros(300)
    assert lib.cd_tri_witness_points(t.ctypes.data, 300, d.ctypes.data, None, None, None) == mi355cd.CD_OK
    assert np.array_equal(_bits(d), _bits(want.dist[:300]))
    assert lib.cd_tri_witness_points(t.ctypes.data, 300, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_tri_witness_points(None, 0, None, None, None, None) == mi355cd.CD_ERR_ARG


# ---------------------------------------------------------------- self proximity
@pytest.mark.parametrize("name", list(wr.self_meshes()))
def test_self_proximity_witness(name):
    verts, vidx, ids, edge = wr.self_meshes()[name]
    idv = np.arange(vidx.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    with mi355cd.CollisionDetector(verts, vidx, ids) as cd:
        cd.build_tree()
        for d in wr.self_dists(edge):
            want = wr.cached(("prox", name, d), lambda: wr.witness_pairs(verts, vidx, ids, d))
            cap = max(1, 2 * want.faces.shape[0])
            plain = cd.find_proximity(d, cap=cap)
            got = cd.find_proximity_witness(d, cap=cap)
            _same_as_plain(got[:4], plain, (name, d))
            assert np.array_equal(idv[got[4].faces.astype(np.int64)], got[0]), (name, d)      # row k describes pairs[k]
            _same_rows(_rows(got[0], None, got[1], got[4]), want, (name, d))


# ---------------------------------------------------------------- between two meshes
@pytest.mark.parametrize("name", list(wr.between_cases()))
def test_between_proximity_witness(name):
    va, ia, vb, ib, d = wr.between_cases()[name]
    ab = wr.cached(("bprox", name), lambda: wr.witness_pairs_between(va, ia, vb, ib, d))
    ba = wr.cached(("bprox-swapped", name), lambda: wr.witness_pairs_between(vb, ib, va, ia, d))
    cap = 2 * ab.faces.shape[0]
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:
        a.build_tree(); b.build_tree()
        got = {}
        for key, x, y, want in (("ab", a, b, ab), ("ba", b, a, ba)):
            plain = x.find_proximity_between(y, d, cap=cap)
            g = x.find_proximity_between_witness(y, d, cap=cap)
            _same_as_plain(g[:4], plain, (name, key))
            got[key] = _rows(g[0], None, g[1], g[4])
            _same_rows(got[key], want, (name, key))
        # each call reports the other's rows, A and B exchanged
        assert np.array_equal(wr.sort_rows(got["ba"].faces[:, ::-1])[0], got["ab"].faces)


# ---------------------------------------------------------------- continuous collision
def _prox_rows_at(rows, sel, va, ia, vb, ib):
    """tri_witness of the selected rows' triangles at the given positions (the proximity witness there)."""
    fa, fb = rows.faces[sel, 0].astype(np.int64), rows.faces[sel, 1].astype(np.int64)
    return wr.tri_witness_np(np.concatenate([va[np.asarray(ia, dtype=np.int64)[fa]], vb[np.asarray(ib, dtype=np.int64)[fb]]], axis=1))


def _ends_are_proximity(got, va0, va1, ia, vb0, vb1, ib, what):
    for t, xa, xb in ((0.0, va0, vb0), (1.0, va1, vb1)):
        sel = got.toi == t
        assert sel.any(), (what, t)
        w = _prox_rows_at(got, sel, xa, ia, xb, ib)
        assert np.array_equal(_bits(got.dists[sel]), _bits(w.dist)), (what, t)
        assert np.array_equal(got.feature[sel], w.feature) and np.array_equal(_bits(got.bary[sel]), _bits(w.bary)), (what, t)
        assert np.array_equal(_bits(got.points[sel]), _bits(w.points)), (what, t)


@pytest.mark.parametrize("name", ["soup10k", "cloth100"])
def test_self_ccd_witness(name):
    verts, vidx, ids, edge = wr.self_meshes()[name]
    x1, d = wr.ccd_case(name)
    want = wr.cached(("ccd", name, d), lambda: wr.witness_pairs(verts, vidx, ids, d, verts_end=x1))
    cap = 2 * want.faces.shape[0]
    with mi355cd.CollisionDetector(verts, vidx, ids) as cd:
        cd.build_tree()
        plain = cd.find_ccd(x1, d, cap=cap)
        got = cd.find_ccd_witness(x1, d, cap=cap)
        _same_as_plain(got[:5], plain, name)
        rows = _rows(got[0], got[1], got[2], got[5])
        _same_rows(rows, want, name)
        _ends_are_proximity(rows, verts, x1, vidx, verts, x1, vidx, name)


@pytest.mark.parametrize("name", list(wr.between_cases()))
def test_between_ccd_witness(name):
    va, ia, vb, ib, d = wr.between_cases()[name]
    va1 = br.motion(va, 0.3 * d, 12)                                            # b is a static obstacle: verts_end = None
    want = wr.cached(("bccd", name), lambda: wr.witness_pairs_between(va, ia, vb, ib, d, ccd=True, va1=va1))
    cap = 2 * want.faces.shape[0]
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:
        a.build_tree(); b.build_tree()
        plain = a.find_ccd_between(b, d, verts_end=va1, cap=cap)
        got = a.find_ccd_between_witness(b, d, verts_end=va1, cap=cap)
        _same_as_plain(got[:5], plain, name)
        rows = _rows(got[0], got[1], got[2], got[5])
        _same_rows(rows, want, name)
        _ends_are_proximity(rows, va, va1, ia, vb, vb, ib, name)


# ---------------------------------------------------------------- independence of the tree
def test_result_does_not_depend_on_the_tree():
    name = "cloth100"
    verts, vidx, ids, edge = wr.self_meshes()[name]
    d = wr.self_dists(edge)[1]
    x1, dc = wr.ccd_case(name)
    want = wr.cached(("prox", name, d), lambda: wr.witness_pairs(verts, vidx, ids, d))
    want_ccd = wr.cached(("ccd", name, dc), lambda: wr.witness_pairs(verts, vidx, ids, dc, verts_end=x1))
    cap = 2 * max(want.faces.shape[0], want_ccd.faces.shape[0])
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        for setup in ("auto", "reference", "trav0", "trav1", "trav3", "stagewise"):
            if setup == "auto":
                cd.set_morton_frame(mi355cd.CD_FRAME_AUTO)
            elif setup == "reference":
                cd.set_morton_frame(mi355cd.CD_FRAME_REFERENCE)
            elif setup == "stagewise":
                cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 1)
            else:
                cd.set_option(mi355cd.CD_OPT_TRAVERSAL, int(setup[-1]))
            cd.self_collide(cap=1 << 20)                                        # the tree, through the fused build the setup selects
            g = cd.find_proximity_witness(d, cap=cap)
            assert g[3] == mi355cd.CD_OK, setup
            _same_rows(_rows(g[0], None, g[1], g[4]), want, setup)
            g = cd.find_ccd_witness(x1, dc, cap=cap)
            assert g[4] == mi355cd.CD_OK, setup
            _same_rows(_rows(g[0], g[1], g[2], g[5]), want_ccd, setup)


# ---------------------------------------------------------------- capacity, growth, NULL outputs
CANARY = 0xA5


class _Raw:
    """The arrays of one raw call, `rows` rows each, filled with a canary."""

    def __init__(self, rows, ccd):
        mk = lambda shape, dt: np.frombuffer(bytes([CANARY]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dtype=dt).reshape(shape).copy()
        self.pairs, self.dists = mk((rows, 2), np.uint32), mk((rows,), np.float64)
        self.toi = mk((rows,), np.float64) if ccd else None
        self.faces, self.points, self.bary, self.feature = mk((rows, 2), np.uint32), mk((rows, 6), np.float64), mk((rows, 4), np.float64), mk((rows, 2), np.uint8)
        self.out = mi355cd.CdWitnessOut(self.faces.ctypes.data, self.points.ctypes.data, self.bary.ctypes.data, self.feature.ctypes.data)

    def arrays(self):
        return [x for x in (self.pairs, self.dists, self.toi, self.faces, self.points, self.bary, self.feature) if x is not None]

    def untouched_from(self, k):
        return all(np.all(x[k:].view(np.uint8) == CANARY) for x in self.arrays())


def _raw_call(cd, r, dist, cap, x1=None, w="own"):
    """cd_find_proximity_witness (x1 None) or cd_find_ccd_witness into r's arrays: (rc, n).  w: 'own' r's record, None, or a record."""
    lib, n = cd.lib, C.c_uint64(0)
    wp = C.byref(r.out) if w == "own" else (None if w is None else C.byref(w))
    if x1 is None:
        rc = lib.cd_find_proximity_witness(cd._ctx, float(dist), r.pairs.ctypes.data, r.dists.ctypes.data, cap, C.byref(n), None, wp)
    else:
        x1 = np.ascontiguousarray(x1, dtype=np.float64)
        rc = lib.cd_find_ccd_witness(cd._ctx, x1.ctypes.data, float(dist), r.pairs.ctypes.data, r.toi.ctypes.data, r.dists.ctypes.data, cap, C.byref(n), None, wp)
    return rc, n.value


@pytest.mark.parametrize("ccd", [False, True], ids=["proximity", "ccd"])
def test_capacity_growth_and_null_outputs(ccd):
    name = "soup10k"
    verts, vidx, ids, edge = wr.self_meshes()[name]
    x1, dc = wr.ccd_case(name)
    d = dc if ccd else wr.self_dists(edge)[1]
    x1 = x1 if ccd else None
    want = wr.cached(("ccd", name, d), lambda: wr.witness_pairs(verts, vidx, ids, d, verts_end=x1)) if ccd else \
        wr.cached(("prox", name, d), lambda: wr.witness_pairs(verts, vidx, ids, d))
    total = want.faces.shape[0]
    assert total >= 64
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        # a small dist first (CCD: and no motion), with exactly the room it needs: the device buffers are sized for it, then grow
        small = _Raw(total, ccd)
        xs = verts if ccd else None
        rc, n0 = _raw_call(cd, small, d / 8, 0, xs)
        assert rc == mi355cd.CD_OVERFLOW and 0 < 4 * n0 <= total and small.untouched_from(0), (n0, total)
        rc, n = _raw_call(cd, small, d / 8, n0, xs)
        assert rc == mi355cd.CD_OK and n == n0 and small.untouched_from(n0)
        # a cap below the count: CD_OVERFLOW, the true count, nothing at or past cap in any array
        cap = total // 3
        r = _Raw(total + 8, ccd)
        rc, n = _raw_call(cd, r, d, cap, x1)
        assert rc == mi355cd.CD_OVERFLOW and n == total
        assert r.untouched_from(cap)
        assert not np.any(np.all(r.faces[:cap].view(np.uint8) == CANARY, axis=1))          # ... and every row below it written
        full = {tuple(f) for f in want.faces.tolist()}
        assert all(tuple(f) in full for f in r.faces[:cap].tolist())
        # enough room: the whole result (the buffers grew from the small call's)
        r = _Raw(total + 8, ccd)
        rc, n = _raw_call(cd, r, d, total, x1)
        assert rc == mi355cd.CD_OK and n == total and r.untouched_from(total)
        wit = mi355cd.Witness(r.faces[:n], r.points[:n].reshape(-1, 2, 3), r.bary[:n].reshape(-1, 2, 2), r.feature[:n])
        _same_rows(_rows(r.pairs[:n], r.toi[:n] if ccd else None, r.dists[:n], wit), want, "full")
        # NULL w, and a w whose members are all NULL: the plain call
        plain = cd.find_ccd(x1, d, cap=total)[:3] if ccd else cd.find_proximity(d, cap=total)[:2]
        for w in (None, mi355cd.CdWitnessOut()):
            q = _Raw(total + 8, ccd)
            rc, n = _raw_call(cd, q, d, total, x1, w=w)
            assert rc == mi355cd.CD_OK and n == total
            vals = (q.toi[:n], q.dists[:n]) if ccd else (q.dists[:n],)
            for g, p in zip(wr.sort_by_ids(q.pairs[:n], *vals), wr.sort_by_ids(*plain)):
                assert np.array_equal(g, p)
            assert all(np.all(x.view(np.uint8) == CANARY) for x in (q.faces, q.points, q.bary, q.feature))
        # single members
        q = _Raw(total, ccd)
        only = mi355cd.CdWitnessOut(q.faces.ctypes.data, None, None, None)
        rc, n = _raw_call(cd, q, d, total, x1, w=only)
        assert rc == mi355cd.CD_OK and np.array_equal(wr.sort_rows(q.faces)[0], want.faces)
        assert all(np.all(x.view(np.uint8) == CANARY) for x in (q.points, q.bary, q.feature))


@pytest.mark.parametrize("ccd", [False, True], ids=["proximity", "ccd"])
def test_between_null_witness_is_the_plain_call(ccd):
    """cd_find_proximity_between_witness / cd_find_ccd_between_witness with a NULL w, and with a w whose members are all NULL, against
    the plain between call; then with every member set, in the same context."""
    verts, vidx, ids, edge = wr.self_meshes()["n65"]
    x1 = np.ascontiguousarray(br.motion(verts, 0.1 * edge, 3)) if ccd else None
    bv, bi = br.soup(63, 0.3, 31)
    d = 0.15                                        # between_ref on these meshes: 17 proximity pairs, 19 CCD pairs
    with mi355cd.CollisionDetector(verts, vidx) as cd, mi355cd.CollisionDetector(bv, bi) as ob:
        cd.build_tree()
        ob.build_tree()
        *plain, n0, rc0 = cd.find_ccd_between(ob, d, verts_end=x1) if ccd else cd.find_proximity_between(ob, d)
        assert rc0 == mi355cd.CD_OK and n0 >= 8
        plain = wr.sort_by_ids(*plain)
        for w in (None, mi355cd.CdWitnessOut(), "own"):
            q, n = _Raw(n0 + 8, ccd), C.c_uint64(0)
            wp = None if w is None else C.byref(q.out if w == "own" else w)
            if ccd:
                rc = cd.lib.cd_find_ccd_between_witness(cd._ctx, x1.ctypes.data, ob._ctx, None, d, q.pairs.ctypes.data, q.toi.ctypes.data,
                                                        q.dists.ctypes.data, n0, C.byref(n), None, wp)
            else:
                rc = cd.lib.cd_find_proximity_between_witness(cd._ctx, ob._ctx, d, q.pairs.ctypes.data, q.dists.ctypes.data, n0, C.byref(n), None, wp)
            assert (rc, n.value) == (rc0, n0), w
            vals = (q.toi[:n0], q.dists[:n0]) if ccd else (q.dists[:n0],)
            for g, p in zip(wr.sort_by_ids(q.pairs[:n0], *vals), plain):
                assert np.array_equal(g, p), w
            assert q.untouched_from(n0)
            if w == "own":
                assert not np.any(np.all(q.faces[:n0].view(np.uint8) == CANARY, axis=1))      # every row written
            else:
                assert all(np.all(x.view(np.uint8) == CANARY) for x in (q.faces, q.points, q.bary, q.feature))


# ---------------------------------------------------------------- state the calls leave alone
def test_witness_calls_leave_the_context_as_it_was():
    name = "soup10k"
    verts, vidx, ids, edge = wr.self_meshes()[name]
    x1, dc = wr.ccd_case(name)
    d = wr.self_dists(edge)[1]
    other_v, other_i = br.soup(65, 0.3, 32)
    with mi355cd.CollisionDetector(verts, vidx) as cd, mi355cd.CollisionDetector(other_v, other_i) as ob:
        ob.build_tree()
        pairs, n, rc = cd.self_collide(cap=1 << 16)
        assert rc == mi355cd.CD_OK and n > 0
        st0, sp0 = cd.stats(), cd.sorted_pairs(cap=1 << 16)
        prox0, ccd0 = cd.find_proximity(d), cd.find_ccd(x1, dc)
        cd.find_proximity_witness(d)
        cd.find_ccd_witness(x1, dc)
        cd.find_proximity_between_witness(ob, d)
        cd.find_ccd_between_witness(ob, dc, verts_end=x1)
        st1, sp1 = cd.stats(), cd.sorted_pairs(cap=1 << 16)
        for f, _ in mi355cd.CdStats._fields_:
            assert getattr(st0, f) == getattr(st1, f), f
        assert np.array_equal(sp0[0], sp1[0]) and sp0[1] == sp1[1]
        _same_as_plain(cd.find_proximity(d), prox0, "proximity after")
        _same_as_plain(cd.find_ccd(x1, dc), ccd0, "ccd after")


# ---------------------------------------------------------------- errors
def test_order_and_argument_errors():
    verts, vidx, ids, edge = wr.self_meshes()["n65"]
    x1 = br.motion(verts, 0.1 * edge, 3)
    bv, bi = br.soup(63, 0.3, 31)
    with mi355cd.CollisionDetector(verts, vidx) as cd, mi355cd.CollisionDetector(bv, bi) as ob:
        calls = {
            "proximity": lambda dist=0.1: cd.find_proximity_witness(dist),
            "ccd": lambda dist=0.1: cd.find_ccd_witness(x1, dist),
            "between": lambda dist=0.1: cd.find_proximity_between_witness(ob, dist),
            "between ccd": lambda dist=0.1: cd.find_ccd_between_witness(ob, dist, verts_end=x1),
        }

        def rc_of(fn, *a):
            with pytest.raises(mi355cd.CdError) as e:
                fn(*a)
            return e.value.rc

        ob.build_tree()
        for what, fn in calls.items():                                          # before a tree
            assert rc_of(fn) == mi355cd.CD_ERR_ORDER, what
        cd.build_tree()
        for what, fn in calls.items():
            assert fn()[-2] == mi355cd.CD_OK, what
        cd.update_vertices(verts)                                               # vertices newer than the tree
        for what, fn in calls.items():
            assert rc_of(fn) == mi355cd.CD_ERR_ORDER, what
        cd.build_tree()
        ob.update_vertices(bv)                                                  # ... or the other mesh's
        for what in ("between", "between ccd"):
            assert rc_of(calls[what]) == mi355cd.CD_ERR_ORDER, what
        ob.build_tree()
        for what, fn in calls.items():                                          # dist as the plain calls: NaN, negative, infinite; CCD also 0
            for bad in (float("nan"), -1.0, float("inf")) + ((0.0,) if "ccd" in what else ()):
                assert rc_of(fn, bad) == mi355cd.CD_ERR_ARG, (what, bad)
        assert rc_of(lambda: cd.find_proximity_between_witness(cd, 0.1)) == mi355cd.CD_ERR_ARG        # a == b
        assert rc_of(lambda: cd.find_ccd_between_witness(cd, 0.1)) == mi355cd.CD_ERR_ARG
        r = _Raw(4, False)                                                      # cap_pairs > 0 without pairs
        n = C.c_uint64(0)
        assert cd.lib.cd_find_proximity_witness(cd._ctx, 0.1, None, None, 4, C.byref(n), None, C.byref(r.out)) == mi355cd.CD_ERR_ARG
        assert cd.lib.cd_find_ccd_witness(cd._ctx, None, 0.1, r.pairs.ctypes.data, None, None, 4, C.byref(n), None, C.byref(r.out)) == mi355cd.CD_ERR_ARG
        assert r.untouched_from(0)
