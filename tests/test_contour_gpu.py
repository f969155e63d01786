"""The contour of the contact queries on the device (cd_tri_isect_points, cd_find_collisions_contour, cd_find_collisions_between_contour)
against the CPU restatement (tests/isect_ref.py): every code, parameter and point bit for bit, the pair sets equal to the plain calls',
and the calls' capacity, growth, state and tree-independence rules."""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools

import numpy as np
import pytest

import isect_ref as ir
import mi355cd

pytestmark = pytest.mark.gpu


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _rows(pairs, con, tested=None) -> ir.Rows:
    """A contour call's result as Rows sorted by (face_a, face_b)."""
    n = con.faces.shape[0]
    return ir.Rows(*ir.sort_got(con.faces, pairs, con.code, con.param.reshape(n, 6), con.points.reshape(n, 6)), tested)


def _same_rows(got: ir.Rows, want: ir.Rows, what):
    assert got.faces.shape == want.faces.shape, (what, got.faces.shape, want.faces.shape)
    assert np.array_equal(got.faces, want.faces), what
    assert np.array_equal(got.pairs, want.pairs), what
    assert np.array_equal(got.code, want.code), (what, np.nonzero((got.code != want.code).any(axis=1))[0][:5])
    assert np.array_equal(_bits(got.param), _bits(want.param)), what
    assert np.array_equal(_bits(got.points), _bits(want.points)), what
    if got.tested is not None:
        assert got.tested == want.tested, (what, got.tested, want.tested)


def _pair_list(p, ordered=True):
    """A pair list as sorted rows; ordered = False: as a set of (smaller ID, larger ID) rows."""
    p = np.asarray(p, dtype=np.uint32).reshape(-1, 2)
    if not ordered:
        p = np.stack([p.min(axis=1), p.max(axis=1)], axis=1) if p.shape[0] else p
    return p[np.lexsort((p[:, 1], p[:, 0]))]


# ---------------------------------------------------------------- the pin
def _pin(tri):
    code, param, points = mi355cd.tri_isect_points(tri)
    want = ir.tri_isect_np(tri)
    assert np.array_equal(code, want.code), np.nonzero((code != want.code).any(axis=1))[0][:5]
    assert np.array_equal(_bits(param), _bits(want.param))
    assert np.array_equal(_bits(points), _bits(want.points))
    for wp, wx in ((False, False), (True, False), (False, True)):               # param / points NULL
        c, p, x = mi355cd.tri_isect_points(tri, want_param=wp, want_points=wx)
        assert np.array_equal(c, want.code)
        assert p is None or np.array_equal(_bits(p), _bits(want.param))
        assert x is None or np.array_equal(_bits(x), _bits(want.points))
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_tri_isect_pin_small(n):
    _pin(ir.pin_inputs(n))


def test_tri_isect_pin_large():
    tri = ir.pin_inputs(7 * 28672)                                              # 200 704 pairs, every set of pin_sets
    want = _pin(tri)
    assert set(np.unique(want.hit.sum(axis=1)).tolist()) == {0, 2, 3, 4, 5, 6}
    assert set(np.unique(want.code[:, :2] & 7).tolist()) == {0, 1, 2, 3, 4, 5, 7}


def test_tri_isect_pin_table():
    T = ir.table()
    tri = np.stack([np.concatenate([a, b]) for a, b, _, _ in T.values()] + [ir.grid_six_hits()])
    want = _pin(tri)
    assert want.code[:, 2].tolist() == [m for _, _, _, m in T.values()] + [63]


# ---------------------------------------------------------------- the self call
@pytest.mark.parametrize("name", list(ir.self_meshes()))
def test_self_contour(name):
    verts, vidx, ids = ir.self_meshes()[name]
    idv = np.arange(vidx.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    want = ir.cached(("self", name), lambda: ir.contour_pairs(verts, vidx, ids))
    cap = max(1, 2 * want.faces.shape[0])
    with mi355cd.CollisionDetector(verts, vidx, ids) as cd:
        cd.build_tree()
        plain, n_plain, rc = cd.find_collisions(cap=cap)
        assert rc == mi355cd.CD_OK
        sp, n_sorted = cd.sorted_pairs(cap=cap)[:2]
        pairs, n, rc, con = cd.find_collisions_contour(cap=cap)
        assert rc == mi355cd.CD_OK and n == n_plain == n_sorted == want.faces.shape[0], (name, n, n_plain, n_sorted)
        assert np.array_equal(_pair_list(pairs), _pair_list(sp, ordered=False)), name              # cd_find_collisions + cd_sorted_pairs
        assert np.array_equal(_pair_list(pairs), _pair_list(plain, ordered=False)), name
        assert np.array_equal(idv[con.faces.astype(np.int64)].reshape(-1, 2), pairs), name         # row k describes pairs[k]
        assert np.all(pairs[:, 0] < pairs[:, 1]), name                                              # no pair of equal IDs
        _same_rows(_rows(pairs, con, cd.contour_tested), want, name)
        # a NULL w: the pairs alone, from the same pass
        raw = np.zeros((cap, 2), dtype=np.uint32)
        nn, nt = C.c_uint64(0), C.c_uint64(0)
        assert cd.lib.cd_find_collisions_contour(cd._ctx, raw.ctypes.data, cap, C.byref(nn), C.byref(nt), None) == mi355cd.CD_OK
        assert nn.value == n and nt.value == want.tested and np.array_equal(_pair_list(raw[:n]), _pair_list(pairs)), name


# ---------------------------------------------------------------- between two meshes
@pytest.mark.parametrize("name", list(ir.between_cases()))
def test_between_contour(name):
    va, ia, vb, ib, ida, idb = ir.between_cases()[name]
    ab = ir.cached(("between", name), lambda: ir.contour_pairs_between(va, ia, vb, ib, ida, idb))
    ba = ir.cached(("between-swapped", name), lambda: ir.contour_pairs_between(vb, ib, va, ia, idb, ida))
    cap = max(1, 2 * ab.faces.shape[0])
    with mi355cd.CollisionDetector(va, ia, ida) as a, mi355cd.CollisionDetector(vb, ib, idb) as b:
        a.build_tree(); b.build_tree()
        got = {}
        for key, x, y, want in (("ab", a, b, ab), ("ba", b, a, ba)):
            plain, n_plain, rc = x.find_collisions_between(y, cap=cap)
            tested_plain = x.between_tested
            pairs, n, rc2, con = x.find_collisions_between_contour(y, cap=cap)
            assert rc == rc2 == mi355cd.CD_OK and n == n_plain and x.between_tested == tested_plain, (name, key)
            assert np.array_equal(_pair_list(pairs), _pair_list(plain)), (name, key)
            got[key] = _rows(pairs, con, x.between_tested)
            _same_rows(got[key], want, (name, key))
        # the swap law, row by row: b against a reports the same face pairs, hits the terms (k + 3) mod 6 and gives the same numbers;
        # only the order of the two endpoints may differ (and, where more than two terms hit, which of several farthest pairs is kept)
        g, s = got["ab"], got["ba"]
        o = np.lexsort((s.faces[:, 0], s.faces[:, 1]))
        assert np.array_equal(s.faces[o][:, ::-1], g.faces), name
        mask = g.code[:, 2].astype(np.int64)
        assert np.array_equal(s.code[o][:, 2], ((mask << 3) | (mask >> 3)) & 63), name
        few = np.array([bin(m).count("1") <= 2 for m in mask.tolist()], dtype=bool)
        assert few.any(), name
        eg, es = _endpoints(g.code, g.param, g.points, False), _endpoints(s.code[o], s.param[o], s.points[o], True)
        same = (eg == es).all(axis=(1, 2)) | (eg == es[:, ::-1]).all(axis=(1, 2))
        assert np.all(same[few]), (name, np.nonzero(few & ~same)[0][:5])
        D = lambda x: ((x[:, 0:3] - x[:, 3:6]) ** 2).sum(axis=1)
        assert np.array_equal(_bits(D(g.points)), _bits(D(s.points[o]))), name


def _endpoints(code, param, points, swapped):
    """u64[n, 2, 8]: per endpoint (term, side, t u v bits, x bits); swapped: the terms taken back through (k + 3) mod 6."""
    n = code.shape[0]
    term, side = (code[:, :2] & 7).astype(np.uint64), (code[:, :2] >> 3).astype(np.uint64)
    if swapped:
        term = np.where(term == ir.TERM_NONE, term, (term + 3) % 6)
    return np.concatenate([term[:, :, None], side[:, :, None], _bits(param).reshape(n, 2, 3), _bits(points).reshape(n, 2, 3)], axis=2)


# ---------------------------------------------------------------- independence of the tree
def test_result_does_not_depend_on_the_tree():
    name = "cloth70"
    verts, vidx, ids = ir.self_meshes()[name]
    want = ir.cached(("self", name), lambda: ir.contour_pairs(verts, vidx, ids))
    va, ia, vb, ib, ida, idb = ir.between_cases()["cloth40"]
    want_b = ir.cached(("between", "cloth40"), lambda: ir.contour_pairs_between(va, ia, vb, ib, ida, idb))
    cap = 2 * want.faces.shape[0]
    with mi355cd.CollisionDetector(verts, vidx) as cd, mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:
        b.build_tree()
        for setup in ("auto", "reference", "trav0", "trav1", "trav3", "stagewise"):
            for x in (cd, a):
                if setup == "auto":
                    x.set_morton_frame(mi355cd.CD_FRAME_AUTO)
                elif setup == "reference":
                    x.set_morton_frame(mi355cd.CD_FRAME_REFERENCE)
                elif setup == "stagewise":
                    x.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 1)
                else:
                    x.set_option(mi355cd.CD_OPT_TRAVERSAL, int(setup[-1]))
                x.self_collide(cap=1 << 20)                                     # the tree, through the fused build the setup selects
            pairs, n, rc, con = cd.find_collisions_contour(cap=cap)
            assert rc == mi355cd.CD_OK, setup
            _same_rows(_rows(pairs, con, cd.contour_tested), want, setup)
            pairs, n, rc, con = a.find_collisions_between_contour(b, cap=cap)
            assert rc == mi355cd.CD_OK, setup
            _same_rows(_rows(pairs, con, a.between_tested), want_b, setup)


# ---------------------------------------------------------------- capacity, growth, NULL outputs
CANARY = 0xA5


class _Raw:
    """The arrays of one raw call, `rows` rows each, filled with a canary."""

    def __init__(self, rows):
        mk = lambda shape, dt: np.frombuffer(bytes([CANARY]) * (int(np.prod(shape)) * np.dtype(dt).itemsize), dtype=dt).reshape(shape).copy()
        self.pairs, self.faces, self.code = mk((rows, 2), np.uint32), mk((rows, 2), np.uint32), mk((rows, 3), np.uint8)
        self.param, self.points = mk((rows, 6), np.float64), mk((rows, 6), np.float64)
        self.members = {"faces": self.faces, "code": self.code, "param": self.param, "points": self.points}

    def record(self, names=("faces", "code", "param", "points")):
        return mi355cd.CdContourOut(**{k: self.members[k].ctypes.data for k in names})

    def untouched_from(self, k, names=("pairs", "faces", "code", "param", "points")):
        return all(np.all(getattr(self, x)[k:].view(np.uint8) == CANARY) for x in names)

    def rows(self, n):
        con = mi355cd.Contour(self.faces[:n], self.code[:n], self.param[:n].reshape(-1, 2, 3), self.points[:n].reshape(-1, 2, 3))
        return _rows(self.pairs[:n], con)


def _raw_call(cd, r, cap, other=None, w="all"):
    """cd_find_collisions_contour (other None) or cd_find_collisions_between_contour into r's arrays: (rc, n)."""
    n = C.c_uint64(0)
    rec = None if w is None else (r.record() if w == "all" else w)
    wp = None if rec is None else C.byref(rec)
    if other is None:
        rc = cd.lib.cd_find_collisions_contour(cd._ctx, r.pairs.ctypes.data, cap, C.byref(n), None, wp)
    else:
        rc = cd.lib.cd_find_collisions_between_contour(cd._ctx, other._ctx, r.pairs.ctypes.data, cap, C.byref(n), None, wp)
    return rc, n.value


@pytest.mark.parametrize("between", [False, True], ids=["self", "between"])
def test_capacity_growth_and_null_outputs(between):
    if between:
        va, ia, vb, ib, ida, idb = ir.between_cases()["cloth40"]
        want = ir.cached(("between", "cloth40"), lambda: ir.contour_pairs_between(va, ia, vb, ib, ida, idb))
        sa, sia, sb, sib = ir.between_cases()["soups"][:4]
        small_want = ir.cached(("between", "soups"), lambda: ir.contour_pairs_between(sa, sia, sb, sib))
        small_ctx = (mi355cd.CollisionDetector(sa, sia), mi355cd.CollisionDetector(sb, sib))
        ctx = (mi355cd.CollisionDetector(va, ia), mi355cd.CollisionDetector(vb, ib))
    else:
        verts, vidx, ids = ir.self_meshes()["cloth70"]
        want = ir.cached(("self", "cloth70"), lambda: ir.contour_pairs(verts, vidx, ids))
        ctx = (mi355cd.CollisionDetector(verts, vidx), None)
    total = want.faces.shape[0]
    assert total >= 64
    with contextlib.ExitStack() as stack:
        cd, other = (x if x is None else stack.enter_context(x) for x in ctx)
        cd.build_tree()
        if other is not None:
            other.build_tree()
        # cap 0 first, then a small cap: the device buffers are sized for them, then grow
        r = _Raw(total + 8)
        rc, n = _raw_call(cd, r, 0, other)
        assert rc == mi355cd.CD_OVERFLOW and n == total and r.untouched_from(0)
        cap = total // 3                                                        # CD_OVERFLOW, the true count, nothing at or past cap in any array
        rc, n = _raw_call(cd, r, cap, other)
        assert rc == mi355cd.CD_OVERFLOW and n == total
        assert r.untouched_from(cap)
        assert not np.any(np.all(r.faces[:cap].view(np.uint8) == CANARY, axis=1))          # ... and every row below it written
        index = {tuple(f): k for k, f in enumerate(want.faces.tolist())}
        at = np.array([index[tuple(f)] for f in r.faces[:cap].tolist()])                   # (a KeyError: a row that is not of the result)
        assert np.unique(at).shape[0] == cap
        assert np.array_equal(r.code[:cap], want.code[at]) and np.array_equal(_bits(r.param[:cap]), _bits(want.param[at]))
        assert np.array_equal(_bits(r.points[:cap]), _bits(want.points[at])) and np.array_equal(r.pairs[:cap], want.pairs[at])
        r = _Raw(total + 8)                                                     # enough room: the whole result (the buffers grew)
        rc, n = _raw_call(cd, r, total, other)
        assert rc == mi355cd.CD_OK and n == total and r.untouched_from(total)
        _same_rows(r.rows(n), want._replace(tested=None), "full")
        r = _Raw(2 * total + 8)                                                 # ... and again, larger
        rc, n = _raw_call(cd, r, 2 * total, other)
        assert rc == mi355cd.CD_OK and n == total and r.untouched_from(total)
        _same_rows(r.rows(n), want._replace(tested=None), "larger")
        # NULL w, and a w whose members are all NULL: the pairs alone
        for w in (None, mi355cd.CdContourOut()):
            q = _Raw(total + 8)
            rc, n = _raw_call(cd, q, total, other, w=w)
            assert rc == mi355cd.CD_OK and n == total and q.untouched_from(total, ("pairs",))
            assert np.array_equal(_pair_list(q.pairs[:n]), _pair_list(want.pairs))
            assert q.untouched_from(0, ("faces", "code", "param", "points"))
        # every subset of the members
        names = ("faces", "code", "param", "points")
        for k in range(1, 4):
            for sub in itertools.combinations(names, k):
                q = _Raw(total + 8)
                rc, n = _raw_call(cd, q, total, other, w=q.record(sub))
                assert rc == mi355cd.CD_OK and n == total, sub
                assert q.untouched_from(0, tuple(x for x in names if x not in sub)) and q.untouched_from(total, sub + ("pairs",)), sub
                if "faces" in sub:
                    o = np.lexsort((q.faces[:n, 1], q.faces[:n, 0]))
                    assert np.array_equal(q.faces[:n][o], want.faces), sub
                    for x in sub[1:]:
                        assert np.array_equal(q.members[x][:n][o].view(np.uint8), getattr(want, x).view(np.uint8)), (sub, x)
                else:                                                           # no faces to join on: the rows as multisets
                    for x in sub:
                        assert sorted(r.tobytes() for r in q.members[x][:n]) == sorted(r.tobytes() for r in getattr(want, x)), (sub, x)
        if between:                                                             # another pair of contexts, with exactly the room the result needs
            sa_, sb_ = small_ctx
            with sa_, sb_:
                sa_.build_tree(); sb_.build_tree()
                k = small_want.faces.shape[0]
                q = _Raw(k + 4)
                rc, n = _raw_call(sa_, q, k, sb_)
                assert rc == mi355cd.CD_OK and n == k and q.untouched_from(k)
                _same_rows(q.rows(n), small_want._replace(tested=None), "small")


# ---------------------------------------------------------------- state the calls leave alone
def test_contour_calls_leave_the_context_as_it_was():
    import between_ref as br
    verts, vidx, ids = ir.self_meshes()["soup10k"]
    d = 0.05 / 4
    other_v, other_i = br.soup(65, 0.3, 32)
    with mi355cd.CollisionDetector(verts, vidx) as cd, mi355cd.CollisionDetector(other_v, other_i) as ob:
        ob.build_tree()
        pairs, n, rc = cd.self_collide(cap=1 << 16)
        assert rc == mi355cd.CD_OK and n > 0
        st0, sp0 = cd.stats(), cd.sorted_pairs(cap=1 << 16)
        prox0 = cd.find_proximity(d)
        bw0 = cd.find_proximity_between(ob, d)
        cpairs, cn, crc, _ = cd.find_collisions_contour()
        assert crc == mi355cd.CD_OK and cn == n
        cd.find_collisions_between_contour(ob)
        st1, sp1 = cd.stats(), cd.sorted_pairs(cap=1 << 16)
        for f, _ in mi355cd.CdStats._fields_:
            assert getattr(st0, f) == getattr(st1, f), f
        assert np.array_equal(sp0[0], sp1[0]) and sp0[1] == sp1[1]
        assert np.array_equal(_pair_list(cpairs), _pair_list(sp0[0], ordered=False))
        for got, was in ((cd.find_proximity(d), prox0), (cd.find_proximity_between(ob, d), bw0)):
            assert got[2] == was[2] and got[3] == was[3] == mi355cd.CD_OK
            o, p = np.lexsort((got[0][:, 1], got[0][:, 0])), np.lexsort((was[0][:, 1], was[0][:, 0]))
            assert np.array_equal(got[0][o], was[0][p]) and np.array_equal(_bits(got[1][o]), _bits(was[1][p]))


# ---------------------------------------------------------------- a mesh that moves
def test_moving_mesh():
    import moving_inputs as mv
    s = mv.seq("jitter")                                                        # frame 2 is the dense one: a shard of the first candidate buffer overflows
    rows = []
    with mi355cd.CollisionDetector(s.frames[0], s.vidx) as cd:
        for f in range(4):
            if f:
                cd.update_vertices(s.frames[f])
            cd.build_tree()
            want = ir.cached(("jitter", f), lambda: ir.contour_pairs(s.frames[f], s.vidx))
            cap = max(1, 2 * want.faces.shape[0])
            pairs, n, rc, con = cd.find_collisions_contour(cap=cap)
            assert rc == mi355cd.CD_OK, f
            _same_rows(_rows(pairs, con, cd.contour_tested), want, f)
            plain, n_plain, rc = cd.find_collisions(cap=cap)
            assert rc == mi355cd.CD_OK and np.array_equal(_pair_list(plain, ordered=False), _pair_list(pairs)), f
            rows.append(want.faces.shape[0])
    assert min(rows) > 0 and rows[2] > 4 * rows[1], rows
