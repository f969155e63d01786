"""The swept-tree restatement (tests/swept_ref.py) against exact arithmetic and a naive recursion, without a GPU: the directed
roundings against Fraction, the range-min records against a bottom-up union over the oracle's tree, the grid's candidate count against
all pairs, and the comparison functions of tests/test_swept_gpu.py against planted errors (a correct record array with one half
rounded the wrong way, one half left at a child's box, a pad without its M term, one candidate fewer)."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import between_ref as br
import mi355_synth as synth
import oracle
import swept_ref as sr
from query_meshes import _comb

FLT_MAX = float(np.finfo(np.float32).max)
TINY = 2.0 ** -149


def _frac(f):
    return Fraction(float(f))


def _round_frac(v: Fraction, down: bool) -> float:
    """The fp32 neighbour of the rational v on the asked side (+-inf beyond +-FLT_MAX), by exact comparisons."""
    if v > Fraction(FLT_MAX):
        return FLT_MAX if down else float("inf")
    if v < -Fraction(FLT_MAX):
        return float("-inf") if down else -FLT_MAX
    f = np.float32(float(v)) if abs(v) < Fraction(2) ** 200 else np.float32(FLT_MAX if v > 0 else -FLT_MAX)
    if not np.isfinite(f):
        f = np.float32(FLT_MAX if v > 0 else -FLT_MAX)
    if down:
        while _frac(f) > v:
            f = np.nextafter(f, np.float32(-np.inf))
        while np.isfinite(np.nextafter(f, np.float32(np.inf))) and _frac(np.nextafter(f, np.float32(np.inf))) <= v:
            f = np.nextafter(f, np.float32(np.inf))
    else:
        while _frac(f) < v:
            f = np.nextafter(f, np.float32(np.inf))
        while np.isfinite(np.nextafter(f, np.float32(-np.inf))) and _frac(np.nextafter(f, np.float32(-np.inf))) >= v:
            f = np.nextafter(f, np.float32(-np.inf))
    return float(f)


def _doubles(seed=1):
    g = np.random.default_rng(seed)
    x = [g.normal(size=1000) * 2.0 ** g.integers(-170, 135, 1000)]
    f = (g.normal(size=400) * 2.0 ** g.integers(-150, 127, 400)).astype(np.float32).astype(np.float64)
    f = f[np.isfinite(f)]
    nxt = np.nextafter(f.astype(np.float32), np.float32(np.inf)).astype(np.float64)
    nxt = np.where(np.isfinite(nxt), nxt, f)
    x += [f, (f + nxt) / 2, np.nextafter(f, np.inf), np.nextafter(f, -np.inf), np.nextafter((f + nxt) / 2, np.inf)]   # floats, ties, one ulp64 off
    d = np.arange(0, 40) * TINY
    x += [d, -d, d + TINY / 2, -(d + TINY / 2), d + TINY / 4, np.array([1e-60, -1e-60, 5e-324, -5e-324, 2.0 ** -126, -(2.0 ** -126)])]
    edge = np.array([FLT_MAX, -FLT_MAX, np.nextafter(FLT_MAX, np.inf), np.nextafter(FLT_MAX, 0.0), np.nextafter(-FLT_MAX, -np.inf),
                     2.0 ** 128, -(2.0 ** 128), FLT_MAX + 2.0 ** 102, FLT_MAX + 2.0 ** 103, 1e39, -1e39, 1e300, -1e300, 0.0, -0.0])
    x += [edge]
    return np.concatenate(x)


def test_rd32_ru32_against_exact_arithmetic():
    x = _doubles()
    assert x.size > 3000
    lo, hi = sr.rd32(x), sr.ru32(x)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    for v, a, b in zip(x.tolist(), lo.tolist(), hi.tolist()):
        assert a == _round_frac(Fraction(v), True), (v, a)
        assert b == _round_frac(Fraction(v), False), (v, b)
    assert np.all(lo.astype(np.float64) <= x) and np.all(hi.astype(np.float64) >= x)
    # the cases named in the module's contract, and the zeros' signs
    assert sr.ru32(1e39) == np.inf and sr.rd32(1e39) == np.float32(FLT_MAX) and sr.rd32(-1e39) == -np.inf and sr.ru32(-1e39) == np.float32(-FLT_MAX)
    assert sr.rd32(np.inf) == np.inf and sr.ru32(-np.inf) == -np.inf and sr.rd32(-np.inf) == -np.inf and sr.ru32(np.inf) == np.inf
    assert sr.bits1(sr.ru32(-1e-60)) == 0x80000000 and sr.bits1(sr.rd32(1e-60)) == 0
    assert sr.bits1(sr.rd32(-1e-60)) == 0x80000001 and sr.bits1(sr.ru32(1e-60)) == 1
    assert sr.bits1(sr.rd32(-0.0)) == 0x80000000 and sr.bits1(sr.ru32(0.0)) == 0


def _float_pairs(seed=2):
    g = np.random.default_rng(seed)
    n = 1500
    a = (g.normal(size=n) * 2.0 ** g.integers(-149, 127, n)).astype(np.float32)
    b = (g.normal(size=n) * 2.0 ** g.integers(-149, 127, n)).astype(np.float32)             # far apart: the exact sum is no double
    c = (g.normal(size=n) * 2.0 ** g.integers(-20, 20, n)).astype(np.float32)
    near = (c * np.float32(1 + 2.0 ** -12) * g.choice([-1.0, 1.0], n)).astype(np.float32)    # near-cancelling, within a few binades
    tiny = np.full(n, TINY, dtype=np.float32) * g.choice([-1.0, 1.0], n).astype(np.float32)
    big = np.array([FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX, 1.0, -1.0, 0.0, -0.0, 0.0, -0.0, 1.0], dtype=np.float32)
    big2 = np.array([FLT_MAX, TINY, -FLT_MAX, -TINY, TINY, TINY, 0.0, -0.0, -0.0, 0.0, -1.0], dtype=np.float32)
    A = np.concatenate([a, c, c, a, big])
    B = np.concatenate([b, near, tiny, -a, big2])
    ok = np.isfinite(A) & np.isfinite(B)
    return A[ok], B[ok]


def test_directed_sums_against_exact_arithmetic():
    A, B = _float_pairs()
    assert A.size > 5000
    lo, hi = sr.sub_rd32(A, B), sr.add_ru32(A, B)
    for a, b, l, h in zip(A.tolist(), B.tolist(), lo.tolist(), hi.tolist()):
        d, s = Fraction(a) - Fraction(b), Fraction(a) + Fraction(b)
        assert l == _round_frac(d, True), (a, b, l)
        assert h == _round_frac(s, False), (a, b, h)
    # a double rounding would get these wrong: 1 - 2^-149 rounds down to the float below 1, 1 + 2^-149 up to the float above
    one, t = np.float32(1.0), np.float32(TINY)
    assert sr.sub_rd32(one, t) == np.nextafter(one, np.float32(0)) and sr.add_ru32(one, t) == np.nextafter(one, np.float32(2))
    assert sr.sub_rd32(one, -t) == one and sr.add_ru32(one, -t) == one
    # exact zeros: x - x is -0 rounding down, x + (-x) is +0 rounding up; infinities pass through
    assert sr.bits1(sr.sub_rd32(one, one)) == 0x80000000 and sr.bits1(sr.add_ru32(one, -one)) == 0
    assert sr.bits1(sr.sub_rd32(np.float32(0.0), np.float32(-0.0))) == 0 and sr.bits1(sr.add_ru32(np.float32(-0.0), np.float32(-0.0))) == 0x80000000
    inf = np.float32(np.inf)
    assert sr.sub_rd32(one, inf) == -inf and sr.add_ru32(one, inf) == inf and sr.sub_rd32(-inf, inf) == -inf and sr.add_ru32(inf, inf) == inf
    assert sr.sub_rd32(np.float32(-FLT_MAX), np.float32(FLT_MAX)) == -inf and sr.add_ru32(np.float32(-FLT_MAX), np.float32(-FLT_MAX)) == np.float32(-FLT_MAX)


def test_pad_and_m_bits():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -3.0000001], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]])
    t = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.uint32)
    x1 = v.copy(); x1[1, 0] = 1e39
    assert sr.m_bits(v, v, t) == int(sr.bits1(sr.ru32(3.0000001)))
    assert sr.m_bits(v, x1, t) == 0x7F800000 and sr.pad(0x7F800000, 0.01) == np.inf
    assert sr.m_bits(v, v, t[:1]) == 0                                         # one triangle: no refit, M stays 0
    vz = np.concatenate([v, np.full((3, 3), -0.0)]); tz = np.concatenate([t, np.array([[6, 7, 8]], dtype=np.uint32)])
    assert sr.m_bits(vz, vz, tz) == sr.m_bits(v, v, t)                         # a leaf of -0.0 coordinates adds a zero, whatever its sign
    assert sr.m_bits_between(v, v, t[:1], v, v, t[1:]) == int(sr.bits1(np.float32(1.0)))   # b of one leaf: a's M alone
    assert sr.m_bits_between(v, v, t[:1], v, v, t) == sr.m_bits(v, v, t)
    for mb, dist in ((0, 0.01), (sr.m_bits(v, v, t), 0.01), (0x7F7FFFFF, 1e-30), (0x00000001, 1e-50), (0, 1.7976931348623157e308)):
        m = Fraction(float(np.array([mb], dtype=np.uint32).view(np.float32)[0]))
        exact = 2 * Fraction(dist) * (1 + Fraction(1, 1 << 20)) + m * Fraction(1, 1 << 20)
        p = float(sr.pad(mb, dist))
        if np.isfinite(p):                                                     # the FP64 sum is within three roundings of the exact value
            assert Fraction(p) >= exact * (1 - Fraction(1, 1 << 50)) and Fraction(p) <= exact * (1 + Fraction(1, 1 << 22)) + Fraction(TINY)
        else:
            assert exact > Fraction(FLT_MAX) * (1 - Fraction(1, 1 << 50))


def _small_meshes():
    v, i = synth.soup(3000, e=0.05, seed=3); yield "soup3k", v, i, 0.05
    v, i = synth.cloth_pair(20, round_f32=False); yield "cloth20d", v, i, 2.88 / 20
    verts, vidx = synth.soup(500, 0.2, 21)                                      # test_proximity_gpu._meshes' duplicates mesh
    v2 = np.concatenate([verts, verts[:300]], axis=0)
    dup = (np.arange(300, dtype=np.uint32) + verts.shape[0]).reshape(100, 3)
    vi = np.concatenate([vidx, dup, np.array([[0, 0, 1], [5, 5, 5]], dtype=np.uint32), vidx[:50]], axis=0)
    yield "duplicates", v2, vi, 0.2
    v, i = _comb([1 << (59 - k) for k in range(60)]); yield "comb", v, i, 0.2
    for n in (2, 3, 65):
        v, i = synth.soup(n, e=0.3, seed=n); yield f"n{n}", v, i, 0.3


def _move(verts, edge, seed):
    g = np.random.default_rng(seed)
    return verts + g.normal(size=verts.shape) * edge * 0.3 + g.normal(size=(1, 3)) * edge


def _naive_halves(r, lo, hi):
    """Bottom-up union over the oracle's tree (Karras numbering), children before parents by range length."""
    left, right, rf, rl = (np.asarray(r[k], dtype=np.int64) for k in ("left", "right", "range_first", "range_last"))
    n = left.shape[0] + 1
    blo = np.concatenate([np.zeros((n - 1, 3), dtype=np.float32), lo])
    bhi = np.concatenate([np.zeros((n - 1, 3), dtype=np.float32), hi])
    for idx in np.argsort(rl - rf, kind="stable"):
        a, b = left[idx], right[idx]
        blo[idx] = np.minimum(blo[a], blo[b]); bhi[idx] = np.maximum(bhi[a], bhi[b])
    return blo, bhi, left, right


@pytest.mark.parametrize("name,verts,vidx,edge", list(_small_meshes()), ids=lambda x: x if isinstance(x, str) else "")
def test_swept_records_against_naive_recursion(name, verts, vidx, edge):
    x1 = _move(verts, edge, 3)
    # (the comb is 60 levels deep in the frame of test_cd_gpu.py's deep-tree test: one leaf's climb runs the whole chain)
    r = oracle.pipeline(verts, vidx, off=np.zeros(3), span=np.full(3, 1048576.0)) if name == "comb" else oracle.pipeline(verts, vidx)
    n = vidx.shape[0]
    lo, hi = sr.swept_leaf_boxes(verts, x1, vidx, r["perm"])
    six = np.concatenate([verts[vidx.astype(np.int64)], x1[vidx.astype(np.int64)]], axis=1)[r["perm"].astype(np.int64)]
    assert np.all(lo.astype(np.float64) <= six.min(axis=1)) and np.all(hi.astype(np.float64) >= six.max(axis=1))
    (L, R, F, La), split_of = sr.tree_from_karras(r["left"], r["right"], r["range_first"], r["range_last"])
    assert sorted(split_of.tolist()) == list(range(n - 1))
    root = sr.check_tree(L, R, F, La)
    up = sr.parents(L, R)
    assert up[n + root] == -1 and np.count_nonzero(up == -1) == 1
    if name == "comb":
        assert max(sr.depth_of(s, up, n) for s in range(n - 1)) >= 60
    l_lo, l_hi, r_lo, r_hi = sr.swept_records((lo, hi), L, R, F, La)
    blo, bhi, left, right = _naive_halves(r, lo, hi)
    for idx in range(n - 1):
        s = split_of[idx]
        assert np.array_equal(sr.bits(l_lo[s]), sr.bits(blo[left[idx]])) and np.array_equal(sr.bits(l_hi[s]), sr.bits(bhi[left[idx]])), (name, idx)
        assert np.array_equal(sr.bits(r_lo[s]), sr.bits(blo[right[idx]])) and np.array_equal(sr.bits(r_hi[s]), sr.bits(bhi[right[idx]])), (name, idx)


def test_check_tree_rejects_a_wrong_tree():
    verts, vidx = synth.soup(200, e=0.1, seed=5)
    r = oracle.pipeline(verts, vidx)
    (L, R, F, La), _ = sr.tree_from_karras(r["left"], r["right"], r["range_first"], r["range_last"])
    sr.check_tree(L, R, F, La)
    k = int(np.nonzero(L >= 0)[0][0])
    for arr, val in ((L, L[k] + 1 if L[k] + 1 != k else L[k] - 1), (La, La[k] - 1 if La[k] - 1 > k else La[k] + 1)):
        a = arr.copy(); a[k] = val
        with pytest.raises(AssertionError):
            sr.check_tree(*(a if x is arr else x for x in (L, R, F, La)))


def test_grid_candidate_count_equals_all_pairs():
    verts, vidx = synth.soup(1800, e=0.05, seed=8)
    x1 = _move(verts, 0.05, 4)
    perm = oracle.pipeline(verts, vidx)["perm"]
    lo, hi = sr.swept_leaf_boxes(verts, x1, vidx, perm)
    for dist in (0.005, 0.03):
        p = sr.pad(sr.m_bits(verts, x1, vidx), dist)
        a = sr.expected_candidates(lo, hi, p, brute=True)
        b = sr.expected_candidates(lo, hi, p, brute=False)
        assert a == b and a > 0, (dist, a, b)
    naive = sum(int(sr._meets(*(q[j] for q in sr.query_boxes(lo, hi, p)), lo[j + 1:], hi[j + 1:]).sum()) for j in range(lo.shape[0] - 1))
    assert naive == a
    # between two meshes, and b of one leaf
    va, ia, vb, ib = br.split(*br.soup(1300, 0.06, 5), 700)
    x1a, x1b = br.motion(va, 0.03, 11), br.motion(vb, 0.03, 12)
    la, ha = sr.swept_leaf_boxes(va, x1a, ia, np.arange(ia.shape[0]))
    lb, hb = sr.swept_leaf_boxes(vb, x1b, ib, np.arange(ib.shape[0]))
    p = sr.pad(sr.m_bits_between(va, x1a, ia, vb, x1b, ib), 0.02)
    a = sr.expected_candidates(la, ha, p, lb, hb, brute=True)
    b = sr.expected_candidates(la, ha, p, lb, hb, brute=False)
    assert a == b and a > 0
    assert sr.expected_candidates(la, ha, p, lb[:1], hb[:1]) == la.shape[0]
    assert sr.expected_candidates(lo[:1], hi[:1], p) == 0


def _records(want, L, R, F, La):
    """Record halves u32[n, 8] holding the restatement's boxes: what a correct device would leave."""
    m = L.shape[0]
    rr, rl = np.zeros((m + 1, 8), dtype=np.uint32), np.zeros((m + 1, 8), dtype=np.uint32)
    l_lo, l_hi, r_lo, r_hi = want
    rl[:m, 0:3], rl[:m, 3:6], rl[:m, 6], rl[:m, 7] = sr.bits(l_lo), sr.bits(l_hi), L.view(np.uint32), F.astype(np.uint32)
    rr[:m, 0:3], rr[:m, 3:6], rr[:m, 6], rr[:m, 7] = sr.bits(r_lo), sr.bits(r_hi), R.view(np.uint32), La.astype(np.uint32) | np.uint32(0x80000000)
    return rr, rl


def test_comparison_reports_planted_errors():
    verts, vidx = synth.soup(3000, e=0.05, seed=3)
    x1 = _move(verts, 0.05, 3)
    r = oracle.pipeline(verts, vidx)
    n = vidx.shape[0]
    lo, hi = sr.swept_leaf_boxes(verts, x1, vidx, r["perm"])
    (L, R, F, La), _ = sr.tree_from_karras(r["left"], r["right"], r["range_first"], r["range_last"])
    want = sr.swept_records((lo, hi), L, R, F, La)
    rr, rl = _records(want, L, R, F, La)
    up = sr.parents(L, R)
    assert sr.compare_links(rr, rl, rr, rl, up) == 2 * (n - 1)
    assert sr.compare_records(rr, rl, want, up) == 2 * (n - 1)
    # (a) one half's hi rounded to nearest instead of up: pick a leaf half whose hi the nearest rounding puts below the true bound
    six = np.concatenate([verts[vidx.astype(np.int64)], x1[vidx.astype(np.int64)]], axis=1)[r["perm"].astype(np.int64)]
    with np.errstate(over="ignore"):
        near = six.max(axis=1).astype(np.float32)
    j = int(np.nonzero((near != hi).any(axis=1) & (np.arange(n) > 0))[0][0])
    s, side = int(up[j]) >> 1, int(up[j]) & 1
    bad = [rr.copy(), rl.copy()]
    bad[1 - side][s, 3:6] = sr.bits(near[j])
    with pytest.raises(AssertionError, match=rf"split {s} {'left' if side == 0 else 'right'} half") as e:
        sr.compare_records(bad[0], bad[1], want, up)
    assert "1 of" in str(e.value) and f"leaves [{j}, {j}]" in str(e.value)
    # (b) one internal half left at its first-arriving child's box
    k = int(np.nonzero((L >= 0) & (F < np.arange(n - 1) - 4))[0][0])               # record k's left child is the node of split c
    c = int(L[k])
    bad = [rr.copy(), rl.copy()]
    bad[1][k, :6] = rl[c, :6]                                                  # ... whose own left child's box is all that arrived
    assert not np.array_equal(bad[1][k, :6], rl[k, :6])
    with pytest.raises(AssertionError, match=rf"split {k} left half, depth \d+, leaves \[{int(F[k])}, {k}\]"):
        sr.compare_records(bad[0], bad[1], want, up)
    # the sign of a zero: accepted on an internal half only where its leaves hold zeros of both signs in that bound
    zlo = lo.copy(); zlo[:, 0] = 0.0
    j0 = int(F[k])                                                             # a leaf under record k's left child ...
    zlo[j0, 0] = -0.0
    zwant = sr.swept_records((zlo, hi), L, R, F, La)
    zrr, zrl = _records(zwant, L, R, F, La)
    assert sr.compare_records(zrr, zrl, zwant, up, leaves=(zlo, hi)) == 2 * (n - 1)
    flip = zrl.copy(); flip[k, 0] ^= np.uint32(0x80000000)
    assert sr.compare_records(zrr, flip, zwant, up, leaves=(zlo, hi)) == 2 * (n - 1)      # both signs below: either passes
    with pytest.raises(AssertionError, match=rf"split {k} left half"):
        sr.compare_records(zrr, flip, zwant, up)                               # (not without the leaves)
    other = int(np.nonzero((L >= 0) & ((F > j0) | (np.arange(n - 1) < j0)))[0][0])        # ... and a left child without that leaf
    flip = zrl.copy(); flip[other, 0] ^= np.uint32(0x80000000)
    with pytest.raises(AssertionError, match=rf"split {other} left half"):
        sr.compare_records(zrr, flip, zwant, up, leaves=(zlo, hi))
    leafhalf = int(np.nonzero(L < 0)[0][0])
    flip = zrl.copy(); flip[leafhalf, 0] ^= np.uint32(0x80000000)
    with pytest.raises(AssertionError, match=rf"split {leafhalf} left half"):
        sr.compare_records(zrr, flip, zwant, up, leaves=(zlo, hi))
    # a wrong link, a stale up[] word
    bad_l = rl.copy(); bad_l[k, 6] = rl[k, 6] + 1
    with pytest.raises(AssertionError):
        sr.compare_links(rr, rl, rr, bad_l, up)
    bad_up = up.copy(); bad_up[n + c] = -1
    with pytest.raises(AssertionError, match="inverse"):
        sr.compare_links(rr, rl, rr, rl, bad_up)
    # (c) a pad computed without its M term, (d) one candidate dropped
    mb, dist = sr.m_bits(verts, x1, vidx), 0.005
    p = sr.compare_pad(mb, sr.pad(mb, dist), mb, dist)
    with pytest.raises(AssertionError, match="pad"):
        sr.compare_pad(mb, sr.pad(0, dist), mb, dist)
    with pytest.raises(AssertionError, match="m_bits"):
        sr.compare_pad(mb - 1, sr.pad(mb, dist), mb, dist)
    count = sr.expected_candidates(lo, hi, p)
    assert count > 0 and sr.expected_candidates(lo, hi, sr.pad(0, dist)) <= count
    assert sr.compare_count(count, count) == count
    with pytest.raises(AssertionError, match="candidates"):
        sr.compare_count(count - 1, count)
