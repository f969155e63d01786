"""The swept tree of the continuous collision queries on the device (k_ccd_links + k_ccd_refit, read back with cd_debug_swept) and
what its walk finds, against the exact restatement (tests/swept_ref.py): every record half bit for bit, every link, up[], M, the pad
and the number of candidates.  No tolerance, nothing sampled: each case prints how many record halves it compared.

The records, up[] and M are device data.  The pad cd_debug_swept returns is not: the descent computes ccd_pad in registers, and the
reader gives its host twin (the same FP64 sum from M and dist, rounded up), so comparing it pins the twin and M.  The device's own
pad is held by the candidate count, which is exact and moves with the pad.

The candidate count is compared wherever the CPU count is affordable: every case here except the 1 M and 4 M cloths (their trees are
compared whole; the largest mesh whose pairs of query box and leaf box are counted on the CPU is cloth_pair(300), 360 k triangles).  Pair lists are
compared with the restatements of tests/ccd_ref.py and tests/between_ref.py through the existing helpers on the meshes on which
tests/test_ccd_gpu.py and tests/test_between_gpu.py do it."""
from __future__ import annotations

import numpy as np
import pytest

import between_ref as br
import ccd_ref as cr
import mi355_synth as synth
import mi355cd
import scale_inputs as si
import swept_ref as sr
from test_between_gpu import CASES, _same_ccd
from test_ccd_gpu import _move, _same
from query_meshes import _meshes

pytestmark = pytest.mark.gpu

BIG = ("soup100k", "cloth300", "cloth300d")
DEEP_FRAME = (np.zeros(3), np.full(3, 1048576.0))       # the frame in which the comb is 60 levels deep (test_cd_gpu.py's deep-tree test)


def _read(cd, other=None):
    """The swept tree `cd` holds (its own, or other's after find_ccd_between) with the static records and the order it lies over."""
    srr, srl, up, mb, pad = cd.debug_swept(other)
    owner = cd if other is None else other
    rr, rl, _, _ = owner.debug_records()
    _, perm = owner.export_keys()
    return dict(srr=srr, srl=srl, up=up, m_bits=mb, pad=pad, rr=rr, rl=rl, perm=perm)


def _check_tree(t, x0, x1, vidx, what):
    """Links, up[] and every box float of the read-back `t` against the restatement on (x0, x1).  Returns (halves compared, (lo, hi) of
    the sorted leaves)."""
    n = vidx.shape[0]
    lo, hi = sr.swept_leaf_boxes(x0, x1, vidx, t["perm"])
    if n < 2:                                                                  # no records: nothing was read, nothing to compare
        assert t["srr"].shape[0] == 0 and t["srl"].shape[0] == 0 and t["up"].shape[0] == 0, what
        return 0, (lo, hi)
    halves = sr.compare_links(t["rr"], t["rl"], t["srr"], t["srl"], t["up"])
    want = sr.swept_records((lo, hi), *sr.tree_from_records(t["rr"], t["rl"]))
    assert sr.compare_records(t["srr"], t["srl"], want, t["up"], what, leaves=(lo, hi)) == halves == 2 * (n - 1)
    return halves, (lo, hi)


def _check_self(cd, x0, x1, vidx, dist, what, count=True):
    """After a CCD call on cd: the whole swept tree, M, the pad and (count) the candidates of the final pass."""
    t = _read(cd)
    halves, (lo, hi) = _check_tree(t, x0, x1, vidx, what)
    t["leaves"] = (lo, hi)
    p = sr.compare_pad(t["m_bits"], t["pad"], sr.m_bits(x0, x1, vidx), dist)
    cands = None
    if count:
        cands = sr.compare_count(cd.ccd_info.n_candidates, sr.expected_candidates(lo, hi, p), what)
    print(f"{what}: {halves} record halves compared, M bits {t['m_bits']:#010x}, pad {float(p)!r}, candidates {cands if count else 'not counted'}")
    return t


def _depth(t):
    n = t["srr"].shape[0]
    up = t["up"]
    d = np.zeros(n, dtype=np.int64)
    u = up[:n].astype(np.int64)
    live = u >= 0
    while live.any():
        d[live] += 1
        u = np.where(live, up[n + (np.maximum(u, 0) >> 1)], -1).astype(np.int64)
        live = u >= 0
    return int(d.max())


@pytest.mark.parametrize("name,verts,vidx,ids,edge", list(_meshes()), ids=lambda x: x if isinstance(x, str) else "")
def test_swept_tree_matches_restatement(name, verts, vidx, ids, edge):
    x1 = _move(verts, edge, 3)
    dists = (edge / 10,) if name in BIG else (edge / 10, edge / 2)
    with mi355cd.CollisionDetector(verts, vidx, ids) as cd:
        for k, d in enumerate(dists):
            got = cd.self_ccd(x1, d, cap=1 << 22) if k == 0 else cd.find_ccd(x1, d, cap=1 << 22)
            assert got[4] == mi355cd.CD_OK, (name, d)
            _check_self(cd, verts, x1, vidx, d, f"{name} dist={d:g}")
            if k == 0 and name not in BIG:
                _same(got, cr.ccd_pairs(verts, x1, vidx, ids, d))
        if name == "comb":                                                     # one lane climbs the whole chain
            cd.set_morton_frame(mi355cd.CD_FRAME_CUSTOM, *DEEP_FRAME)
            got = cd.self_ccd(x1, edge / 10, cap=1 << 22)
            t = _check_self(cd, verts, x1, vidx, edge / 10, "comb in its deep frame")
            assert _depth(t) >= 60, _depth(t)
            _same(got, cr.ccd_pairs(verts, x1, vidx, ids, edge / 10))


def test_order_error_before_any_ccd_pass():
    verts, vidx = synth.soup(500, e=0.1, seed=2)
    with mi355cd.CollisionDetector(verts, vidx) as cd, mi355cd.CollisionDetector(verts + 0.01, vidx) as other:
        cd.build_tree(); other.build_tree()
        for o in (None, other):
            with pytest.raises(mi355cd.CdError) as e:
                cd.debug_swept(o)
            assert e.value.rc == mi355cd.CD_ERR_ORDER
        cd.find_ccd(verts + 0.01, 0.01)
        cd.debug_swept()
        with pytest.raises(mi355cd.CdError) as e:                              # the two trees are told apart
            cd.debug_swept(other)
        assert e.value.rc == mi355cd.CD_ERR_ORDER
        assert cd.lib.cd_debug_swept(cd._ctx, 2, None, None, None, None, None) == mi355cd.CD_ERR_ARG


def test_after_candidate_regrowth():
    """Every pair a candidate: far more than the first candidate buffer holds, so the pass is redone on a grown buffer; the tree and the
    count are those of the final pass."""
    v, vidx = si.box_soup(1500, 0.3, 1.0, 3.0, 21)
    x1 = si.motion(v, 0.3, seed=8)
    big = float(np.ceil(np.linalg.norm(np.maximum(v.max(0), x1.max(0)) - np.minimum(v.min(0), x1.min(0)))))
    n = vidx.shape[0]
    with mi355cd.CollisionDetector(v, vidx) as cd:
        cd.build_tree()
        cd.find_ccd(x1, big, cap=16)
        assert cd.ccd_info.n_candidates == n * (n - 1) // 2 > 64 * max(4096, (16 * n + 63) // 64)
        _check_self(cd, v, x1, vidx, big, "all pairs, grown buffer")
        cd.find_ccd(x1, 0.05, cap=16)
        _check_self(cd, v, x1, vidx, 0.05, "small dist on the grown buffer")


def _boxes_equal(a, b):
    """Per split: (left halves equal, right halves equal) of two read-backs, box floats only."""
    m = a["srr"].shape[0] - 1
    return np.all(a["srl"][:m, :6] == b["srl"][:m, :6], axis=1), np.all(a["srr"][:m, :6] == b["srr"][:m, :6], axis=1)


@pytest.fixture(scope="module")
def cloth1m():
    return synth.cloth_pair(500)


def test_cloth_1m_repeated_calls_thrown_vertex_and_no_motion(cloth1m):
    """cloth_pair(500) under cloth_motion: about 2 M record halves compared whole, four times over: the same call twice and other end
    positions after it (arrival counters and up[] start clean every time), one thrown vertex (only the halves on the root paths of
    its triangles change), and x1 == x0 (every half is the outward-rounded static FP64 box).  The candidates are not counted here."""
    verts, vidx = cloth1m
    n = vidx.shape[0]
    dist = 0.001
    x1 = synth.cloth_motion(verts, approach=0.5, wave=0.5)
    x1t = synth.cloth_motion(verts, approach=0.5, wave=0.5, throw=True)
    kv = np.nonzero(np.any(x1t != x1, axis=1))[0]
    assert kv.size == 1
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        cd.find_ccd(x1, dist, cap=16)
        base = _check_self(cd, verts, x1, vidx, dist, "cloth 1 M", count=False)
        assert base["srr"].shape[0] == n
        c0 = cd.ccd_info.n_candidates
        cd.find_ccd(x1, dist, cap=16)
        again = _check_self(cd, verts, x1, vidx, dist, "cloth 1 M, the same call again", count=False)
        assert all(e.all() for e in _boxes_equal(base, again)) and cd.ccd_info.n_candidates == c0
        # one thrown vertex
        cd.find_ccd(x1t, dist, cap=16)
        thrown = _check_self(cd, verts, x1t, vidx, dist, "cloth 1 M, one vertex thrown", count=False)
        inv = np.empty(n, dtype=np.int64); inv[base["perm"].astype(np.int64)] = np.arange(n)
        leaves = inv[np.nonzero(np.any(vidx == kv[0], axis=1))[0]]
        up = thrown["up"]
        may = [np.zeros(n - 1, dtype=bool), np.zeros(n - 1, dtype=bool)]      # by side: the halves on those leaves' root paths
        eq = _boxes_equal(base, thrown)
        for j in leaves.tolist():
            u = int(up[j])
            assert not eq[u & 1][u >> 1], ("the leaf-level half of a triangle of the thrown vertex did not change", j)
            while u >= 0:
                may[u & 1][u >> 1] = True
                u = int(up[n + (u >> 1)])
        for side in (0, 1):
            off = np.nonzero(~eq[side] & ~may[side])[0]
            assert off.size == 0, ("halves off the thrown vertex's root paths changed", side, off[:5])
        changed = int((~eq[0]).sum() + (~eq[1]).sum())
        print(f"thrown vertex: {leaves.size} triangles, {changed} of {2 * (n - 1)} halves changed, all on their root paths ({int(may[0].sum() + may[1].sum())} halves)")
        # other end positions after it: back to x1 exactly
        cd.find_ccd(x1, dist, cap=16)
        back = _check_self(cd, verts, x1, vidx, dist, "cloth 1 M, back to the first end positions", count=False)
        assert all(e.all() for e in _boxes_equal(base, back)) and cd.ccd_info.n_candidates == c0
        # no motion: the static FP64 tree, rounded outward
        cd.find_ccd(verts, dist, cap=16)
        still = _check_self(cd, verts, verts, vidx, dist, "cloth 1 M, x1 == x0", count=False)
        parent, left, right, boxes, bounded = cd.export_tree()
    left, right = left.astype(np.int64), right.astype(np.int64)
    split_of = np.where(left >= n - 1, left - (n - 1), left)
    want = [np.zeros((n - 1, 3), dtype=np.float32) for _ in range(4)]
    want[0][split_of], want[1][split_of] = sr.rd32(boxes[left][:, 0::2]), sr.ru32(boxes[left][:, 1::2])
    want[2][split_of], want[3][split_of] = sr.rd32(boxes[right][:, 0::2]), sr.ru32(boxes[right][:, 1::2])
    assert sr.compare_records(still["srr"], still["srl"], tuple(want), still["up"], "x1 == x0 against the static FP64 boxes",
                              leaves=still["leaves"]) == 2 * (n - 1)


def test_cloth_4m_whole_tree():
    """cloth_pair(1000), 4 M triangles: all of its about 8 M record halves, M and the pad.  The candidates are not counted here."""
    verts, vidx = synth.cloth_pair(1000)
    n = vidx.shape[0]
    assert n == 4_000_000
    x1 = synth.cloth_motion(verts, approach=0.5, wave=0.5, quads=1000)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        got = cd.self_ccd(x1, 0.0005, cap=16)
        assert got[4] in (mi355cd.CD_OK, mi355cd.CD_OVERFLOW) and got[3] > 0
        t = _check_self(cd, verts, x1, vidx, 0.0005, "cloth 4 M", count=False)
        assert t["srr"].shape[0] == n


@pytest.mark.parametrize("build", ["fused", "stagewise", "auto_frame", "no_cell_table"])
def test_every_build_of_the_static_tree(build):
    verts, vidx = synth.cloth_pair(100, round_f32=False)
    edge = 2.88 / 100
    x1 = _move(verts, edge, 5)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        if build == "stagewise":
            cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 1)
        elif build == "auto_frame":
            cd.set_morton_frame(mi355cd.CD_FRAME_AUTO)
        elif build == "no_cell_table":
            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, 0)
        got = cd.self_ccd(x1, edge / 10, cap=1 << 22)
        assert got[4] == mi355cd.CD_OK
        assert cd.debug_get(mi355cd.CD_DBG_GET_TREE_WAS_FUSED) == (0 if build == "stagewise" else 1)
        _check_self(cd, verts, x1, vidx, edge / 10, f"cloth100d, {build} build")


SCALE_MESHES = si.meshes()


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(SCALE_MESHES))
def test_fp32_range(name, k):
    """tests/scale_inputs.py's meshes scaled by 2^k over the whole band of tests/test_query_scales_gpu.py: bounds that become +-inf,
    FLT_MAX, subnormal or 0 are the directed roundings, and the pad may be +inf."""
    v, vidx, edge = SCALE_MESHES[name]
    verts, x1 = si.scaled(v, k), si.scaled(si.motion(v, edge), k)
    dist = float(np.ldexp(edge / 4, k))
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.build_tree()
        got = cd.find_ccd(x1, dist, cap=1 << 20)
        assert got[4] == mi355cd.CD_OK
        t = _check_self(cd, verts, x1, vidx, dist, f"{name} k={k}")
    m = max(vidx.shape[0] - 1, 0)
    box = np.concatenate([t["srr"][:m, :6], t["srl"][:m, :6]]).view(np.float32)
    if k >= 128:                                                               # the range end is really reached
        assert np.isinf(box).any() and (np.abs(box) == np.float32(si.FLT_MAX)).any(), (name, k)
    if k >= 149:
        assert np.isinf(t["pad"]), (name, k, t["pad"])
    if k <= -200:
        assert np.all(np.abs(box) <= np.float32(2.0 ** -149)) and (box == 0).any(), (name, k)


# ---------------------------------------------------------------- between two meshes
def _check_between(a, b, ma, mb, dist, what, want=None):
    """a.find_ccd_between(b) on meshes (x0, x1 or None, vidx) and b's swept tree as a holds it, M over both meshes, the pad and the
    candidates of the between descent; want: the restatement's pairs."""
    (va, x1a, ia), (vb, x1b, ib) = ma, mb
    got = a.find_ccd_between(b, dist, x1a, x1b, cap=1 << 20)
    assert got[4] == mi355cd.CD_OK, what
    if want is not None:
        _same_ccd(got, want, what)
    ea, eb = (va if x1a is None else x1a), (vb if x1b is None else x1b)
    t = _read(a, b)
    halves, (lo_b, hi_b) = _check_tree(t, vb, eb, ib, what)
    p = sr.compare_pad(t["m_bits"], t["pad"], sr.m_bits_between(va, ea, ia, vb, eb, ib), dist)
    lo_a, hi_a = sr.swept_leaf_boxes(va, ea, ia, a.export_keys()[1])
    cands = sr.compare_count(a.ccd_info.n_candidates, sr.expected_candidates(lo_a, hi_a, p, lo_b, hi_b), what)
    print(f"{what}: {halves} record halves compared, M bits {t['m_bits']:#010x}, pad {float(p)!r}, candidates {cands}")
    return t


def _with_point_at_minus_zero(n, seed):
    """A soup of n triangles plus one degenerate triangle whose three vertices are (-0.0, -0.0, -0.0): the largest |coordinate| of
    that leaf is a zero with the sign bit set."""
    v, i = br.soup(n, 0.08, seed)
    v = np.concatenate([v, np.full((3, 3), -0.0)])
    i = np.concatenate([i, np.array([[3 * n, 3 * n + 1, 3 * n + 2]], dtype=np.uint32)])
    x1 = br.motion(v, 0.03, seed + 100)
    x1[3 * n:] = -0.0                                                          # the point stays where it is, sign included
    assert np.all(np.signbit(v[3 * n:])) and np.all(np.signbit(x1[3 * n:]))
    return v, x1, i


def test_a_leaf_of_minus_zeros_does_not_take_m():
    """M is the largest |coordinate| over the leaves, kept as fp32 bits under an unsigned maximum.  A leaf whose six points are all
    -0.0 has |coordinate| -0.0 under the device's compare-and-select abs: its bits must not beat every positive M (the pad would lose
    its M 2^-20 term for the whole mesh).  Self (k_ccd_refit), and between two meshes with that leaf on a's side (k_between_mbits)
    and on b's (k_ccd_refit over b)."""
    v, x1, i = _with_point_at_minus_zero(400, 51)
    assert sr.m_bits(v, x1, i) not in (0, 0x80000000)
    vb, ib = br.soup(300, 0.08, 52)
    x1b = br.motion(vb, 0.03, 53)
    with mi355cd.CollisionDetector(v, i) as cd, mi355cd.CollisionDetector(vb, ib) as b:
        got = cd.self_ccd(x1, 0.01, cap=1 << 20)
        _check_self(cd, v, x1, i, 0.01, "soup + a point at -0.0")
        _same(got, cr.ccd_pairs(v, x1, i, None, 0.01))
        cd.find_ccd(v, 0.01, cap=1 << 20)
        _check_self(cd, v, v, i, 0.01, "soup + a point at -0.0, x1 == x0")
        b.build_tree()
        _check_between(cd, b, (v, x1, i), (vb, x1b, ib), 0.01, "the point at -0.0 in a", br.ccd_pairs(v, i, vb, ib, 0.01, x1, x1b))
        _check_between(b, cd, (vb, x1b, ib), (v, x1, i), 0.01, "the point at -0.0 in b", br.ccd_pairs(vb, ib, v, i, 0.01, x1b, x1))
        _check_between(b, cd, (vb, None, ib), (v, None, i), 0.01, "the point at -0.0 in b, nothing moves")


@pytest.mark.parametrize("name", ["soup_1500_500_s6", "soup_1_400_s2", "soup_400_1_s3", "shared_positions"])
def test_between_two_meshes(name):
    va, ia, vb, ib = CASES[name]
    x1a, x1b = br.motion(va, 0.03, 11), br.motion(vb, 0.03, 12)
    dist = 0.01
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vb, ib) as b:
        a.build_tree(); b.build_tree()
        _check_between(a, b, (va, x1a, ia), (vb, x1b, ib), dist, f"{name}, both moving", br.ccd_pairs(va, ia, vb, ib, dist, x1a, x1b))
        _check_between(a, b, (va, x1a, ia), (vb, None, ib), dist, f"{name}, b static", br.ccd_pairs(va, ia, vb, ib, dist, x1a, None))
        _check_between(b, a, (vb, x1b, ib), (va, x1a, ia), dist, f"{name}, roles swapped", br.ccd_pairs(vb, ib, va, ia, dist, x1b, x1a))
        _check_between(b, a, (vb, x1b, ib), (va, None, ia), dist, f"{name}, roles swapped, b static", br.ccd_pairs(vb, ib, va, ia, dist, x1b, None))


def test_between_smaller_b_after_a_larger_one():
    """The buffers a keeps for b's swept tree were sized by a larger b: the second call reads and writes only the smaller tree's part."""
    va, ia = br.soup(600, 0.06, 41)
    vbig, ibig = br.soup(1500, 0.06, 42)
    vsmall, ismall = br.soup(130, 0.06, 43)
    vone, ione = br.soup(1, 0.3, 44, 0.4, 0.6)
    x1a = br.motion(va, 0.03, 1)
    with mi355cd.CollisionDetector(va, ia) as a, mi355cd.CollisionDetector(vbig, ibig) as big, \
            mi355cd.CollisionDetector(vsmall, ismall) as small, mi355cd.CollisionDetector(vone, ione) as one:
        for cd in (a, big, small, one):
            cd.build_tree()
        ma = (va, x1a, ia)
        tb = _check_between(a, big, ma, (vbig, br.motion(vbig, 0.03, 2), ibig), 0.01, "larger b")
        x1s = br.motion(vsmall, 0.03, 3)
        ts = _check_between(a, small, ma, (vsmall, x1s, ismall), 0.01, "smaller b after it", br.ccd_pairs(va, ia, vsmall, ismall, 0.01, x1a, x1s))
        assert ts["srr"].shape[0] == 130 and tb["srr"].shape[0] == 1500
        _check_between(a, one, ma, (vone, None, ione), 0.01, "b of one triangle after it", br.ccd_pairs(va, ia, vone, ione, 0.01, x1a, None))
        assert a.ccd_info.n_candidates == ia.shape[0]
        _check_between(a, big, ma, (vbig, None, ibig), 0.01, "the larger b again, static")
