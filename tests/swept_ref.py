"""CPU restatement of the swept tree of the continuous collision queries (csrc/cd_ccd.h k_ccd_links + k_ccd_refit) and of what its
walk must find (k_ccd_descend / k_between_descend through prox_walk<HiTrue>), exact: numpy, FP64 and fp32 with directed rounding.

The swept tree is determined by its inputs.  A leaf's box is the FP64 box of its six points (x0 and x1) rounded outward to fp32
(rd32 / ru32); a record half is the fp32 min / max over the leaves of the child it describes, and every node of the tree covers a
contiguous range of sorted leaves, so each of the 2 (n - 1) halves is a range-min / range-max over the sorted leaf boxes with one
right bit pattern.  (The one freedom: a zero bound of an internal half carries the sign of whichever child arrived with it when the
range holds zeros of both signs -- compare_records accepts either sign there, and only there; a leaf's own box follows the device's
order of comparisons, signs of zeros included.)  Because every ancestor's box contains its leaves' boxes exactly, the
walk reaches leaf k if and only if leaf k's own box meets the query box: the number of candidates has one right value too.

Split naming (csrc/cd_bvh.h): the record of the internal node whose left child ends at sorted leaf s is record s, s in [0, n - 2];
its left child covers [first[s], s], its right child [s + 1, last[s]]; a child link is the child's own split, or ~j for leaf j.
"""
from __future__ import annotations

import numpy as np

import proximity_ref as pr

REC_MASK = 0x3FFFFFFF                       # cd_bvh.h REC_LAST_MASK: the range word without its flag bits
SLACK = 2.0 ** -20                          # cd_proximity.h PROX_SLACK
REFIT_THREADS = 256                         # cd_ccd.h CCD_THREADS: leaves per workgroup of k_ccd_refit (failure reports only)
_NINF, _PINF = np.float32(-np.inf), np.float32(np.inf)


# ---------------------------------------------------------------- directed rounding
def rd32(x) -> np.ndarray:
    """double -> float toward -inf (__double2float_rd): rd32(1e39) = FLT_MAX, rd32(-1e39) = -inf."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
        return np.where(f.astype(np.float64) > x, np.nextafter(f, _NINF), f).astype(np.float32)


def ru32(x) -> np.ndarray:
    """double -> float toward +inf (__double2float_ru): ru32(1e39) = +inf, ru32(-1e39) = -FLT_MAX, ru32(-1e-60) = -0."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
        return np.where(f.astype(np.float64) < x, np.nextafter(f, _PINF), f).astype(np.float32)


def _directed_sum(a, b, down: bool) -> np.ndarray:
    """The fp32 sum a + b rounded toward -inf (down) or +inf, from the exact sum: s = RN64(a + b) and the two-sum error term e give
    a + b = s + e exactly (no overflow: the operands are floats).  s is the double nearest the sum, so no double -- hence no float --
    lies strictly between them: the directed rounding of s is right unless s is itself a float and e points the other way."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    a, b = np.broadcast_arrays(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        s = a + b
        bb = s - a
        e = (a - (s - bb)) + (b - bb)
        r = rd32(s) if down else ru32(s)
        exact = r.astype(np.float64) == s
        if down:
            r = np.where(exact & (e < 0.0), np.nextafter(r, _NINF), r)
        else:
            r = np.where(exact & (e > 0.0), np.nextafter(r, _PINF), r)
    # an exact zero: x + (-x) is -0 rounding down and +0 rounding up; zeros of one sign keep it
    zero = (s == 0.0) & (e == 0.0)
    both = (a == 0.0) & (b == 0.0) & (np.signbit(a) == np.signbit(b))
    z = np.where(both, np.where(np.signbit(a), -0.0, 0.0), -0.0 if down else 0.0)
    return np.where(zero, z, r).astype(np.float32)


def sub_rd32(a, b) -> np.ndarray:
    """a - b on fp32 operands rounded toward -inf (__ocml_sub_rtn_f32)."""
    return _directed_sum(a, -np.asarray(b, dtype=np.float32), True)


def add_ru32(a, b) -> np.ndarray:
    """a + b on fp32 operands rounded toward +inf (__ocml_add_rtp_f32)."""
    return _directed_sum(a, b, False)


def bits(f) -> np.ndarray:
    return np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)


def bits1(f) -> int:
    """The bit pattern of one fp32 value."""
    return int(np.asarray(f, dtype=np.float32).reshape(1).view(np.uint32)[0])


# ---------------------------------------------------------------- leaves, M and the pad
def _six(x0, x1, vidx):
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, 3)
    x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(vidx, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([x0[t], x1[t]], axis=1)                              # [n, 6, 3]


def _fold(pts, less):
    """The device's compare-selects over a triangle's three vertices (cd_math.h fmin3 / fmax3: the first of equals stays)."""
    t = pts[:, 0]
    for k in (1, 2):
        t = np.where(less(pts[:, k], t), pts[:, k], t)
    return t


def swept_leaf_boxes(x0, x1, vidx, perm):
    """(lo f32[n, 3], hi f32[n, 3]) per SORTED leaf j (triangle perm[j]): the FP64 box of its six points rounded outward, in the order
    of swept_box's comparisons (box_set at x0, box_set at x1, then fmin2 / fmax2 of the two: the second of equals wins there), so a
    bound that is zero has the device's sign when a triangle holds zeros of both signs."""
    six = _six(x0, x1, vidx)[np.asarray(perm, dtype=np.int64)]
    if six.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.float32)
    lt, gt = (lambda a, b: a < b), (lambda a, b: a > b)
    lo0, lo1, hi0, hi1 = _fold(six[:, :3], lt), _fold(six[:, 3:], lt), _fold(six[:, :3], gt), _fold(six[:, 3:], gt)
    return rd32(np.where(lo0 < lo1, lo0, lo1)), ru32(np.where(hi0 > hi1, hi0, hi1))


def _m64(x0, x1, vidx) -> float:
    six = _six(x0, x1, vidx)
    return float(np.max(np.abs(six))) if six.size else 0.0


def m_bits(x0, x1, vidx) -> int:
    """CcdState::m_bits after k_ccd_refit: the fp32 bits of the largest |coordinate| of the leaves' FP64 swept boxes, rounded up (ru32 is
    monotonic, so the largest of the roundings is the rounding of the largest).  One triangle: the refit does not run, 0."""
    if np.asarray(vidx).reshape(-1, 3).shape[0] < 2:
        return 0
    return int(bits1(ru32(_m64(x0, x1, vidx))))


def m_bits_between(a0, a1, ia, b0, b1, ib) -> int:
    """... of cd_find_ccd_between: k_between_mbits adds a's leaves beside what k_ccd_refit leaves for b's (which does not run when b
    is one triangle: a's alone then)."""
    m = _m64(a0, a1, ia)
    if np.asarray(ib).reshape(-1, 3).shape[0] >= 2:
        m = max(m, _m64(b0, b1, ib))
    return int(bits1(ru32(m)))


def pad(mbits: int, dist: float) -> np.float32:
    """ccd_pad: 2 dist + 2 dist 2^-20 + M 2^-20 in FP64 (left to right, no contraction), rounded up to fp32."""
    m = float(np.array([mbits], dtype=np.uint32).view(np.float32)[0])
    dist = float(dist)
    with np.errstate(over="ignore"):
        v = np.float64(2.0) * dist + np.float64(2.0) * dist * SLACK + np.float64(m) * SLACK
    return np.float32(ru32(v)[()])


# ---------------------------------------------------------------- the tree
def tree_from_records(rr, rl):
    """(left i32[n-1], right i32[n-1], first i64[n-1], last i64[n-1]) from record halves u32[n, 8] (right halves, left halves: the
    layout of cd_debug_records): slot n - 1 names no split."""
    n = rr.shape[0]
    m = max(n - 1, 0)
    left = np.ascontiguousarray(rl[:m, 6]).view(np.int32)
    right = np.ascontiguousarray(rr[:m, 6]).view(np.int32)
    return left, right, (rl[:m, 7] & REC_MASK).astype(np.int64), (rr[:m, 7] & REC_MASK).astype(np.int64)


def tree_from_karras(left, right, rf, rl):
    """The same from a tree in the oracle's numbering (oracle.build_hierarchy: internal nodes by Karras index, leaf j as n - 1 + j)
    -> (left, right, first, last) by split, and split_of[internal index]."""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    m = left.shape[0]
    n = m + 1
    split_of = np.where(left >= n - 1, left - (n - 1), left)                   # the left child ends at the split, whatever it is
    def link(c):
        return np.where(c >= n - 1, ~(c - (n - 1)), split_of[np.minimum(c, max(m - 1, 0))]).astype(np.int32)
    L, R = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    F, La = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    L[split_of], R[split_of] = link(left), link(right)
    F[split_of], La[split_of] = np.asarray(rf, dtype=np.int64), np.asarray(rl, dtype=np.int64)
    return (L, R, F, La), split_of


def check_tree(left, right, first, last):
    """left / right / first / last by split describe one binary tree over the contiguous leaf ranges [first[s], last[s]] of n leaves:
    every child is the node its parent's range implies.  Raises AssertionError otherwise.  Returns the root's split (-1: n < 2)."""
    m = left.shape[0]
    n = m + 1
    if m == 0:
        return -1
    s = np.arange(m, dtype=np.int64)
    assert np.all((first <= s) & (s < last) & (last <= n - 1)), "a split outside its own range"
    for name, c, want_leaf, leaf_is, f_want, l_want in (("left", left.astype(np.int64), first == s, s, first, s),
                                                        ("right", right.astype(np.int64), last == s + 1, s + 1, s + 1, last)):
        isleaf = c < 0
        bad = np.nonzero(isleaf != want_leaf)[0]
        assert bad.size == 0, (f"{name} child: leaf where a node is due or the reverse", bad[:5])
        assert np.array_equal(~c[isleaf], leaf_is[isleaf]), f"{name} child: the wrong leaf"
        ci = c[~isleaf]
        assert np.all((ci >= 0) & (ci < m)), f"{name} child: link out of range"
        assert np.array_equal(first[ci], f_want[~isleaf]) and np.array_equal(last[ci], l_want[~isleaf]), f"{name} child: not the range its parent implies"
    root = np.nonzero((first == 0) & (last == n - 1))[0]
    assert root.size == 1, ("roots", root[:5])
    return int(root[0])


def parents(left, right):
    """up[] as k_ccd_links leaves it: up[j] for leaf j, up[n + s] for the node of split s = (parent split << 1) | side; -1: the root."""
    m = left.shape[0]
    n = m + 1
    up = np.full(2 * n - 1, -1, dtype=np.int32)
    s = np.arange(m, dtype=np.int64)
    for c, side in ((left.astype(np.int64), 0), (right.astype(np.int64), 1)):
        at = np.where(c < 0, ~c, n + c)
        up[at] = ((s << 1) | side).astype(np.int32)
    return up


def _range_minmax(lo, hi, a, b):
    """min of lo[a[q] .. b[q]] and max of hi[a[q] .. b[q]] (inclusive, per column) for every q: a sparse table built one level at a
    time, each level answering the ranges whose length has that power of two -- O(n log n) work, two arrays of n at a time."""
    q = a.shape[0]
    out_lo = np.empty((q, lo.shape[1]), dtype=np.float32)
    out_hi = np.empty((q, hi.shape[1]), dtype=np.float32)
    if q == 0:
        return out_lo, out_hi
    assert np.all((0 <= a) & (a <= b) & (b < lo.shape[0]))
    lev = np.frexp((b - a + 1).astype(np.float64))[1] - 1                      # floor(log2(length))
    order = np.argsort(lev, kind="stable")
    cuts = np.searchsorted(lev[order], np.arange(int(lev.max()) + 2))
    tlo, thi = lo, hi
    for k in range(int(lev.max()) + 1):
        if k:
            h = 1 << (k - 1)
            tlo, thi = np.minimum(tlo[:-h], tlo[h:]), np.maximum(thi[:-h], thi[h:])
        sel = order[cuts[k]:cuts[k + 1]]
        if sel.size:
            i0, i1 = a[sel], b[sel] - (1 << k) + 1
            out_lo[sel] = np.minimum(tlo[i0], tlo[i1])
            out_hi[sel] = np.maximum(thi[i0], thi[i1])
    return out_lo, out_hi


def swept_records(leaf_boxes, left, right, first, last):
    """The expected box of every record half, by split: (l_lo, l_hi, r_lo, r_hi) f32[n - 1, 3] -- the left child's over the sorted
    leaves [first[s], s], the right child's over [s + 1, last[s]].  The tree is checked first (check_tree)."""
    lo, hi = leaf_boxes
    check_tree(left, right, first, last)
    m = left.shape[0]
    s = np.arange(m, dtype=np.int64)
    l_lo, l_hi = _range_minmax(lo, hi, np.asarray(first, dtype=np.int64), s)
    r_lo, r_hi = _range_minmax(lo, hi, s + 1, np.asarray(last, dtype=np.int64))
    return l_lo, l_hi, r_lo, r_hi


# ---------------------------------------------------------------- comparison (shared by the GPU tests and the CPU check of their teeth)
def depth_of(split: int, up, n: int) -> int:
    d, u = 0, int(up[n + split])
    while u >= 0 and d <= 2 * n:
        d += 1
        u = int(up[n + (u >> 1)])
    return d


def _describe(split, side, first, last, up, n):
    a, b = (int(first[split]), split) if side == 0 else (split + 1, int(last[split]))
    g0, g1 = a // REFIT_THREADS, b // REFIT_THREADS
    xcds = sorted({g % 8 for g in range(g0, min(g1, g0 + 7) + 1)})
    return (f"split {split} {'left' if side == 0 else 'right'} half, depth {depth_of(split, up, n) + 1}, leaves [{a}, {b}], "
            f"refit workgroups {g0}..{g1} (XCDs {xcds})")


def compare_links(rr, rl, srr, srl, up):
    """Links and range words of every swept half equal the static records'; up[] is the inverse of the links, -1 at the root."""
    n = rr.shape[0]
    m = max(n - 1, 0)
    for name, a, b in (("right", srr, rr), ("left", srl, rl)):
        bad = np.nonzero(np.any(a[:m, 6:8] != b[:m, 6:8], axis=1))[0]
        assert bad.size == 0, (f"{name} halves: link / range words differ from the static records'", bad.size, bad[:5], a[bad[:5], 6:8], b[bad[:5], 6:8])
    left, right, first, last = tree_from_records(rr, rl)
    root = check_tree(left, right, first, last)
    want = parents(left, right)
    bad = np.nonzero(np.asarray(up) != want)[0]
    assert bad.size == 0, ("up[] is not the inverse of the links", bad.size, bad[:5], np.asarray(up)[bad[:5]], want[bad[:5]])
    assert m == 0 or up[n + root] == -1
    return 2 * m


def _both_zero_signs(leaves, a, b):
    """bool[q, 6] per range [a[q], b[q]] of sorted leaves and bound (lo x y z, hi x y z): the range holds a -0 AND a +0 in that bound."""
    v = np.concatenate([bits(leaves[0]).reshape(-1, 3), bits(leaves[1]).reshape(-1, 3)], axis=1)
    ind = np.concatenate([v == np.uint32(0x80000000), v == np.uint32(0)], axis=1).astype(np.float32)
    _, any_ = _range_minmax(ind, ind, a, b)
    return (any_[:, :6] > 0) & (any_[:, 6:] > 0)


def compare_records(srr, srl, want, up, what="", leaves=None):
    """The six box floats of every swept half (srr / srl u32[n, 8]) against swept_records' (l_lo, l_hi, r_lo, r_hi), as uint32.
    leaves: the sorted leaf boxes (lo, hi) the records were made from -- with them, a zero bound of the other sign passes where the
    child is an internal node whose leaf range holds zeros of both signs in that bound (module docstring); without them, and
    everywhere else, the bits must be equal.  Returns the number of halves compared; raises AssertionError naming the first
    offending halves."""
    n = srr.shape[0]
    m = max(n - 1, 0)
    left, right, first, last = tree_from_records(srr, srl)
    l_lo, l_hi, r_lo, r_hi = want
    assert l_lo.shape[0] == m and r_lo.shape[0] == m, (l_lo.shape, m)
    s_all = np.arange(m, dtype=np.int64)
    offenders = []
    for side, got, w_lo, w_hi, link in ((0, srl, l_lo, l_hi, left), (1, srr, r_lo, r_hi, right)):
        g = got[:m, :6]
        w = np.concatenate([bits(w_lo).reshape(m, 3), bits(w_hi).reshape(m, 3)], axis=1)
        ne = g != w
        zero = ne & ((((g | w) & np.uint32(0x7FFFFFFF)) == 0) & (link >= 0)[:, None])   # +0 against -0 on an internal half
        if leaves is not None and zero.any():
            a, b = (first, s_all) if side == 0 else (s_all + 1, last)
            ne &= ~(zero & _both_zero_signs(leaves, a, b))
        for s in np.nonzero(ne.any(axis=1))[0]:
            offenders.append((int(s), side, g[s].view(np.float32).tolist(), w[s].view(np.float32).tolist()))
    if offenders:
        offenders.sort()
        lines = [f"  {_describe(s, side, first, last, up, n)}\n    got  {g}\n    want {w}" for s, side, g, w in offenders[:8]]
        raise AssertionError(f"{what}: {len(offenders)} of {2 * m} swept record halves differ from the restatement\n" + "\n".join(lines))
    return 2 * m


# ---------------------------------------------------------------- what the walk must find
def query_boxes(lo, hi, p):
    """The descent's query boxes: the leaf's swept fp32 box widened by the pad with directed rounding."""
    return sub_rd32(lo, np.float32(p)), add_ru32(hi, np.float32(p))


def _meets(qlo, qhi, lo, hi):
    return np.all((qlo <= hi) & (lo <= qhi), axis=-1)


def expected_candidates(lo, hi, p, lo_b=None, hi_b=None, brute=None, chunk=1 << 22) -> int:
    """The candidates of one descent.  Self (lo_b None): the ordered pairs (j, k), k > j in sorted order, whose query box of j meets
    leaf k's swept box (closed).  Between: lo / hi are a's leaves, lo_b / hi_b b's; every (i, k); b of one leaf: the device has no
    records to walk and takes every leaf of a against it.  Every pair is tested up to proximity_ref.BRUTE_MAX leaves (BRUTE_MAX^2 / 2
    pairs between two meshes); above that the pairs come from proximity_ref._candidates' grid over the QUERY boxes of all leaves: a
    query box contains its own leaf's box (the pad is >= 0 and the rounding outward), so two leaves whose query box and box meet
    have query boxes that meet, and the grid returns every such pair."""
    between = lo_b is not None
    na = lo.shape[0]
    if between and lo_b.shape[0] == 1:
        return int(na)
    nb = lo_b.shape[0] if between else na
    if na == 0 or nb == 0 or (not between and na < 2):
        return 0
    qlo, qhi = query_boxes(lo, hi, p)
    if brute is None:
        brute = (na * nb <= pr.BRUTE_MAX * pr.BRUTE_MAX // 2) if between else na <= pr.BRUTE_MAX
    tl, th = (lo_b, hi_b) if between else (lo, hi)
    total = 0
    if brute:
        rows = max(1, chunk // nb)
        for r0 in range(0, na, rows):
            r1 = min(na, r0 + rows)
            ok = _meets(qlo[r0:r1, None, :], qhi[r0:r1, None, :], tl[None, :, :], th[None, :, :])
            if not between:
                ok &= np.arange(nb)[None, :] > np.arange(r0, r1)[:, None]
            total += int(ok.sum())
        return total
    if between:
        qlb, qhb = query_boxes(lo_b, hi_b, p)
        allq_lo, allq_hi = np.concatenate([qlo, qlb]), np.concatenate([qhi, qhb])
    else:
        allq_lo, allq_hi = qlo, qhi
    assert np.all(np.isfinite(allq_lo)) and np.all(np.isfinite(allq_hi)), "the grid needs finite query boxes"
    c = pr._candidates(allq_lo.astype(np.float64), allq_hi.astype(np.float64))
    if between:
        c = c[(c[:, 0] < na) & (c[:, 1] >= na)]
        i, k = c[:, 0], c[:, 1] - na
    else:
        i, k = c[:, 0], c[:, 1]                                                # (i < k)
    for c0 in range(0, i.shape[0], chunk):
        ii, kk = i[c0:c0 + chunk], k[c0:c0 + chunk]
        total += int(_meets(qlo[ii], qhi[ii], tl[kk], th[kk]).sum())
    return total


def compare_pad(got_m_bits: int, got_pad, want_m_bits: int, dist: float):
    """M (device data) and the pad cd_debug_swept returns (the host twin of ccd_pad on that M, not device data) against the
    restatement, as bits.  The device's own pad is pinned by the candidate count."""
    assert int(got_m_bits) == int(want_m_bits), ("m_bits", hex(int(got_m_bits)), hex(int(want_m_bits)))
    w = pad(want_m_bits, dist)
    assert bits1(np.float32(got_pad)) == bits1(w), ("pad", float(got_pad), float(w))
    return w


def compare_count(got: int, want: int, what=""):
    """cd_ccd_info.n_candidates against expected_candidates: one right value."""
    assert int(got) == int(want), (f"{what}: candidates", int(got), int(want), int(got) - int(want))
    return int(got)
