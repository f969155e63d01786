"""The CPU restatement of the box queries (tests/box_ref.py) against exact arithmetic, and the inputs the GPU test relies on.

box_ref.box_tri_np restates box_tri with its operation order; here it is checked against the SAME separating-axis test evaluated
exactly, in integers, on the true box: every input coordinate is a multiple of a power of two, so the inputs times that power are
Python integers and every sum and product of them is exact (the box centre and half-widths are kept doubled: 2 c = lo + hi,
2 h = hi - lo).  No test in here needs a device."""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import box_ref as br
import scale_inputs as si

N = br.N
REL_MIN = 2.0 ** -40
LEFT_OUT_MAX = N // 1000                                                        # 0.1 % of a family


# ---------------------------------------------------------------- the exact evaluation
def _shift(*arrays):
    """The smallest s >= 0 for which every double of the arrays times 2^s is an integer."""
    s = 0
    for x in arrays:
        x = np.asarray(x, dtype=np.float64).ravel()
        m, e = np.frexp(x[x != 0.0])
        mi = np.ldexp(m, 53).astype(np.int64)
        tz = np.log2((mi & -mi).astype(np.float64)).astype(np.int64)
        s = max(s, int(-(e - 53 + tz).min(initial=0)))
    return s


def _ints(x, shift):
    """The doubles x times 2^shift as Python integers (asserted exact)."""
    y = np.ldexp(np.asarray(x, dtype=np.float64), shift)
    assert np.array_equal(y, np.rint(y)) and np.abs(y).max(initial=0.0) < 2.0 ** 200
    return [int(Fraction(float(t))) for t in y.ravel()]


def exact_box_tri(box, tri, vertex_rule=True):
    """box: 6 integers {x1, x2, y1, y2, z1, z2}; tri: 9 integers.  -> (hit, inside, code, rel): box_tri's steps in its order with
    exact arithmetic, and the smallest relative margin of the arithmetic axes it evaluated: the distance of min(q) - r and max(q) + r
    (or d - r and d + r) from 0, over the axis' 1-norm and the largest |coordinate| (inf when no such axis was evaluated; an axis
    whose 1-norm is 0 -- a zero edge, a zero normal -- is 0 > 0 in any arithmetic and has no margin)."""
    lo, hi = box[0::2], box[1::2]
    P = (tri[0:3], tri[3:6], tri[6:9])
    for a in range(3):
        if max(p[a] for p in P) < lo[a] or min(p[a] for p in P) > hi[a]:
            return False, False, 1 + a, math.inf
    if all(lo[a] <= p[a] <= hi[a] for p in P for a in range(3)):
        return True, True, 0, math.inf
    if vertex_rule and any(all(lo[a] <= p[a] <= hi[a] for a in range(3)) for p in P):      # (rule 2b; test_vertex_rule_... below: the axes agree)
        return True, False, 0, math.inf
    big = max(max(abs(t) for t in tri), max(abs(t) for t in box))
    C2 = [lo[a] + hi[a] for a in range(3)]
    H2 = [hi[a] - lo[a] for a in range(3)]
    V = [[2 * p[a] - C2[a] for a in range(3)] for p in P]                       # 2 v_i
    F = [[P[1][a] - P[0][a] for a in range(3)], [P[2][a] - P[1][a] for a in range(3)], [P[0][a] - P[2][a] for a in range(3)]]
    rel = math.inf

    def margin(lo_q, hi_q, r, norm1):                                           # (all doubled)
        nonlocal rel
        if norm1:
            rel = min(rel, min(abs(lo_q - r), abs(hi_q + r)) / (2 * norm1 * big))

    for k in range(3):
        for j in range(3):
            a, b = (j + 1) % 3, (j + 2) % 3
            q = [V[i][b] * F[k][a] - V[i][a] * F[k][b] for i in range(3)]
            r = H2[a] * abs(F[k][b]) + H2[b] * abs(F[k][a])
            margin(min(q), max(q), r, abs(F[k][a]) + abs(F[k][b]))
            if min(q) > r or max(q) < -r:
                return False, False, 4 + 3 * k + j, rel
    n = [F[0][1] * F[1][2] - F[0][2] * F[1][1], F[0][2] * F[1][0] - F[0][0] * F[1][2], F[0][0] * F[1][1] - F[0][1] * F[1][0]]
    d = n[0] * V[0][0] + n[1] * V[0][1] + n[2] * V[0][2]
    r = H2[0] * abs(n[0]) + H2[1] * abs(n[1]) + H2[2] * abs(n[2])
    margin(d, d, r, abs(n[0]) + abs(n[1]) + abs(n[2]))
    if d > r or d < -r:
        return False, False, 13, rel
    return True, False, 0, rel


def _exact_family(boxes, tris):
    shift = _shift(boxes, tris)
    b, t = _ints(boxes, shift), _ints(tris, shift)
    return [exact_box_tri(b[6 * i:6 * i + 6], t[9 * i:9 * i + 9]) for i in range(boxes.shape[0])]


def _agreement(boxes, tris, what):
    hit, inside, code = br.box_tri_np(boxes, tris)
    exact = _exact_family(boxes, tris)
    left_out = disagree = 0
    for i, (h, ins, c, rel) in enumerate(exact):
        if rel < REL_MIN:
            left_out += 1
        elif (bool(hit[i]), bool(inside[i]), int(code[i])) != (h, ins, c):
            disagree += 1
    hits = sum(1 for e in exact if e[0])
    smallest = min(e[3] for e in exact)
    print(f"{what}: {len(exact)} cases, {hits} hits, {left_out} left out, {disagree} disagreements, smallest relative margin {smallest:.3g}")
    return hits, left_out, disagree, exact


def test_integer_family_agrees_with_exact_arithmetic_in_every_case():
    boxes, tris = br.integer_family()
    hits, left_out, disagree, exact = _agreement(boxes, tris, "integer family")
    hit, inside, code = br.box_tri_np(boxes, tris)
    assert all((bool(hit[i]), bool(inside[i]), int(code[i])) == e[:3] for i, e in enumerate(exact))        # margins of 0 included
    assert N // 10 <= hits <= N - N // 10
    # touching configurations occur: a vertex on the box's boundary, and a triangle in the plane of a box face
    lo, hi = boxes[:, None, 0::2], boxes[:, None, 1::2]
    on_boundary = (((tris == lo) | (tris == hi)) & (tris >= lo).all(axis=2, keepdims=True) & (tris <= hi).all(axis=2, keepdims=True)).any(axis=(1, 2))
    in_face = ((tris == lo).all(axis=1) | (tris == hi).all(axis=1)).any(axis=1)
    assert (on_boundary & hit).sum() > 100 and (in_face & hit).sum() > 10 and any(e[3] == 0 for e in exact)


@pytest.mark.parametrize("offset", [0.0, br.OFFSET])
def test_random_families_agree_with_exact_arithmetic_beyond_the_margin(offset):
    boxes, tris = br.random_family(offset)
    hits, left_out, disagree, _ = _agreement(boxes, tris, f"random family, offset {offset}")
    assert N // 10 <= hits <= N - N // 10, hits
    assert left_out <= LEFT_OUT_MAX and disagree == 0, (left_out, disagree)


def test_vertex_rule_changes_no_exact_answer():
    """Rule 2b (a vertex in the closed box is a hit) is what the thirteen axes say in exact arithmetic: none separates such a triangle."""
    for boxes, tris in (br.integer_family(), br.random_family(0.0)):
        shift = _shift(boxes, tris)
        b, t = _ints(boxes, shift), _ints(tris, shift)
        used = 0
        for i in range(boxes.shape[0]):
            with_rule, without = exact_box_tri(b[6 * i:6 * i + 6], t[9 * i:9 * i + 9]), exact_box_tri(b[6 * i:6 * i + 6], t[9 * i:9 * i + 9], vertex_rule=False)
            assert with_rule[:3] == without[:3], i
            used += with_rule[3] != without[3]
        assert used > 100                                                       # the rule did decide cases


# ---------------------------------------------------------------- structure
def test_every_code_and_both_hit_kinds_occur():
    seen, kinds = set(), set()
    for boxes, tris in (br.integer_family(), br.random_family(0.0), br.random_family(br.OFFSET)):
        hit, inside, code = br.box_tri_np(boxes, tris)
        seen |= set(np.unique(code).tolist())
        kinds |= {(bool(h), bool(i)) for h, i in zip(hit[:2000], inside[:2000])}
        assert not (inside & ~hit).any() and ((code == 0) == hit).all()
    assert seen == set(range(14)) and {(True, True), (True, False), (False, False)} <= kinds, (seen, kinds)


def _segment_meets_box(lo, hi, a, b):
    """Exact: does the segment a b meet the closed box?  (Clipping the parameter range axis by axis, in fractions.)"""
    t0, t1 = Fraction(0), Fraction(1)
    for k in range(3):
        d = b[k] - a[k]
        if d == 0:
            if a[k] < lo[k] or a[k] > hi[k]:
                return False
            continue
        u, v = Fraction(lo[k] - a[k], d), Fraction(hi[k] - a[k], d)
        if u > v:
            u, v = v, u
        t0, t1 = max(t0, u), min(t1, v)
        if t0 > t1:
            return False
    return True


def test_degenerate_triangles_are_points_and_segments():
    n = 5000
    boxes, tris = br.integer_family()
    boxes, tris = boxes[:n], tris[:n].copy()
    lo, hi = boxes[:, 0::2], boxes[:, 1::2]
    pts = tris.copy(); pts[:, 1] = pts[:, 0]; pts[:, 2] = pts[:, 0]              # a point
    hit, inside, _ = br.box_tri_np(boxes, pts)
    want = ((lo <= pts[:, 0]) & (pts[:, 0] <= hi)).all(axis=1)
    assert np.array_equal(hit, want) and np.array_equal(inside, want) and 50 < want.sum() < n - 50
    for dup in ((0, 1, 1), (0, 1, 0), (0, 0, 1)):                               # a segment, the repeated vertex in every place
        seg = tris[:, list(dup)]
        hit, inside, _ = br.box_tri_np(boxes, seg)
        want = np.array([_segment_meets_box(lo[i].astype(int).tolist(), hi[i].astype(int).tolist(), tris[i, 0].astype(int).tolist(),
                                            tris[i, 1].astype(int).tolist()) for i in range(n)])
        assert np.array_equal(hit, want), dup
        assert 100 < want.sum() < n - 100 and (hit & ~inside).any()


BAND = tuple(k for k in si.SCALES if abs(k) <= 300) + (-300, 300)               # ray_tri's band, which box_tri's statement takes


def test_invariant_under_power_of_two_scaling_over_the_band():
    for boxes, tris in (br.integer_family(), br.random_family(0.0)):
        want = br.box_tri_np(boxes, tris)
        for k in BAND:
            got = br.box_tri_np(si.scaled(boxes, k), si.scaled(tris, k))
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), k


# ---------------------------------------------------------------- the two calls' restatements, and the GPU test's inputs
@pytest.mark.parametrize("name", ["n1", "n2", "n3", "n65", "duplicates", "comb", "custom_ids"])
def test_counts_of_the_rows_are_the_count_restatement(name):
    v, i, ids, edge = br.MESHES[name]
    n = 1000 if i.shape[0] <= 1000 else 200
    w = br.take_items(br.want_rows(name), n)
    count, n_inside = br.boxes_count_ref(v, i, br.boxes(name)[:n])
    c, ci = br.counts_of(w, n)
    assert np.array_equal(c, count) and np.array_equal(ci, n_inside)
    assert np.unique(w.rows, axis=0).shape[0] == w.rows.shape[0]


@pytest.mark.parametrize("name", br.NAMES)
def test_input_conditions_of_the_gpu_test(name):
    br.input_conditions(name)
    b = br.boxes(name)
    assert (b[:, 0::2] <= b[:, 1::2]).all() and np.isfinite(b).all()
    assert (b[3::8, 0::2] == b[3::8, 1::2]).all() and (b[4::8, 2] == b[4::8, 3]).all()       # the point boxes and the slabs
