"""CPU checks of the restatement test_records_gpu.py pins the device's fp32 records to (records_ref.py) and of its inputs
(records_inputs.py): the roundings against exact rational arithmetic, the theorem the encoding rests on (cd_bvh.h, lines 16-32) by
brute force over all pairs of leaf boxes, the internal boxes as min / max of the leaves', that every mesh holds the classes of leaves
it is there for, and that the comparison raises on each kind of planted error."""
from fractions import Fraction

import numpy as np
import pytest

import records_inputs as ri
import records_ref as rr

F32_MAX = Fraction(rr.FLT_MAX)
DEN32 = float(np.float32(1.4e-45))
_b1 = rr.sr.bits1


def _specials():
    rng = np.random.Generator(np.random.PCG64(41))
    x = [0.0, -0.0, 5e-324, -5e-324, 1e-323, -1e-323, 2.2250738585072014e-308, -2.2250738585072014e-308,          # +-0, double denormals, the smallest normal double
         DEN32, -DEN32, DEN32 * 0.75, -DEN32 * 0.75, DEN32 * 1.5, -DEN32 * 1.5, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38,   # fp32 denormals and around them
         1.1754943508222875e-38, -1.1754943508222875e-38, rr.FLT_MAX, -rr.FLT_MAX, float(np.nextafter(rr.FLT_MAX, np.inf)), float(np.nextafter(-rr.FLT_MAX, -np.inf)),
         1e39, -1e39, 1e300, -1e300, 1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0, 1.0 + 2.0 ** -40, -1.0 - 2.0 ** -40, 1.0 - 2.0 ** -40, -1.0 + 2.0 ** -40]
    x += list((rng.random(300) - 0.5) * 8) + list(np.ldexp(rng.random(200) - 0.5, rng.integers(-160, 140, size=200)))
    x += list(rng.random(60).astype(np.float32).astype(np.float64))                                  # fp32 values: the rounding is the identity
    return np.array(x, dtype=np.float64)


def test_rd32_is_the_largest_float_not_above():
    x = _specials()
    r = rr.rd32(x)
    assert r.dtype == np.float32
    for xi, ri_ in zip(x, r):
        X = Fraction(float(xi))
        if X < -F32_MAX:
            assert np.isneginf(ri_), xi                                        # below -FLT_MAX: -inf
            continue
        assert np.isfinite(ri_), xi
        R = Fraction(float(ri_))
        assert R <= X, (xi, ri_)
        with np.errstate(over="ignore"):
            up = np.nextafter(ri_, np.float32(np.inf))                             # nothing between: the next float lies above x (+inf: x above FLT_MAX gives FLT_MAX)
        assert np.isposinf(up) or Fraction(float(up)) > X, (xi, ri_)
        if X > F32_MAX:
            assert float(ri_) == rr.FLT_MAX
    z = rr.rd32(np.array([0.0, -0.0, 5e-324, -5e-324]))
    assert rr.bits(z).tolist() == [0, 0x80000000, 0, 0x80000001]               # signed zeros kept; 5e-324 -> +0; -5e-324 -> -(smallest denormal)
    assert rr.cell(np.array([0.0, -0.0, 5e-324, -5e-324])).tolist() == [0, 0, 0, 0x80000001]


def test_next_up_is_one_ulp_toward_plus_infinity():
    f = rr.rd32(_specials())
    f = f[np.isfinite(f)]
    u = rr.next_up(f)
    for a, b in zip(f, u):
        if float(a) == rr.FLT_MAX:
            assert np.isposinf(b)
            continue
        A, B = Fraction(float(a)), Fraction(float(b))
        assert B > A, (a, b)
        mid = np.float32((float(a) + float(b)) / 2)                            # (exact in FP64) no float strictly between
        assert mid == a or mid == b, (a, b)
    bits = lambda v: rr.bits(rr.next_up(np.array(v, dtype=np.uint32).view(np.float32))).tolist()
    assert bits([0, 0x80000000]) == [1, 1]                                     # +-0 -> the smallest positive denormal
    assert bits([0x80000001, 0xBF800000]) == [0x80000000, 0xBF7FFFFF]          # a negative value moves toward zero; -denormal -> -0.0
    assert bits([0x7F7FFFFF, 0x007FFFFF]) == [0x7F800000, 0x00800000]          # FLT_MAX -> +inf; the largest denormal -> the smallest normal
    assert rr.bits(rr.prox_hi(np.array([np.inf, 1.0], dtype=np.float32))).tolist() == [0x7F800000, 0x3F800001]


def test_cell_table_counts_distinct_doubles_of_all_vertices():
    b = float(np.float32(1.5))
    v = np.array([[b, b, b], [b, b + 2.0 ** -30, 0.0], [b, b + 2.0 ** -30, -0.0], [2.0, 3.0, 5e-324]])
    t = rr.cell_table(v, "table")
    assert [a.tolist() for a in t.amb] == [[], [_b1(np.float32(b))], [0]]         # the same double twice: one value; -0.0 and +0.0: one value; 5e-324 makes 0's cell ambiguous
    assert rr.detect_mode(v) == "table" and rr.detect_mode(v, False) == "off" and rr.detect_mode(rr.rd32(v).astype(np.float64)) == "none"
    box = np.array([[0.0, b + 2.0 ** -30, 0.0, b, 0.0, 5e-324]])
    e = rr.enc(box, t)
    assert rr.bits(e["hi"]).tolist() == [[_b1(np.float32(b)), _b1(np.float32(b)), 1]]           # x: alone in its cell; y: the base; z: moved
    assert e["moved"].tolist() == [[False, False, True]] and not e["certain"][0] and not e["exact"][0]
    e = rr.enc(box, rr.cell_table(v, "off"))
    assert e["moved"].tolist() == [[True, False, True]]                        # off: every hi that is not an fp32 value
    with pytest.raises(AssertionError):
        rr.cell_table(v, "none")


def _leaf_args(w):
    l64 = w["leaf64"]
    return l64[:, 0::2], l64[:, 1::2], w["leaf"]["lo"], w["leaf"]["hi"], w["leaf"]["certain"]


SMALL = [m for m in ri.MESHES if m in ri.SMALL]                                # (a static table: no mesh is built at collection)


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("mode", ["auto", "off"])
def test_theorem_by_brute_force(name, mode):
    """Over all pairs of leaf boxes and the three axes, with FP64 comparisons as the reference: the fp32 '<' never loses an FP64 '<', and
    decides exactly where the box with the hi is CERTAIN; [lo', prox_hi(hi')] contains the box."""
    v, _ = ri.mesh(name)
    w = ri.want(name, None if mode == "auto" else ("off" if rr.detect_mode(v) != "none" else "none"))
    pairs, with_certain = rr.check_theorem(*_leaf_args(w), what=name)
    assert pairs == 3 * w["n"] ** 2
    # the theorem check has teeth: a moved hi left unmoved loses the pair with a cell mate below it (a leaf's lo in the hi's cell) -- searched over ALL moved
    # bounds, and it must fire on every mesh that is meant to hold one (records_inputs.TEETH), on each axis that has one
    if mode != "auto":
        return
    lo64, hi64, lo32, hi32, c = _leaf_args(w)
    fired = 0
    for a in range(3):
        cells_lo = rr.cell(lo64[:, a])
        for j in np.nonzero(w["leaf"]["moved"][:, a])[0]:
            if ((cells_lo == rr.cell(hi64[j, a])) & (lo64[:, a] < hi64[j, a])).any():
                hi_bad = hi32.copy(); hi_bad[j, a] = rr.rd32(hi64[j, a])
                with pytest.raises(AssertionError, match="a pair would be lost"):
                    rr.check_theorem(lo64, hi64, lo32, hi_bad, c)
                fired += 1
                break
    print(name, "moved bounds with a cell mate found on", fired, "axes")
    assert fired > 0 or name not in ri.TEETH, name
    if name == "bases":
        assert fired == 3


@pytest.mark.parametrize("name", SMALL)
def test_internal_boxes_are_the_min_max_of_the_leaves_encoded_boxes(name):
    """cd_bvh.h, lines 29-30: hi' is monotone in hi, so encoding commutes with max -- every child box of the expected records (the encoded
    FP64 box of the oracle's node) is, bit for bit, the min / max over the encoded boxes of the leaves under it."""
    w = ri.want(name)
    if w["n"] < 2:
        return
    l_lo, l_hi, r_lo, r_hi = rr.leaf_merge_boxes(w["leaf"]["lo"], w["leaf"]["hi"], w["left"], w["right"], w["first"], w["last"])
    m = w["n"] - 1
    assert np.array_equal(rr.bits(l_lo), w["rl"][:m, 0:3]) and np.array_equal(rr.bits(l_hi), w["rl"][:m, 3:6])
    assert np.array_equal(rr.bits(r_lo), w["rr"][:m, 0:3]) and np.array_equal(rr.bits(r_hi), w["rr"][:m, 3:6])


@pytest.mark.parametrize("name", sorted(ri.CLASSES))
def test_inputs_hold_the_classes_they_are_there_for(name):
    w = ri.want(name)
    counts = dict(zip(("exact", "certain", "uncertain"), ri.classes(w)))
    print(name, w["n"], counts, [len(a) for a in w["table"].amb])
    need, never = ri.CLASSES[name]
    for c in need:
        assert counts[c] > 0, (name, c, counts)
    for c in never:
        assert counts[c] == 0, (name, c, counts)
    assert ri.mesh(name)[1].shape[0] <= 40000


def test_inputs_do_their_job():
    """What the constructed meshes claim in their docstrings, read off the restatement."""
    # bases: the hi of triangle 3k IS the base of an ambiguous cell and stays; triangle 3k + 1's hi is the cell's other double and moves; triangle 3k + 2's lo is the base
    w = ri.want("bases")
    perm = ri.step("bases")["perm"].astype(np.int64)
    hi64, moved = w["leaf64"][:, 1::2], w["leaf"]["moved"]
    at_base, other, lo_base = perm % 3 == 0, perm % 3 == 1, perm % 3 == 2
    for a in range(3):
        assert w["table"].ambiguous(a, hi64[~lo_base, a]).all()
    assert not moved[at_base].any() and rr.is_f32(hi64[at_base]).all() and moved[other].all() and not moved[lo_base].any()
    assert (hi64[other] < 0).any() and (hi64[other] > 0).any()                  # both directions of the step
    lo64 = w["leaf64"][:, 0::2]
    assert np.array_equal(np.sort(rr.cell(lo64[lo_base]), axis=0), np.sort(rr.cell(hi64[other]), axis=0)) and rr.is_f32(lo64[lo_base]).all()   # the moved his' cell mates
    # zeros
    w = ri.want("zeros")
    assert [a.tolist() for a in w["table"].amb] == [[0, 0x80000001]] * 3        # 0's cell through 5e-324 alone; -1.4e-45's through -5e-324 and -1e-323
    qb, l64 = w["qb"], w["leaf64"]
    hi_bits = {(float(h), int(b)) for h, b in zip(l64[:, 1], qb[:, 3])}
    assert (5e-324, 1) in hi_bits and (-5e-324, 0x80000000) in hi_bits and (-1e-323, 0x80000000) in hi_bits      # moved: 0 -> denormal, -denormal -> -0.0
    z = l64[:, 1] == 0.0
    assert set(qb[z, 3].tolist()) == {0, 0x80000000}                           # an hi that is a zero is a base: kept, with its sign
    assert {int(b) for l, b in zip(l64[:, 0], qb[:, 0]) if l == -5e-324} == {0x80000001}
    flat = (l64[:, 4] == 0.0) & (l64[:, 5] == 0.0)
    assert flat.sum() >= 2 and not (qb[flat, 6] & rr.LB_SELF).any() and {int(x) for x in qb[flat, 2]} == {0, 0x80000000}   # the flat triangles in z = -0.0 and z = +0.0
    thin = np.all(l64[:, 0::2] < l64[:, 1::2], axis=1) & ((qb[:, 6] & rr.LB_SELF) == 0)
    assert thin.sum() == 1 and np.abs(l64[thin]).max() <= 5e-324               # lo < hi, yet no overlap with itself: the reference's product underflows
    # negatives: wholly below zero; a moved hi steps toward zero
    w = ri.want("negatives")
    assert (ri.mesh("negatives")[0] < 0).all()
    mv = w["leaf"]["moved"]
    assert mv.any() and (np.abs(w["leaf"]["hi"][mv]) < np.abs(rr.rd32(w["leaf64"][:, 1::2])[mv])).all()
    # beyond_fp32: -inf for a lo below -FLT_MAX; FLT_MAX for an hi alone above it (y), +inf where two doubles share that cell (x)
    w = ri.want("beyond_fp32")
    l64, qb = w["leaf64"], w["qb"]
    assert {int(b) for l, b in zip(l64[:, 0], qb[:, 0]) if l < -rr.FLT_MAX} == {0xFF800000} and (l64[:, 0] < -rr.FLT_MAX).sum() >= 2
    assert {int(b) for h, b in zip(l64[:, 1], qb[:, 3]) if h > rr.FLT_MAX} == {0x7F800000} and (l64[:, 1] > rr.FLT_MAX).sum() >= 2
    assert {int(b) for h, b in zip(l64[:, 3], qb[:, 4]) if h > rr.FLT_MAX} == {0x7F7FFFFF} and (l64[:, 3] > rr.FLT_MAX).sum() >= 2
    assert (w["rr"][: w["n"] - 1, 3] == 0x7F800000).any()                      # ... and in the records of internal nodes
    # duplicates: no ambiguity from equal values
    assert all(len(a) == 0 for a in ri.want("duplicates")["table"].amb)
    # few_cells: x takes eight doubles in four ambiguous cells; many_cells: the table at its working load
    v, _ = ri.mesh("few_cells")
    assert np.unique(v[:, 0]).size == 8 and len(ri.want("few_cells")["table"].amb[0]) == 4
    v, _ = ri.mesh("many_cells")
    assert all(np.unique(v[:, a]).size > 119000 for a in range(3)) and all(len(a) > 50 for a in ri.want("many_cells")["table"].amb)
    # off differs from the table on a mesh with doubles
    assert not np.array_equal(ri.want("cloth_double", "off")["qb"], ri.want("cloth_double")["qb"])


def _got(w):
    return [w["rr"].copy(), w["rl"].copy(), w["qb"].copy(), w["root"], w["root_box"].copy()]


def _leaf_child(w, pred):
    """(split, side, leaf) of the first leaf child whose leaf satisfies pred(j)."""
    for s in range(w["n"] - 1):
        for side, link in ((0, int(w["left"][s])), (1, int(w["right"][s]))):
            if link < 0 and pred(~link):
                return s, side, ~link
    raise AssertionError("no such leaf child")


def test_comparison_reports_planted_errors():
    w = ri.want("bases")
    n = w["n"]
    assert rr.same_records(_got(w), w, n) > 0
    moved, hi64 = w["leaf"]["moved"], w["leaf64"][:, 1::2]

    def plant(fn, match):
        g = _got(w)
        fn(g)
        with pytest.raises(AssertionError, match=match):
            rr.same_records(g, w, n)

    # one hi left unmoved: in a record half, and in a query box
    s, side, j = _leaf_child(w, lambda j: moved[j, 0])
    def unmoved(g): g[1 - side][s, 3] = _b1(rr.rd32(hi64[j, 0]))
    plant(unmoved, rf"{'left' if side == 0 else 'right'} halves: split {s} word 3 \(hi.x\).*ambiguous")
    def unmoved_q(g): g[2][j, 3] = _b1(rr.rd32(hi64[j, 0]))
    plant(unmoved_q, rf"query boxes: leaf {j} word 3")
    # one hi moved that should not be (it is the cell's base)
    s2, side2, j2 = _leaf_child(w, lambda j: not moved[j].any())
    def overmoved(g): g[1 - side2][s2, 4] = _b1(rr.next_up(rr.rd32(hi64[j2, 1])))
    plant(overmoved, rf"split {s2} word 4 \(hi.y\).*is an fp32 value")
    # one lo rounded up
    def lo_up(g): g[1][0, 2] = rr.bits(rr.next_up(g[1][0:1, 2].view(np.float32)))[0]
    plant(lo_up, r"left halves: split 0 word 2 \(lo.z\)")
    # a flipped CERTAIN / EXACT bit on a leaf child; a flipped flag of a query box
    def certain(g): g[0][s, 7] ^= np.uint32(1 << (30 + side))
    plant(certain, rf"right halves: split {s} word 7 bit {30 + side} \(CERTAIN")
    def exact(g): g[1][s2, 7] ^= np.uint32(1 << (30 + side2))
    plant(exact, rf"left halves: split {s2} word 7 bit {30 + side2} \(EXACT")
    def qflag(g): g[2][j, 6] ^= np.uint32(rr.LB_CERTAIN)
    plant(qflag, rf"query boxes: leaf {j} word 6")
    # a link, a range word, the root's name, the root box
    def link(g): g[0][1, 6] ^= np.uint32(1)
    plant(link, r"right halves: split 1 word 6")
    def rng_(g): g[1][1, 7] ^= np.uint32(1)
    plant(rng_, r"left halves: split 1 word 7 \(range\)")
    def root(g): g[3] = (w["root"] + 1) % (n - 1)
    plant(root, r"root: got split")
    def rbox(g): g[4][3] = np.nextafter(g[4][3], np.inf)
    plant(rbox, r"root box: word 3")
    # NOT errors: the flag bits of an internal child, the slot that names no split
    si = next(s for s in range(n - 1) if w["left"][s] >= 0)
    g = _got(w)
    g[0][si, 7] ^= np.uint32(1 << 30); g[1][si, 7] ^= np.uint32(1 << 30)
    g[0][n - 1] = 0xDEADBEEF; g[1][n - 1] = 0xDEADBEEF
    rr.same_records(g, w, n)


def test_comparison_expects_each_builds_sign_of_a_zero():
    """Where the leaves under an internal child hold zeros of both signs in one bound, the stage-wise build keeps the rightmost's sign and the fused build
    has -0 for a lo, +0 for an hi: same_records expects the bits of the build it is told, and nothing else -- not the other build's, not on a leaf child."""
    w = ri.want("zeros")
    n = w["n"]
    mm = rr.for_minmax(w)
    diff = np.argwhere(mm["rl"] != w["rl"]).tolist() + np.argwhere(mm["rr"] != w["rr"]).tolist()
    assert len(diff) > 0 and all(k < 6 for _, k in diff)                       # the mesh holds such words, and the two builds differ in them
    rr.same_records(_got(w), w, n)
    rr.same_records(_got(mm), w, n, zeros="minmax")
    with pytest.raises(AssertionError, match="halves: split"):
        rr.same_records(_got(mm), w, n)
    with pytest.raises(AssertionError, match="halves: split"):
        rr.same_records(_got(w), w, n, zeros="minmax")
    s, side, j = _leaf_child(w, lambda j: w["qb"][j, 2] & 0x7FFFFFFF == 0)
    for zeros in ("rightmost", "minmax"):
        g = _got(mm if zeros == "minmax" else w); g[1 - side][s, 2] ^= np.uint32(0x80000000)
        with pytest.raises(AssertionError, match="word 2"):
            rr.same_records(g, w, n, zeros=zeros)
    g = _got(w); g[4][0] = -0.0 if g[4][0] != 0 else g[4][0]
    with pytest.raises(AssertionError, match="root box"):
        rr.same_records(g, w, n)


def test_one_triangle_has_query_box_and_root_box_only():
    w = ri.want("soup1")
    assert w["root"] is None and w["rr"].shape == (1, 8)
    g = [np.full((1, 8), 7, np.uint32), np.full((1, 8), 9, np.uint32), w["qb"].copy(), 12345, w["root_box"].copy()]
    rr.same_records(g, w, 1)
    g[2][0, 0] ^= np.uint32(1)
    with pytest.raises(AssertionError, match="query boxes: leaf 0 word 0"):
        rr.same_records(g, w, 1)
