"""CPU restatement of the static tree's fp32 records and query boxes (csrc/cd_bvh.h, lines 16-40: the cell table and the encoding;
include/mi355cd.h: cd_debug_records, cd_root_box), exact: numpy, FP64 and fp32 with directed rounding.  Written from that text, not
from the kernels: the table here is a sort, not a hash table, and a leaf's bounds are looked up like any other box's.

  cell(x)  = rd32(x), -0.0 folded onto +0.0.  A cell of an axis is AMBIGUOUS iff two distinct doubles among ALL the mesh's vertex
             coordinates of that axis lie in it (-0.0 and +0.0 are one value).
  lo'      = rd32(lo)
  hi'      = rd32(hi), one ulp up (next_up) iff hi is not an fp32 value and cell(hi) is ambiguous
  CERTAIN  = no hi of the box was moved;  EXACT = CERTAIN and the six bounds are fp32 values.

Everything is compared as bits, with no freedom.  One word has two right values, by build: where the leaf range of an INTERNAL child
holds zeros of both signs in one bound, the stage-wise build keeps the sign of the rightmost (box.cuh:24-32's compare-selects on the
FP64 boxes: what the oracle's boxes hold) and the fused build -0 for a lo and +0 for a hi (v_min_f32 / v_max_f32 on the leaves' fp32
boxes, cd_build.h).  same_records is told which build it looks at (zeros = "rightmost" / "minmax") and expects that build's bits.
"""
from __future__ import annotations

import numpy as np

import swept_ref as sr

FLT_MAX = float(np.finfo(np.float32).max)
REC_MASK = sr.REC_MASK
REC_L, REC_R = np.uint32(0x40000000), np.uint32(0x80000000)      # cd_bvh.h REC_L_* / REC_R_*: EXACT in `first`, CERTAIN in `last`
LB_EXACT, LB_SELF, LB_CERTAIN = 1, 2, 4                          # cd_bvh.h LeafBox32::flags
MODES = ("table", "none", "off")

rd32 = sr.rd32                                                   # np.float32 + np.nextafter; test_records_ref.py checks it against Fraction
bits = sr.bits


def next_up(f) -> np.ndarray:
    """cd_bvh.h f32_next_up on fp32 values: +-0 -> the smallest positive denormal; a negative value one step toward zero
    (-denorm_min -> -0.0); FLT_MAX -> +inf.  Never applied to +inf or a NaN by the encoding."""
    u = bits(np.asarray(f, dtype=np.float32)).astype(np.uint32)
    zero = (u << np.uint32(1)) == 0
    neg = (u >> np.uint32(31)) != 0
    r = np.where(zero, np.uint32(1), np.where(neg, u - np.uint32(1), u + np.uint32(1))).astype(np.uint32)
    return r.view(np.float32)


def prox_hi(h) -> np.ndarray:
    """cd_proximity.h: a stored hi read as an upper bound by the other queries -- next_up(hi), +inf stays +inf."""
    h = np.asarray(h, dtype=np.float32)
    return np.where(bits(h) == np.uint32(0x7F800000), h, next_up(h)).astype(np.float32)


def is_f32(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    return rd32(x).astype(np.float64) == x


def cell(x) -> np.ndarray:
    """The cell of a double as the bits of its base: rd32(x), -0.0 folded onto +0.0."""
    c = bits(rd32(x)).astype(np.uint32)
    return np.where(c == np.uint32(0x80000000), np.uint32(0), c)


class CellTable:
    """mode 'table': amb[axis] = the sorted cells of that axis that hold two distinct doubles; 'none' / 'off': no table."""

    def __init__(self, mode, amb):
        self.mode, self.amb = mode, amb

    def ambiguous(self, axis: int, x) -> np.ndarray:
        x = np.asarray(x, dtype=np.float64)
        if self.mode == "none":
            return np.zeros(x.shape, dtype=bool)
        if self.mode == "off":
            return ~is_f32(x)
        return np.isin(cell(x), self.amb[axis])

    def state(self, axis: int, x) -> str:
        x = np.array([x], dtype=np.float64).reshape(1)
        return (f"cell 0x{int(cell(x)[0]):08x} (base {float(rd32(x)[0])!r}), {'ambiguous' if self.ambiguous(axis, x)[0] else 'not ambiguous'}, "
                f"bound {'is' if is_f32(x)[0] else 'is not'} an fp32 value, mode {self.mode}")


def detect_mode(verts, cell_table_opt: bool = True) -> str:
    """What amb_refresh decides on upload: no table when every coordinate is an fp32 value, else the table, unless CD_OPT_CELL_TABLE is 0."""
    if bool(np.all(is_f32(verts))):
        return "none"
    return "table" if cell_table_opt else "off"


def cell_table(verts, mode: str | None = None) -> CellTable:
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    if mode is None:
        mode = detect_mode(verts)
    assert mode in MODES, mode
    if mode == "none":
        assert bool(np.all(is_f32(verts))), "mode 'none' is for a mesh whose coordinates are all fp32 values"
    amb = []
    for a in range(3):
        vals = np.unique(verts[:, a] + 0.0)                                   # distinct doubles; x + 0.0 folds -0.0 onto +0.0
        c, count = np.unique(cell(vals), return_counts=True)
        amb.append(c[count >= 2].astype(np.uint32))
    return CellTable(mode, amb)


def enc(box64, table: CellTable):
    """box64 f64[m, 6] as {x1, x2, y1, y2, z1, z2} -> dict(lo f32[m, 3], hi f32[m, 3], moved bool[m, 3], certain bool[m], exact bool[m])."""
    b = np.asarray(box64, dtype=np.float64).reshape(-1, 6)
    lo64, hi64 = b[:, 0::2], b[:, 1::2]
    lo, hi = rd32(lo64).reshape(-1, 3), rd32(hi64).reshape(-1, 3)
    moved = np.zeros(hi.shape, dtype=bool)
    for a in range(3):
        moved[:, a] = ~is_f32(hi64[:, a]) & table.ambiguous(a, hi64[:, a])
    hi = np.where(moved, next_up(hi), hi).astype(np.float32)
    certain = ~moved.any(axis=1)
    exact = certain & np.all(is_f32(b), axis=1)
    return dict(lo=lo, hi=hi, moved=moved, certain=certain, exact=exact)


def _half(e, link, word7):
    m = link.shape[0]
    h = np.zeros((m + 1, 8), dtype=np.uint32)                                  # slot n - 1 names no split
    h[:m, 0:3], h[:m, 3:6], h[:m, 6], h[:m, 7] = bits(e["lo"]), bits(e["hi"]), link.view(np.uint32), word7
    return h


def expected_records(verts, vidx, step, mode: str | None = None):
    """What cd_debug_records and cd_root_box give on a correct device for the oracle's tree `step` (oracle.pipeline): rr / rl (right and
    left halves u32[n, 8] by split), qb (query boxes u32[n, 8]), root (the root's split; None for n == 1), root_box f64[6]; and for the
    failure reports the FP64 boxes they came from (l64 / r64 by split, leaf64), the tree by split and the table."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(vidx).reshape(-1, 3).shape[0]
    table = cell_table(verts, mode)
    boxes = np.asarray(step["boxes"], dtype=np.float64).reshape(-1, 6)
    leaf64 = boxes[n - 1:]
    el = enc(leaf64, table)
    # SELF: box.cuh:40-43 with a == b, in the reference's product form -- (lo - hi) * (lo - hi) > 0 per axis.  That is lo < hi, except that a box
    # thinner than about 1e-162 along an axis does not overlap itself: the product underflows to 0 (records_inputs' box inside the denormals)
    with np.errstate(over="ignore"):
        ext = leaf64[:, 0::2] - leaf64[:, 1::2]
        self_ = np.all(ext * ext > 0, axis=1)
    qb = np.zeros((n, 8), dtype=np.uint32)
    qb[:, 0:3], qb[:, 3:6] = bits(el["lo"]), bits(el["hi"])
    qb[:, 6] = (np.where(el["exact"], LB_EXACT, 0) | np.where(self_, LB_SELF, 0) | np.where(el["certain"], LB_CERTAIN, 0)).astype(np.uint32)
    out = dict(n=n, table=table, leaf64=leaf64, leaf=el, qb=qb, root_box=boxes[0].copy())
    if n < 2:
        none = np.zeros((n, 8), dtype=np.uint32)
        return dict(out, rr=none, rl=none.copy(), root=None, l64=np.zeros((0, 6)), r64=np.zeros((0, 6)),
                    left=np.zeros(0, np.int32), right=np.zeros(0, np.int32), first=np.zeros(0, np.int64), last=np.zeros(0, np.int64))
    (L, R, F, La), split_of = sr.tree_from_karras(step["left"], step["right"], step["range_first"], step["range_last"])
    sr.check_tree(L, R, F, La)
    m = n - 1
    l64, r64 = np.zeros((m, 6)), np.zeros((m, 6))
    l64[split_of], r64[split_of] = boxes[np.asarray(step["left"], dtype=np.int64)], boxes[np.asarray(step["right"], dtype=np.int64)]
    e_l, e_r = enc(l64, table), enc(r64, table)
    w_first = F.astype(np.uint32) | np.where(e_l["exact"], REC_L, np.uint32(0)) | np.where(e_r["exact"], REC_R, np.uint32(0))
    w_last = La.astype(np.uint32) | np.where(e_l["certain"], REC_L, np.uint32(0)) | np.where(e_r["certain"], REC_R, np.uint32(0))
    return dict(out, rl=_half(e_l, L, w_first), rr=_half(e_r, R, w_last), root=int(split_of[0]), l64=l64, r64=r64, left=L, right=R, first=F, last=La)


# ---------------------------------------------------------------- comparison
_WORDS = ("lo.x", "lo.y", "lo.z", "hi.x", "hi.y", "hi.z")


def _f(u) -> str:
    u = np.uint32(u)
    return f"{float(np.array([u], dtype=np.uint32).view(np.float32)[0])!r} (0x{int(u):08x})"


def _source(want, box64, w):
    """The FP64 bound word w (0..5) of a box came from, and its cell's state."""
    axis = w % 3
    bound = float(box64[2 * axis + (1 if w >= 3 else 0)])
    return f"from FP64 {'hi' if w >= 3 else 'lo'} {bound!r} ({bound.hex()}): {want['table'].state(axis, bound)}"


def _zero_freedom(want, first, last):
    """bool[q, 6]: the sorted leaf range [first[q], last[q]] holds a -0 and a +0 in that bound of the leaves' fp32 boxes."""
    return sr._both_zero_signs((want["leaf"]["lo"], want["leaf"]["hi"]), np.asarray(first, dtype=np.int64), np.asarray(last, dtype=np.int64))


def for_minmax(want):
    """The expectation for a build that merges the leaves' fp32 boxes with v_min_f32 / v_max_f32: the same words, but a zero bound of an
    internal child whose leaf range holds zeros of both signs is -0 as a lo and +0 as an hi."""
    n = want["n"]
    if n < 2:
        return want
    m, s = n - 1, np.arange(n - 1, dtype=np.int64)
    out = dict(want, rl=want["rl"].copy(), rr=want["rr"].copy())
    sign = np.array([0x80000000] * 3 + [0] * 3, dtype=np.uint32)
    for h, link, a, b in ((out["rl"], want["left"], want["first"], s), (out["rr"], want["right"], s + 1, want["last"])):
        both = _zero_freedom(want, a, b) & ((h[:m, :6] & np.uint32(0x7FFFFFFF)) == 0) & (link >= 0)[:, None]
        h[:m, :6] = np.where(both, sign[None, :], h[:m, :6])
    return out


def same_records(got, want, n, zeros="rightmost"):
    """got: cd.debug_records() + (cd.root_box(),) = (right halves, left halves, query boxes, root split, FP64 root box); want:
    expected_records'.  Raises AssertionError naming the array, the split or leaf, the word, the FP64 bound it came from and its cell's
    state.  Records are named by split: slots 0 .. n - 2 are compared, slot n - 1 holds whatever the allocation held; bits 30 / 31
    of word 7 only where the left / right child is a LEAF (no kernel reads those of internal children).  Everything else bit for bit.
    zeros: "rightmost" for a tree of the stage-wise build, "minmax" for one of the fused build (module docstring).  Returns the number
    of words compared."""
    assert zeros in ("rightmost", "minmax"), zeros
    if zeros == "minmax":
        want = for_minmax(want)
    rr, rl, qb, root, rbox = got
    assert n == want["n"] and qb.shape == (n, 8) and rr.shape == (n, 8) and rl.shape == (n, 8), (n, want["n"], qb.shape, rr.shape, rl.shape)
    errs, compared = [], 0
    # the query boxes: all eight words
    ne = qb != want["qb"]
    compared += qb.size
    for j, w in zip(*np.nonzero(ne)):
        what = _source(want, want["leaf64"][j], w) if w < 6 else ("flags: bit 0 EXACT, bit 1 SELF, bit 2 CERTAIN" if w == 6 else "pad word")
        errs.append(f"query boxes: leaf {j} word {w} ({_WORDS[w] if w < 6 else 'flags' if w == 6 else 'pad'}): got {_f(qb[j, w]) if w < 6 else hex(int(qb[j, w]))}, "
                    f"want {_f(want['qb'][j, w]) if w < 6 else hex(int(want['qb'][j, w]))}; {what}")
    # the FP64 root box
    rb, wb = np.ascontiguousarray(rbox, dtype=np.float64).view(np.uint64), np.ascontiguousarray(want["root_box"], dtype=np.float64).view(np.uint64)
    for k in range(6):
        compared += 1
        if rb[k] != wb[k]:
            errs.append(f"root box: word {k}: got {float(rbox[k])!r}, want {float(want['root_box'][k])!r}")
    if n >= 2:
        if root != want["root"]:
            errs.append(f"root: got split {root}, want {want['root']}")
        L, R, F, La = want["left"], want["right"], want["first"], want["last"]
        m = n - 1
        s = np.arange(m, dtype=np.int64)
        for name, g, w, link, src, a, b, flagbit in (("left halves", rl, want["rl"], L, want["l64"], F, s, "EXACT"), ("right halves", rr, want["rr"], R, want["r64"], s + 1, La, "CERTAIN")):
            g, w = g[:m], w[:m]
            ne = g[:, :6] != w[:, :6]
            compared += 8 * m
            for sp, k in zip(*np.nonzero(ne)):
                errs.append(f"{name}: split {sp} word {k} ({_WORDS[k]}), child {'leaf ' + str(~int(link[sp])) if link[sp] < 0 else 'node ' + str(int(link[sp]))}: "
                            f"got {_f(g[sp, k])}, want {_f(w[sp, k])}; {_source(want, src[sp], k)}")
            for sp in np.nonzero(g[:, 6] != w[:, 6])[0]:
                errs.append(f"{name}: split {sp} word 6 (link): got {int(g[sp, 6].view(np.int32))}, want {int(w[sp, 6].view(np.int32))}")
            for sp in np.nonzero((g[:, 7] & np.uint32(REC_MASK)) != (w[:, 7] & np.uint32(REC_MASK)))[0]:
                errs.append(f"{name}: split {sp} word 7 (range): got {int(g[sp, 7] & np.uint32(REC_MASK))}, want {int(w[sp, 7] & np.uint32(REC_MASK))}")
            for bit, side, lk, s64 in ((30, "left", L, want["l64"]), (31, "right", R, want["r64"])):
                leaf = lk < 0
                bad = np.nonzero(leaf & (((g[:, 7] >> np.uint32(bit)) & 1) != ((w[:, 7] >> np.uint32(bit)) & 1)))[0]
                for sp in bad:
                    j = ~int(lk[sp])
                    hi = want["leaf64"][j][1::2]
                    errs.append(f"{name}: split {sp} word 7 bit {bit} ({flagbit} of the {side} child, leaf {j}): got {int(g[sp, 7] >> np.uint32(bit)) & 1}, "
                                f"want {int(w[sp, 7] >> np.uint32(bit)) & 1}; FP64 box {want['leaf64'][j].tolist()}; "
                                + "; ".join(f"hi.{'xyz'[a_]} {want['table'].state(a_, hi[a_])}" for a_ in range(3)))
    if errs:
        raise AssertionError(f"{len(errs)} words differ from the restatement (n = {n}, mode {want['table'].mode}):\n  " + "\n  ".join(errs[:12]))
    return compared


# ---------------------------------------------------------------- the theorem the encoding rests on, by brute force
def check_theorem(lo64, hi64, lo32, hi32, certain, what=""):
    """All pairs (a, b) of leaf boxes and all three axes; FP64 comparisons are exact, so they are the reference.  Uses nothing of enc's
    reasoning: only the FP64 bounds, the fp32 bounds and the CERTAIN flags it is handed (the restatement's, or the device's).
      conservative, all pairs:   a.lo < b.hi  =>  a.lo' < b.hi'
      exact, b CERTAIN:          a.lo' < b.hi'  <=>  a.lo < b.hi
      containment:               lo' <= lo  and  prox_hi(hi') >= hi   (how the other queries read a stored box)
    Returns (pairs x axes checked, of those with b certain)."""
    lo64, hi64 = np.asarray(lo64, dtype=np.float64).reshape(-1, 3), np.asarray(hi64, dtype=np.float64).reshape(-1, 3)
    lo32, hi32 = np.asarray(lo32, dtype=np.float32).reshape(-1, 3), np.asarray(hi32, dtype=np.float32).reshape(-1, 3)
    certain = np.asarray(certain, dtype=bool)
    n = lo64.shape[0]
    assert n <= 2048, "brute force: n^2 pairs"
    for a in range(3):
        lt64 = lo64[:, None, a] < hi64[None, :, a]
        lt32 = lo32[:, None, a] < hi32[None, :, a]
        lost = np.argwhere(lt64 & ~lt32)
        assert lost.size == 0, (f"{what}: axis {a}: a.lo < b.hi in FP64 but not in fp32 -- a pair would be lost", lost[:4].tolist(),
                                [(float(lo64[i, a]), float(hi64[j, a]), float(lo32[i, a]), float(hi32[j, a])) for i, j in lost[:4]])
        wrong = np.argwhere((lt64 != lt32) & certain[None, :])
        assert wrong.size == 0, (f"{what}: axis {a}: b is CERTAIN but the fp32 '<' does not decide what FP64 decides", wrong[:4].tolist(),
                                 [(float(lo64[i, a]), float(hi64[j, a]), float(lo32[i, a]), float(hi32[j, a])) for i, j in wrong[:4]])
    bad = np.argwhere(~(lo32.astype(np.float64) <= lo64))
    assert bad.size == 0, (f"{what}: lo' above lo", bad[:4].tolist())
    bad = np.argwhere(~(prox_hi(hi32).astype(np.float64) >= hi64))
    assert bad.size == 0, (f"{what}: prox_hi(hi') below hi", bad[:4].tolist())
    return 3 * n * n, 3 * n * int(certain.sum())


def leaf_merge_boxes(lo, hi, left, right, first, last):
    """Every child box as the min / max over the fp32 boxes of the leaves under it, by naive recursion through the links (children before
    parents: by range length), with the compare-selects of box.cuh:24-32 (the right operand on ties, so a zero keeps the device's
    sign in the stage-wise build).  -> (l_lo, l_hi, r_lo, r_hi) f32[n - 1, 3]."""
    m = left.shape[0]
    node_lo, node_hi = np.zeros((m, 3), dtype=np.float32), np.zeros((m, 3), dtype=np.float32)
    out = [np.zeros((m, 3), dtype=np.float32) for _ in range(4)]
    for s in np.argsort(np.asarray(last) - np.asarray(first), kind="stable"):
        c = []
        for link in (int(left[s]), int(right[s])):
            c.append((lo[~link], hi[~link]) if link < 0 else (node_lo[link], node_hi[link]))
        (alo, ahi), (blo, bhi) = c
        out[0][s], out[1][s], out[2][s], out[3][s] = alo, ahi, blo, bhi
        node_lo[s], node_hi[s] = np.where(alo < blo, alo, blo), np.where(ahi > bhi, ahi, bhi)
    return tuple(out)
