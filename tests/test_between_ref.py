"""CPU checks of the between-mesh restatement (tests/between_ref.py) and of the new entry points' argument errors.

The restatement must be what the self restatements say about the merged mesh: its triangles a's first (the smaller IDs), b's vertices
offset by a's nv.  Then every self predicate takes a's triangle first, no cross pair shares a vertex index, and the cross pairs of
oracle.brute_force (contact), proximity_ref.proximity_pairs and ccd_ref.ccd_pairs are exactly the between pairs, with the same distance
and toi bits.  Covered: split soups, meshes that share vertex positions but no indices, degenerate triangles; and the grid enumeration
of the restatement against its own every-pair enumeration."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import between_ref as br
import ccd_ref as cr
import mi355cd
import oracle
import proximity_ref as pr


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _cases():
    out = {}
    v, i = br.soup(600, 0.08, 3)
    out["soup_split"] = br.split(v, i, 250)
    v, i = br.soup(300, 0.12, 4)
    out["soup_split_1"] = br.split(v, i, 1)
    out["shared_positions"] = br.shared_positions(120, 5)
    v, i = br.with_degenerate(*br.soup(500, 0.1, 6), seed=6)
    out["degenerate"] = br.split(v, i, 200)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_contact_is_merged_cross_pairs(name):
    va, ia, vb, ib = CASES[name]
    got, tested = br.contact_pairs(va, ia, vb, ib)
    mv, mi = br.merge(va, ia, vb, ib)
    p, n, _ = oracle.brute_force(mv, mi, box_filter=True)
    cp = br.cross(p, ia.shape[0])[0]
    want = cp[np.lexsort((cp[:, 1], cp[:, 0]))]
    assert n < (1 << 22)
    assert np.array_equal(got, want), (name, got.shape, want.shape)
    # n_tested: the strict box test on every a x b pair, by the oracle's own box predicate
    ba, bb = oracle.box_set_batch(va, ia), oracle.box_set_batch(vb, ib)
    i, j = np.meshgrid(np.arange(ia.shape[0]), np.arange(ib.shape[0]), indexing="ij")
    assert tested == int(np.sum(oracle.box_overlap_batch(ba[i.ravel()], bb[j.ravel()]) != 0)), name


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("dist", [0.0, 0.01, 0.05])
def test_proximity_is_merged_cross_pairs(name, dist):
    va, ia, vb, ib = CASES[name]
    gp, gd = br.proximity_pairs(va, ia, vb, ib, dist)
    mv, mi = br.merge(va, ia, vb, ib)
    sp, sd = pr.proximity_pairs(mv, mi, None, dist)
    wp, wd = br.cross(sp, ia.shape[0], sd)
    assert np.array_equal(gp, wp), (name, dist)
    assert np.array_equal(_bits(gd), _bits(wd)), (name, dist)
    if dist == 0.0:                                     # dist 0: the contact pairs at 0, and pairs that only touch
        cp, _ = br.contact_pairs(va, ia, vb, ib)
        inside = np.isin(oracle.pair_set(gp), oracle.pair_set(cp))
        assert int(inside.sum()) == cp.shape[0] and np.all(gd == 0.0), name


@pytest.mark.parametrize("name", ["soup_split", "shared_positions", "degenerate"])
@pytest.mark.parametrize("moving", ["both", "a", "none"])
def test_ccd_is_merged_cross_pairs(name, moving):
    va, ia, vb, ib = CASES[name]
    dist = 0.01
    va1 = br.motion(va, 0.02, 1) if moving in ("both", "a") else None
    vb1 = br.motion(vb, 0.02, 2) if moving == "both" else None
    (gp, gt, gd), (tested, evals) = br.ccd_pairs(va, ia, vb, ib, dist, va1, vb1, counts=True)
    mv, mi = br.merge(va, ia, vb, ib)
    m1, _ = br.merge(va if va1 is None else va1, ia, vb if vb1 is None else vb1, ib)
    sp, st, sd = cr.ccd_pairs(mv, m1, mi, None, dist)
    wp, wt, wd = br.cross(sp, ia.shape[0], st, sd)
    assert gp.shape[0] > 0 and tested > 0 and evals >= tested
    assert np.array_equal(gp, wp), (name, moving)
    assert np.array_equal(_bits(gt), _bits(wt)) and np.array_equal(_bits(gd), _bits(wd)), (name, moving)


def test_grid_enumeration_equals_every_pair():
    va, ia, vb, ib = CASES["soup_split"]
    for brute in (True, False):
        assert br.contact_pairs(va, ia, vb, ib, brute=True)[1] == br.contact_pairs(va, ia, vb, ib, brute=brute)[1]
    a = br.proximity_pairs(va, ia, vb, ib, 0.03, brute=True)
    b = br.proximity_pairs(va, ia, vb, ib, 0.03, brute=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    x1 = br.motion(va, 0.02, 3)
    a = br.ccd_pairs(va, ia, vb, ib, 0.01, x1, None, brute=True)
    b = br.ccd_pairs(va, ia, vb, ib, 0.01, x1, None, brute=False)
    assert all(np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


def test_ids_are_each_contexts_own():
    va, ia, vb, ib = CASES["soup_split"]
    ida = np.arange(ia.shape[0], dtype=np.uint32) * 3 + 7
    idb = np.arange(ib.shape[0], dtype=np.uint32)[::-1].copy()
    p0, d0 = br.proximity_pairs(va, ia, vb, ib, 0.02)
    p1, d1 = br.proximity_pairs(va, ia, vb, ib, 0.02, ids_a=ida, ids_b=idb)
    # map back: the same pairs under the renaming
    inv_a = {int(x): k for k, x in enumerate(ida)}
    inv_b = {int(x): k for k, x in enumerate(idb)}
    back = np.array([[inv_a[int(x)], inv_b[int(y)]] for x, y in p1], dtype=np.uint32).reshape(-1, 2)
    bp, bd = pr.sort_pairs(back, d1)
    assert np.array_equal(bp, p0) and np.array_equal(_bits(bd), _bits(d0))


def test_null_contexts_are_argument_errors():
    """No device needed: the argument checks come before anything touches HIP.  (Fails where the library lacks the entry points.)"""
    lib = mi355cd.load_library()
    n, t = C.c_uint64(7), C.c_uint64(7)
    info = mi355cd.CdCcdInfo()
    assert lib.cd_find_collisions_between(None, None, None, 0, C.byref(n), C.byref(t)) == mi355cd.CD_ERR_ARG
    assert lib.cd_find_proximity_between(None, None, 0.0, None, None, 0, C.byref(n), C.byref(t)) == mi355cd.CD_ERR_ARG
    assert lib.cd_find_ccd_between(None, None, None, None, 0.01, None, None, None, 0, C.byref(n), C.byref(info)) == mi355cd.CD_ERR_ARG
    assert n.value == 7 and t.value == 7
    for name in ("cd_find_collisions_between", "cd_find_proximity_between", "cd_find_ccd_between"):
        assert name in mi355cd.EXPORTS
