"""tests/nearest_ref.py against itself and against what it is built from (no GPU): nearest_rows is the reduction of
witness_ref.witness_pairs_between's rows that defines the query, its distances are the direct all-pairs minimum of
proximity_ref.tri_distance_np, and ties go to the smaller ID, then the smaller face."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import nearest_ref as nr
import proximity_ref as pr

NAMES = ("soup_2_600_s4", "soup_700_900_s5")
CASES = nr.between_cases()


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    for x, y, f in zip(a, b, a._fields):
        same = np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float64 else np.array_equal(x, y)
        assert same, (what, f)


@functools.lru_cache(maxsize=None)
def _rows(name):
    return nr.nearest_rows(*CASES[name], np.inf)


@pytest.mark.parametrize("name", NAMES)
def test_distances_are_the_all_pairs_minimum(name):
    va, ia, vb, ib = CASES[name]
    ta, tb = va[ia.astype(np.int64)], vb[ib.astype(np.int64)]
    na, nb = ta.shape[0], tb.shape[0]
    i, j = np.meshgrid(np.arange(na), np.arange(nb), indexing="ij")
    d = pr.tri_distance_np(np.concatenate([ta[i.ravel()], tb[j.ravel()]], axis=1)).reshape(na, nb)
    rows = _rows(name)
    assert (rows.faces[:, 0] == np.arange(na)).all() and (rows.ids == rows.faces).all()
    assert np.array_equal(_bits(rows.dist), _bits(d.min(axis=1)))
    assert np.array_equal(_bits(d[np.arange(na), rows.faces[:, 1]]), _bits(rows.dist))
    assert (rows.faces[:, 1] == d.argmin(axis=1)).all()                        # IDs are face indices here: the first minimum wins
    m = nr.nearest_min(rows)
    assert m.dist[0] == d.min() and tuple(m.faces[0]) == tuple(np.argwhere(d == d.min())[0])


@pytest.mark.parametrize("name", NAMES)
def test_rows_are_the_reduction_of_the_witness_rows(name):
    va, ia, vb, ib = CASES[name]
    rows = _rows(name)
    if name == NAMES[0]:                                                       # (the witness of ALL pairs of the larger case takes 10 s)
        _same(rows, nr.rows_of_all_pairs(va, ia, vb, ib, np.inf), name)
    r = float(np.median(rows.dist))
    assert 0 < int((rows.dist <= r).sum()) < rows.dist.shape[0] or rows.dist.shape[0] < 3
    at_r = nr.nearest_rows(va, ia, vb, ib, r)
    _same(at_r, nr.rows_of_all_pairs(va, ia, vb, ib, r), f"{name} r={r}")
    _same(nr.within(rows, r), at_r, f"{name} within r={r}")
    lone = nr.within(rows, 0.0)
    none = lone.faces[:, 0] == nr.NONE
    assert (lone.dist[none] == np.inf).all() and (lone.dist[~none] == 0.0).all() and (lone.feature[~none] == 7).all()
    assert not lone.points[none].any() and not lone.bary[none].any() and not lone.feature[none].any() and not lone.ids[none].any()
    assert (lone.faces[none, 1] == nr.NONE).all()


@pytest.mark.parametrize("name", NAMES)
def test_ties_go_to_the_smaller_id_then_the_smaller_face(name):
    va, ia, vb, ib = CASES[name]
    nb = ib.shape[0]
    rows = _rows(name)
    vb2, ib2 = nr.doubled(vb, ib)
    # even faces: the second copy has the smaller ID and wins although its face index is larger; odd faces: both copies have the
    # same ID and the smaller face index wins
    even = np.arange(nb) % 2 == 0
    ids_b = np.concatenate([np.arange(nb) + nb * even, np.arange(nb)]).astype(np.uint32)
    r = nr.nearest_rows(va, ia, vb2, ib2, np.inf, None, ids_b)
    assert np.array_equal(_bits(r.dist), _bits(rows.dist))
    fb = rows.faces[:, 1]
    assert (r.faces[:, 1] == fb + nb * even[fb]).all() and (r.ids[:, 1] == fb).all()
    _same(rows._replace(faces=r.faces, ids=r.ids), r, name)
    if name != NAMES[0]:
        return
    # the five-key minimum: with a doubled a as well, the smaller ID in a decides before anything of b
    va2, ia2 = nr.doubled(va, ia)
    na = ia.shape[0]
    ids_a = np.concatenate([np.arange(na) + na, np.arange(na)]).astype(np.uint32)
    m0 = nr.nearest_min(rows)
    m = nr.nearest_min(nr.nearest_rows(va2, ia2, vb2, ib2, np.inf, ids_a, ids_b))
    assert m.dist[0] == m0.dist[0] and m.faces[0, 0] == m0.faces[0, 0] + na and m.ids[0, 0] == m0.faces[0, 0] and m.faces[0, 1] == m0.faces[0, 1]
