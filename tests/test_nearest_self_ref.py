"""tests/nearest_self_ref.py against a second derivation and against what follows from the definition (CPU only)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import between_ref as br
import mi355_synth as synth
import nearest_ref as nr
import nearest_self_ref as ns
import witness_ref as wr

NONE = ns.NONE


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _same(got, want, what):
    (g, gp), (w, wp) = got, want
    assert np.array_equal(gp, wp), what
    for name, x, y in zip(g._fields, g, w):
        same = np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float64 else np.array_equal(x, y)
        assert same, (what, name)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return synth.cloth_pair(8) if name == "cloth8" else br.soup(700, 0.06, 5)


@functools.lru_cache(maxsize=None)
def _rows(name):
    return ns.nearest_rows(*_mesh(name))


@pytest.mark.parametrize("name", ["cloth8", "soup700"])
def test_rows_equal_the_witness_pairs_reduced_per_face(name):
    """The second derivation: witness_ref.witness_pairs at dist = 2 x diameter -- every admissible pair with its witness -- reduced."""
    v, i = _mesh(name)
    n = np.asarray(i).reshape(-1, 3).shape[0]
    r = wr.witness_pairs(v, i, None, 2.0 * ns.diameter(v), brute=True)
    want = ns.reduce_pairs(n, r.faces, r.pairs, r.dists, r.points, r.bary, r.feature)
    got = _rows(name)
    _same(got, want, name)
    assert (got[0].faces[:, 0] == np.arange(n)).all()                           # every face has an admissible partner here
    med = float(np.median(got[0].dist))
    r = wr.witness_pairs(v, i, None, med, brute=True)
    _same(ns.within(got, med), ns.reduce_pairs(n, r.faces, r.pairs, r.dists, r.points, r.bary, r.feature), f"{name} within the median")


@pytest.mark.parametrize("name", ["cloth8", "soup700"])
def test_partner_is_at_least_as_near(name):
    """The pair (i, f) is a candidate of row f too, with the same bits: dist[partner[i]] <= dist[i]."""
    rows, played = _rows(name)
    found = rows.faces[:, 0] != NONE
    f = rows.faces[found, 1].astype(np.int64)
    assert (rows.dist[f] <= rows.dist[found]).all()
    assert (np.sort(played[found], axis=1) == np.sort(rows.faces[found], axis=1)).all()
    m, mp = ns.nearest_min((rows, played))
    assert m.dist[0] == rows.dist.min() and rows.dist[m.faces[0, 1]] == m.dist[0]
    if name == "cloth8":
        assert m.dist[0] == 0.0 and (m.feature == wr.FEATURE_NONE).all()        # the sheets intersect


def test_fan_has_no_admissible_pair():
    v, i = ns.fan(40)
    a, b = ns.admissible_pairs(i)
    assert i.shape[0] == 40 and a.size == 0 and b.size == 0
    got = ns.nearest_rows(v, i)
    _same(got, ns.nothing(40), "fan")
    _same(ns.nearest_min(got), ns.nothing(1), "fan MIN")
    v, i = ns.fan_and_far(40)
    rows, played = ns.nearest_rows(v, i)
    assert (rows.faces[:40, 1] == 40).all() and rows.faces[40, 0] == 40 and rows.faces[40, 1] == int(np.argmin(rows.dist[:40]))


@pytest.mark.parametrize("ids", ["nine", "mod3", None])
def test_doubled_mesh_the_coincident_copy_wins_at_zero(ids):
    v, i = nr.doubled(*br.soup(150, 0.1, 42))
    n = i.shape[0]
    idv = {"nine": np.full(n, 9, dtype=np.uint32), "mod3": (np.arange(n) % 3).astype(np.uint32), None: None}[ids]
    rows, played = ns.nearest_rows(v, i, ids=idv)
    assert (rows.dist == 0.0).all() and (rows.feature == wr.FEATURE_NONE).all()
    if ids == "nine":
        # all IDs equal: among the partners at 0 the smaller face index decides; the copy is one of them
        k = np.arange(150)
        assert (rows.faces[k, 1] <= k + 150).all() and (rows.faces[k + 150, 1] <= k).all()
        assert (played[:, 0] < played[:, 1]).all()
        m, mp = ns.nearest_min((rows, played))
        assert m.faces[0, 0] == 0
    else:
        eid = np.arange(n) if idv is None else idv.astype(np.int64)
        f = rows.faces[:, 1].astype(np.int64)
        copy = (np.arange(n) + 150) % n
        assert ((eid[f] < eid[copy]) | ((eid[f] == eid[copy]) & (f <= copy))).all()      # nothing beats the winner; the copy is at 0
