"""CPU checks of the self-proximity restatement (tests/proximity_ref.py) and of the new entry points' argument errors.

The restatement is compared with the EXACT rational minimum of the 15 feature-pair squared distances.  Every term of
tri_distance is |P - Q| for two points that lie on the two triangles up to the rounding of forming them, so its error is
a few ulps of the coordinates whatever the conditioning; measured here against exact rationals on near-parallel edges,
coplanar pairs, degenerate triangles and coordinates scaled by 1e+-100, the error stays below TOL_REL = 2^-40 of the
pair's largest |coordinate|.  The device filter's slack (2^-20 of the root box's largest |coordinate|, DESIGN.md
section 10) rests on that bound with a factor of 2^20 to spare."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import mi355cd
import proximity_ref as pr
import scale_inputs as si

TOL_REL = 2.0 ** -40


def _rng(seed):
    return np.random.default_rng(seed)


def _pair_sets(n=400):
    """f64[k, 6, 3] pairs of several kinds (a few thousand in all)."""
    g = _rng(7)
    sets = {}
    a = g.uniform(-1, 1, (n, 6, 3)); a[:, 3:] += g.uniform(-1.5, 1.5, (n, 1, 3))
    sets["random"] = a
    # near-parallel edges: two thin triangles along almost the same direction, a small gap apart
    b = np.zeros((n, 6, 3)); d = g.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = d + g.normal(size=(n, 3)) * 1e-9; o = g.normal(size=(n, 3)) * 1e-3
    b[:, 1] = d; b[:, 2] = d * 0.5 + g.normal(size=(n, 3)) * 0.3
    b[:, 3] = o + 0.2 * d; b[:, 4] = o + 0.2 * d + e; b[:, 5] = o + g.normal(size=(n, 3)) * 0.3 + d
    sets["near_parallel"] = b
    # coplanar and disjoint: both in z = c
    c = g.uniform(-1, 1, (n, 6, 3)); c[:, :, 2] = 0.25; c[:, 3:, 0] += 2.5
    sets["coplanar"] = c
    # degenerate: a repeated vertex, collinear vertices, a point
    dg = g.uniform(-1, 1, (n, 6, 3)); dg[:, 3:] += 1.2
    k = n // 3
    dg[:k, 1] = dg[:k, 0]
    dg[k:2 * k, 2] = dg[k:2 * k, 0] + 0.37 * (dg[k:2 * k, 1] - dg[k:2 * k, 0])
    dg[2 * k:, 4] = dg[2 * k:, 3]; dg[2 * k:, 5] = dg[2 * k:, 3]
    sets["degenerate"] = dg
    sets["huge"] = a[: n // 2] * 1e100
    sets["tiny"] = a[: n // 2] * 1e-100
    return sets


@pytest.mark.parametrize("kind", ["random", "near_parallel", "coplanar", "degenerate", "huge", "tiny"])
def test_restatement_matches_exact_rationals(kind):
    t = _pair_sets()[kind]
    contact = pr.oracle.tri_contact_points(t.reshape(-1, 18))
    got = pr.tri_distance_np(t, contact)
    checked = 0
    zero = pr.in_contact(t, contact)
    for k in np.nonzero(~zero)[0]:
        ex = math.sqrt(pr.exact_d2(t[k]))
        scale = float(np.max(np.abs(t[k] - t[k, 0])))
        assert np.isfinite(got[k])
        assert abs(got[k] - ex) <= TOL_REL * scale, (kind, k, got[k], ex, scale)
        checked += 1
    assert checked >= 100
    assert np.all(got[zero] == 0.0)


def test_known_answers():
    h = 0.375
    par = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, h], [1, 0, h], [0, 1, h]]], dtype=np.float64)
    assert pr.tri_distance_np(par)[0] == h
    touch = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.25, 0], [1, 1, 1], [2, 1, 1]]], dtype=np.float64)
    assert pr.tri_distance_np(touch)[0] == 0.0
    pt = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.25, 3], [0.25, 0.25, 3], [0.25, 0.25, 3]]], dtype=np.float64)
    assert pr.tri_distance_np(pt)[0] == 3.0                                 # a single-point triangle over a face
    # degenerate triangles get the distance of their point set, although the 17-axis test (all of whose axes are zero
    # between them) says "contact": their boxes do not overlap, so the collision path does not call them in contact
    pts = np.array([[[0, 0, 0], [0, 0, 0], [0, 0, 0], [3, 4, 0], [3, 4, 0], [3, 4, 0]]], dtype=np.float64)
    assert pr.oracle.tri_contact_points(pts.reshape(-1, 18))[0] == 1
    assert pr.tri_distance_np(pts)[0] == 5.0                                # two points
    ps = np.array([[[0, 0, 0], [0, 0, 0], [0, 0, 0], [12, 0, 5], [12, 10, 5], [12, 5, 5]]], dtype=np.float64)
    assert pr.tri_distance_np(ps)[0] == 13.0                                # a point and a segment triangle
    ss = np.array([[[0, 0, 0], [4, 0, 0], [2, 0, 0], [0, 0, 7], [4, 0, 7], [1, 0, 7]]], dtype=np.float64)
    assert pr.tri_distance_np(ss)[0] == 7.0                                 # two parallel segment triangles
    seg = np.array([[[-1, 0, 0], [1, 0, 0], [0, 0, 0], [0, -1, 2], [0, 1, 2], [0, 0, 2]]], dtype=np.float64)
    assert pr.tri_distance_np(seg)[0] == 2.0


def test_proximity_pairs_small_mesh():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5], [5, 5, 5], [6, 5, 5], [5, 6, 5]], dtype=np.float64)
    vidx = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.uint32)
    p, d = pr.proximity_pairs(verts, vidx, dist=0.5)
    assert p.tolist() == [[0, 1]] and d.tolist() == [0.5]
    p, d = pr.proximity_pairs(verts, vidx, dist=0.4999)
    assert p.shape[0] == 0


def _duplicates_mesh():
    import mi355_synth as synth
    verts, vidx = synth.soup(500, 0.2, 21)
    v2 = np.concatenate([verts, verts[:300]], axis=0)
    dup = (np.arange(300, dtype=np.uint32) + verts.shape[0]).reshape(100, 3)
    vi = np.concatenate([vidx, dup, np.array([[0, 0, 1], [5, 5, 5]], dtype=np.uint32), vidx[:50]], axis=0)
    return v2, vi


@pytest.mark.parametrize("dist", [0.0, 0.02, 0.2, 2.2])
def test_grid_enumeration_equals_all_pairs(dist):
    """The grid's box filter decides nothing: every pair at distance <= dist is among its candidates -- degenerate triangles
    (a segment triangle, a point triangle) included."""
    v, i = _duplicates_mesh()
    a = pr.proximity_pairs(v, i, None, dist, brute=True)
    b = pr.proximity_pairs(v, i, None, dist, brute=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    seg_pt = [k for k, p in enumerate(a[0].tolist()) if p == [600, 601]]
    assert (len(seg_pt) == 1) == (dist >= 2.2)                             # triangles 600 / 601: 2.105 apart


def test_proximity_entry_points_reject_bad_arguments():
    lib = mi355cd.load_library()
    n = C.c_uint64(0)
    for fn in (lib.cd_find_proximity, lib.cd_self_proximity):
        assert fn(None, 0.1, None, None, 0, C.byref(n), None) == mi355cd.CD_ERR_ARG
        for bad in (float("nan"), -1.0, float("inf")):
            # a non-null context pointer that is never dereferenced: the distance is checked first
            assert fn(C.c_void_p(8), bad, None, None, 0, C.byref(n), None) == mi355cd.CD_ERR_ARG
    assert lib.cd_tri_distance_points(None, 1, None) == mi355cd.CD_ERR_ARG


@pytest.mark.parametrize("name", list(si.meshes()))
def test_restatement_is_equivariant_under_powers_of_two(name):
    """Scaling a mesh by 2^k over scale_inputs.SCALES (past both ends of the fp32 range) scales every distance by 2^k exactly and
    changes neither the pairs in contact nor the oracle's collision pairs: the fact the device's range tests
    (tests/test_query_scales_gpu.py) compare against."""
    v, vidx, edge = si.meshes()[name]
    n = vidx.shape[0]
    tv = v[vidx.astype(np.int64)]
    c = pr._candidates(tv.min(axis=1) - edge / 2, tv.max(axis=1) + edge / 2)      # every pair whose boxes are at most `edge` apart
    i, j = c[:, 0], c[:, 1]
    keep = ~(vidx[i][:, :, None] == vidx[j][:, None, :]).any(axis=(1, 2))
    pairs = np.concatenate([tv[i[keep]], tv[j[keep]]], axis=1)
    assert pairs.shape[0] > 5 * n
    d0 = pr.tri_distance_np(pairs)
    z0 = pr.in_contact(pairs)
    coll0 = pr.oracle.pair_set(pr.oracle.brute_force(v, vidx)[0])
    dist = edge / 4
    p0, pd0 = pr.proximity_pairs(v, vidx, None, dist, brute=False)
    assert z0.sum() >= 50 and coll0.size == z0.sum() and p0.shape[0] > z0.sum()
    for k in si.SCALES:
        dk = pr.tri_distance_np(si.scaled(pairs, k))
        bad = np.nonzero(dk.view(np.uint64) != np.ldexp(d0, k).view(np.uint64))[0]
        assert bad.size == 0, (k, bad.size, bad[:3])
        assert np.array_equal(pr.in_contact(si.scaled(pairs, k)), z0), k
        assert np.array_equal(pr.oracle.pair_set(pr.oracle.brute_force(si.scaled(v, k), vidx)[0]), coll0), k
        pk, pdk = pr.proximity_pairs(si.scaled(v, k), vidx, None, np.ldexp(dist, k), brute=False)
        assert np.array_equal(pk, p0) and np.array_equal(pdk.view(np.uint64), np.ldexp(pd0, k).view(np.uint64)), k
