"""The restatement of the plane queries (tests/plane_ref.py) against exact rational arithmetic, and what plane_tri's rule promises on
closed meshes: closed loops bit for bit and exact areas.  No device."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import closed_meshes as cm
import plane_ref as plr


def _exact(plane, tri):
    """Class and the cut edges (edge_a, edge_b) in rational arithmetic, by plane_tri's rule."""
    n = [Fraction(float(x)) for x in plane[:3]]
    d = Fraction(float(plane[3]))
    s = [sum(n[a] * Fraction(float(p[a])) for a in range(3)) - d for p in tri]
    below = [x < 0 for x in s]
    on = sum((1 << i) for i in range(3) if s[i] == 0)
    if all(below):
        return plr.BELOW, None, None, on
    if not any(below):
        return plr.ABOVE, None, None, on
    ea = [e for e in range(3) if not below[e] and below[(e + 1) % 3]]
    eb = [e for e in range(3) if below[e] and not below[(e + 1) % 3]]
    assert len(ea) == 1 and len(eb) == 1                                    # exactly two boundary edges change side
    return plr.CUT, ea[0], eb[0], on


@pytest.mark.parametrize("family", ["integer", "constructed", "random", "offset"])
def test_classes_and_cut_edges_are_exact(family):
    planes, tris = {"integer": plr.integer_family, "constructed": plr.constructed_family, "random": lambda: plr.random_family(0.0, 3000),
                    "offset": lambda: plr.random_family(plr.OFFSET, 3000)}[family]()
    cls, seg, edge, t, on = plr.plane_tri_np(planes, tris)
    seen = np.zeros(3, dtype=np.int64)
    exact_on = family in ("integer", "constructed")                         # there every s is computed without rounding
    for i in range(planes.shape[0]):
        c, ea, eb, o = _exact(planes[i], tris[i])
        if not exact_on and o:
            continue
        assert cls[i] == c, (family, i, cls[i], c)
        seen[c] += 1
        if c == plr.CUT:
            assert (edge[i, 0], edge[i, 1]) == (ea, eb), (family, i)
            assert (0.0 < t[i]).all() and (t[i] <= 1.0).all()
        else:
            assert not seg[i].any() and not t[i].any() and not edge[i].any()
        if exact_on:
            assert on[i] == o, (family, i)
    print(family, "above / below / cut:", seen.tolist(), "with a vertex in the plane:", int((on != 0).sum()))
    assert (seen[[plr.ABOVE, plr.CUT]] > planes.shape[0] // 20).all() and (family == "constructed" or seen[plr.BELOW] > planes.shape[0] // 20)   # (constructed: a vertex lies in the plane)
    if exact_on:
        # a vertex in the plane, an edge in it, a face in it: all occur, and a face in the plane is ABOVE
        nbits = np.array([bin(x).count("1") for x in on])
        few = 1 if family == "integer" else 50                            # (the constructed family is built to hold them)
        assert (nbits == 1).sum() > 50 and (nbits == 2).sum() >= few and (nbits == 3).sum() >= few
        assert (cls[nbits == 3] == plr.ABOVE).all()


def test_points_lie_on_their_edges_and_in_the_plane():
    planes, tris = plr.random_family(0.0, 5000)
    cls, seg, edge, t, on = plr.plane_tri_np(planes, tris)
    cut = cls == plr.CUT
    s = plr.side(tuple(planes[cut, k][:, None] for k in range(4)), tuple(seg[cut][:, :, a] for a in range(3)))
    scale = np.abs(planes[cut, :3]).sum(axis=1)[:, None]
    assert (np.abs(s) <= 64 * np.finfo(np.float64).eps * (scale + np.abs(planes[cut, 3:]))).all()      # a handful of roundings of terms of that size
    for which in (0, 1):
        e = edge[cut, which].astype(np.int64)
        p, q = tris[cut][np.arange(e.size), e], tris[cut][np.arange(e.size), (e + 1) % 3]
        pt = seg[cut][:, which]
        assert (pt >= np.minimum(p, q) - 1e-15).all() and (pt <= np.maximum(p, q) + 1e-15).all()


def test_a_face_below_touching_the_plane_is_a_row_with_a_equal_b():
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, -1.0], [0.0, 1.0, -1.0]]])
    cls, seg, edge, t, on = plr.plane_tri_np(np.array([[0.0, 0.0, 1.0, 0.0]]), tri)
    assert cls[0] == plr.CUT and on[0] == 1 and np.array_equal(seg[0, 0], seg[0, 1]) and np.array_equal(seg[0, 0], tri[0, 0]) and (t[0] == 1.0).all()
    # an edge in the plane: reported by the face below it, not by the face above it
    lower = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]]])
    upper = np.array([[[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]]])
    y0 = np.array([[0.0, 0.0, 1.0, 0.0]])
    c, s, e, tt, o = plr.plane_tri_np(y0, lower)
    assert c[0] == plr.CUT and o[0] == 3 and {tuple(s[0, 0]), tuple(s[0, 1])} == {(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)}
    assert plr.plane_tri_np(y0, upper)[0][0] == plr.ABOVE
    assert plr.plane_tri_np(np.array([[0.0, 0.0, 1.0, -0.0]]), np.array([[[0.0, 0.0, -0.0], [1.0, 0.0, 0.0], [0.0, 1.0, -0.0]]]))[0][0] == plr.ABOVE     # -0.0 is not below


@pytest.mark.parametrize("name,normal,d,want_area,want_loops", plr.CLOSED_CASES)
def test_sections_of_closed_meshes_are_closed_loops(name, normal, d, want_area, want_loops):
    v, f, ids, _ = plr.mesh(name)
    assert cm.signed_volume(v - v.mean(axis=0), f) > 0
    plane = np.array([[*normal, d]])
    w = plr.planes_cut_all_ref(v, f, None, plane)
    assert plr.loops_closed(w.seg), name
    got = plr.area(w.seg, normal)
    print(name, normal, d, "rows", w.rows.shape[0], "area", got, "loops", plr.n_loops(w.seg))
    if want_area is not None:
        assert got == want_area, (got, want_area)
    else:
        assert got >= 0.0
    if want_loops is not None:
        assert plr.n_loops(w.seg) == want_loops
    if want_loops != 0:
        assert w.rows.shape[0] > 0
    n_cut, n_below, n_above = plr.planes_count_ref(v, f, plane)
    assert n_cut[0] == w.rows.shape[0] and n_cut[0] + n_below[0] + n_above[0] == f.shape[0]


def test_every_plane_of_the_shared_sets_gives_closed_loops_on_closed_meshes():
    for name in plr.CLOSED:
        w = plr.want_rows(name, 200)
        pl = plr.planes(name, 200)
        for k in range(200):
            mine = w.rows[:, 0] == k
            assert plr.loops_closed(w.seg[mine]), (name, k, pl[k])
            assert plr.area(w.seg[mine], pl[k, :3]) >= -1e-12, (name, k)


def test_brute_force_rows_and_counts_agree_and_the_inputs_hold_what_the_gpu_test_needs():
    for name in plr.NAMES[:8] + plr.SOUPS[:5] + plr.CLOSED:
        plr.input_conditions(name)
        w, cls = plr.want_rows(name), plr.want_classes(name)
        n_cut = plr.counts_of_classes(cls)[0]
        assert np.array_equal(np.bincount(w.rows[:, 0].astype(np.int64), minlength=1000), n_cut)
        keys = w.rows[:, 0].astype(np.uint64) << np.uint64(32) | w.rows[:, 1].astype(np.uint64)
        assert np.unique(keys).size == keys.size


def test_scaling_by_a_power_of_two_changes_nothing():
    import scale_inputs as si
    planes, tris = plr.random_family(0.0, 4000)
    want = plr.plane_tri_np(planes, tris)
    for k in (-300, -149, 128, 300):
        pk = planes.copy()
        pk[:, 3] = si.scaled(pk[:, 3], k)
        cls, seg, edge, t, on = plr.plane_tri_np(pk, si.scaled(tris, k))
        assert np.array_equal(cls, want[0]) and np.array_equal(edge, want[2]) and np.array_equal(on, want[4])
        assert np.array_equal(t.view(np.uint64), want[3].view(np.uint64))
        assert np.array_equal(seg.view(np.uint64), si.scaled(want[1], k).view(np.uint64))
