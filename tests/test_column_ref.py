"""The numpy restatement of column_tri and the per-point sums (tests/column_ref.py) against answers known in closed form, on the CPU:
the unit box at lattice points that sit exactly under its vertices and edges, the torus against its analytic distance, nested and
open boxes.  No exceptions are allowed: where the arithmetic is exact the counts are the moved point's.  And its equivariance under
powers of two over tests/scale_inputs.SCALES, which the device's range test (tests/test_inside_gpu.py) rests on."""
import numpy as np
import pytest

import closed_meshes as cm
import column_ref as ref
import scale_inputs as si

AXES = (0, 1, 2)


def test_the_meshes_are_closed_and_outward():
    for verts, faces in (cm.box_grid(4), cm.torus(24, 12), cm.nested_boxes(4, invert_inner=False)):
        e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
        fwd = set(map(tuple, e))
        assert len(fwd) == e.shape[0] and all((b, a) in fwd for a, b in fwd)      # every directed edge once, with its reverse
        assert cm.signed_volume(verts, faces) > 0
    v, f = cm.box_grid(4)
    assert v.shape == (98, 3) and f.shape == (192, 3) and cm.signed_volume(v, f) == pytest.approx(1.0)
    assert cm.signed_volume(v, cm.inverted(f)) == pytest.approx(-1.0)


@pytest.mark.parametrize("axis", AXES)
def test_box_lattice_is_the_moved_points_answer(axis):
    verts, faces = cm.box_grid(4)
    pts = cm.lattice(axis)
    want = cm.lattice_inside(pts, axis)
    inside, na, nb, wa, wb = ref.points_inside(pts, verts, faces, axis)
    assert pts.shape[0] == 1331 and want.sum() == 8 * 8 * 8
    assert np.array_equal(inside, want)
    assert np.array_equal(wa + wb, np.zeros_like(wa))
    assert np.array_equal(wa, want.astype(np.int32))
    assert np.array_equal(ref.points_inside(pts, verts, faces, axis, parity=True)[0], want)
    inv = ref.points_inside(pts, verts, cm.inverted(faces), axis)
    assert np.array_equal(inv[3], -wa) and np.array_equal(inv[4], -wb)
    assert np.array_equal(inv[1], na) and np.array_equal(inv[2], nb)


@pytest.mark.parametrize("axis", AXES)
def test_torus_agrees_with_the_analytic_sign(axis):
    verts, faces = cm.torus(24, 12)
    pts, want = cm.torus_points()
    assert pts.shape[0] > 3000 and 100 < want.sum() < pts.shape[0] - 100
    inside, na, nb, wa, wb = ref.points_inside(pts, verts, faces, axis)
    assert np.array_equal(inside, want)
    assert np.array_equal(wa + wb, np.zeros_like(wa))
    assert np.array_equal((na & 1) != 0, want)


@pytest.mark.parametrize("axis", AXES)
def test_nested_boxes_cavity_and_solid(axis):
    between = np.array([[0.125, 0.5, 0.5], [0.5, 0.125, 0.5], [0.5, 0.5, 0.125], [0.875, 0.53, 0.47]])
    core = np.array([[0.5, 0.5, 0.5], [0.3, 0.6, 0.7]])
    v, f = cm.nested_boxes(4, invert_inner=True)
    assert np.array_equal(ref.points_inside(between, v, f, axis)[3], [1, 1, 1, 1])
    assert np.array_equal(ref.points_inside(core, v, f, axis)[3], [0, 0])         # the cavity
    v, f = cm.nested_boxes(4, invert_inner=False)
    assert np.array_equal(ref.points_inside(between, v, f, axis)[3], [1, 1, 1, 1])
    assert np.array_equal(ref.points_inside(core, v, f, axis)[3], [2, 2])         # both shells wind around it
    assert np.array_equal(ref.points_inside(core, v, f, axis, parity=True)[0], [False, False])


def test_nested_boxes_column_through_both_shells():
    """A point between the shells whose column also passes through the inner box: three faces above it, and the inner shell's two
    crossings cancel whichever way it is oriented -- w = 1, the solid between the shells, either way."""
    p = np.array([[0.5, 0.5, 0.125]])
    for invert in (True, False):
        _, na, nb, wa, wb = ref.points_inside(p, *cm.nested_boxes(4, invert), 2)
        assert (na[0], nb[0], wa[0], wb[0]) == (3, 1, 1, -1)


def test_open_box_shows_the_hole():
    verts, faces, _ = cm.open_box(4)
    pts = cm.lattice(2)
    want = cm.lattice_inside(pts, 2)
    _, na, nb, wa, wb = ref.points_inside(pts, verts, faces, 2)
    hole = (0 <= pts[:, 0]) & (pts[:, 0] < 1) & (0 <= pts[:, 1]) & (pts[:, 1] < 1)   # the columns through the missing top
    assert np.array_equal((wa + wb) != 0, hole)
    assert np.array_equal((wa + wb)[hole], np.full(hole.sum(), -1))                  # the bottom (o = -1) is there, the top is not
    # an x or y column never crosses the missing side (it is parallel to them: a line in projection): another axis avoids the hole
    for axis in (0, 1):
        p = cm.lattice(axis)
        inside, _, _, wa, wb = ref.points_inside(p, verts, faces, axis)
        assert not (wa + wb).any() and np.array_equal(inside, cm.lattice_inside(p, axis))
    assert want.any()


def test_ties_and_degenerate_faces():
    tri = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    mirror = np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [0.0, 1.0, 1.0]])            # shares the edge (1,0)-(0,1)
    for p in ([0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.25, 0.0]):
        r = [int(ref.column_tri(np.array(p), t, 2)["cover"]) for t in (tri, mirror)]
        moved = np.array(p) + [1e-9, 1e-18, 0.0]
        m = [int(ref.column_tri(moved, t, 2)["cover"]) for t in (tri, mirror)]
        assert r == m, (p, r, m)
    line = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 5.0]])              # a line in projection
    assert int(ref.column_tri(np.array([1.0, 1.0, 0.0]), line, 2)["cover"]) == 0
    dot = np.array([[1.0, 1.0, 0.0]] * 3)
    assert int(ref.column_tri(np.array([1.0, 1.0, -1.0]), dot, 2)["cover"]) == 0
    nan = tri.copy()
    nan[1, 2] = np.nan                                                                # only the height is NaN: covered, not counted
    r = ref.column_tri(np.array([0.25, 0.25, 0.0]), nan, 2)
    assert int(r["cover"]) == 1 and not bool(r["counted"]) and not bool(r["above"])
    on = ref.column_tri(np.array([0.25, 0.25, 1.0]), tri, 2)                          # the point ON the face is below
    assert int(on["cover"]) == 1 and bool(on["counted"]) and not bool(on["above"])


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("name", list(si.meshes()))
def test_points_inside_is_equivariant_under_powers_of_two(name, axis):
    """scale_inputs' meshes and inside points times 2^k for every k of SCALES: the same five integer arrays as at k = 0, also with
    parity (no E, S or zc over- or underflows in FP64 over that band, so every sign and every exact zero is the unscaled one's).
    A condition on the inputs: at least 200 of the points have a face over or under them, and some cover is the tie rule's."""
    v, vidx, edge = si.meshes()[name]
    pts = si.inside_points(name, axis)
    want = si.want_inside(name, axis)
    crossed = int(((want[1] + want[2]) > 0).sum())
    under = pts[si.INSIDE_RANDOM:]
    r = ref.column_tri(under[:, None, :], v[vidx.astype(np.int64)][None], axis)
    ties = int(((r["cover"] != 0) & (r["E"] == 0).any(axis=-1)).any(axis=1).sum())
    print(f"{name} axis {axis}: {pts.shape[0]} points, {crossed} with a face over or under them, {int(want[0].sum())} inside, {ties} covers by the tie rule")
    assert pts.shape[0] == si.INSIDE_RANDOM + (v.shape[0] + 9) // 10 and crossed >= 200 and ties > 0
    for k in si.SCALES:                                                          # every scale, on every mesh and axis: none is left out
        got = si.want_inside(name, axis, k)
        for j, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, axis, k, j, int((g != w).sum()))
        if k in si.EDGES:
            for g, w in zip(si.want_inside(name, axis, k, True), si.want_inside(name, axis, 0, True)):
                assert np.array_equal(g, w), (name, axis, k, "parity")
