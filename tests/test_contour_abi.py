"""The contour entry points: the exports, the record's layout, the argument errors that need no device (the pattern of
tests/test_abi.py), and -- on the device -- the order errors."""
import ctypes as C

import numpy as np
import pytest

import mi355cd


def _record(rows=4):
    faces = np.zeros((rows, 2), dtype=np.uint32)
    code = np.zeros((rows, 3), dtype=np.uint8)
    return mi355cd.CdContourOut(faces.ctypes.data, code.ctypes.data, None, None), (faces, code)


def test_exports_and_layout():
    lib = mi355cd.load_library()
    for name in ("cd_find_collisions_contour", "cd_find_collisions_between_contour", "cd_tri_isect_points"):
        assert name in mi355cd.EXPORTS and hasattr(lib, name)
    assert [f for f, _ in mi355cd.CdContourOut._fields_] == ["faces", "code", "param", "points"]
    assert C.sizeof(mi355cd.CdContourOut) == 4 * C.sizeof(C.c_void_p)
    for k, f in enumerate(("faces", "code", "param", "points")):
        assert getattr(mi355cd.CdContourOut, f).offset == k * C.sizeof(C.c_void_p)


def test_contour_argument_errors_do_not_need_a_device():
    lib = mi355cd.load_library()
    w, keep = _record()
    n = C.c_uint64(0)
    pairs = np.zeros((4, 2), dtype=np.uint32)
    for wp in (None, C.byref(w), C.byref(mi355cd.CdContourOut())):
        assert lib.cd_find_collisions_contour(None, pairs.ctypes.data, 4, C.byref(n), None, wp) == mi355cd.CD_ERR_ARG
        assert lib.cd_find_collisions_between_contour(None, None, pairs.ctypes.data, 4, C.byref(n), None, wp) == mi355cd.CD_ERR_ARG
    tri = np.zeros((4, 18))
    code = np.zeros((4, 3), dtype=np.uint8)
    assert lib.cd_tri_isect_points(None, 4, code.ctypes.data, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_tri_isect_points(tri.ctypes.data, 4, None, None, None) == mi355cd.CD_ERR_ARG            # code is not optional
    assert lib.cd_tri_isect_points(tri.ctypes.data, 0, code.ctypes.data, None, None) == mi355cd.CD_OK     # n = 0: nothing to do
    c, p, x = mi355cd.tri_isect_points(np.zeros((0, 6, 3)))
    assert c.shape == (0, 3) and p.shape == (0, 2, 3) and x.shape == (0, 2, 3)
    assert not any(a.any() for a in keep) and not code.any() and n.value == 0


@pytest.mark.gpu
def test_order_and_argument_errors():
    import between_ref as br
    verts, vidx = br.soup(65, 0.3, 41)
    bv, bi = br.soup(63, 0.3, 31)
    with mi355cd.CollisionDetector(verts, vidx) as cd, mi355cd.CollisionDetector(bv, bi) as ob:
        calls = {"self": lambda: cd.find_collisions_contour(), "between": lambda: cd.find_collisions_between_contour(ob),
                 "between, swapped": lambda: ob.find_collisions_between_contour(cd)}

        def rc_of(fn):
            with pytest.raises(mi355cd.CdError) as e:
                fn()
            return e.value.rc

        ob.build_tree()
        for what, fn in calls.items():                                          # before a tree
            assert rc_of(fn) == mi355cd.CD_ERR_ORDER, what
        n = C.c_uint64(0)
        pairs = np.zeros((64, 2), dtype=np.uint32)
        assert cd.lib.cd_find_collisions_contour(cd._ctx, pairs.ctypes.data, 64, C.byref(n), None, None) == mi355cd.CD_ERR_ORDER   # NULL w too
        cd.build_tree()
        for what, fn in calls.items():
            assert fn()[2] == mi355cd.CD_OK, what
        cd.update_vertices(verts)                                               # vertices newer than the tree
        for what, fn in calls.items():
            assert rc_of(fn) == mi355cd.CD_ERR_ORDER, what
        assert cd.lib.cd_find_collisions_contour(cd._ctx, pairs.ctypes.data, 64, C.byref(n), None, None) == mi355cd.CD_ERR_ORDER
        cd.build_tree()
        ob.update_vertices(bv)                                                  # ... or the other mesh's
        assert calls["self"]()[2] == mi355cd.CD_OK
        for what in ("between", "between, swapped"):
            assert rc_of(calls[what]) == mi355cd.CD_ERR_ORDER, what
        ob.build_tree()
        assert rc_of(lambda: cd.find_collisions_between_contour(cd)) == mi355cd.CD_ERR_ARG            # a == b
        w, keep = _record(64)
        for wp in (None, C.byref(w)):                                           # cap_pairs > 0 without pairs
            assert cd.lib.cd_find_collisions_contour(cd._ctx, None, 64, C.byref(n), None, wp) == mi355cd.CD_ERR_ARG
            assert cd.lib.cd_find_collisions_between_contour(cd._ctx, ob._ctx, None, 64, C.byref(n), None, wp) == mi355cd.CD_ERR_ARG
        assert not any(a.any() for a in keep)
