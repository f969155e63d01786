"""The C-ABI surface of cd_points_inside, cd_signed_distance and cd_column_tri_points, without a GPU: the symbols are exported and
bound, and their argument errors need no device."""
import ctypes as C

import mi355cd


def test_symbols_are_exported_and_bound():
    lib = mi355cd.load_library()
    for name, nargs in (("cd_points_inside", 11), ("cd_signed_distance", 13), ("cd_column_tri_points", 9)):
        assert name in mi355cd.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert callable(mi355cd.CollisionDetector.points_inside) and callable(mi355cd.CollisionDetector.signed_distance)
    assert callable(mi355cd.column_tri_points) and mi355cd.CD_INSIDE_PARITY == 1


def test_argument_errors_write_nothing_without_a_device():
    lib = mi355cd.load_library()
    pts = (C.c_double * 3)(0.25, 0.25, 0.25)
    inside = (C.c_uint8 * 1)(7)
    cnt = [(C.c_uint32 * 1)(7), (C.c_uint32 * 1)(7), (C.c_int32 * 1)(7), (C.c_int32 * 1)(7)]
    info = mi355cd.CdInsideInfo(5, 5, 5)
    sd = (C.c_double * 1)(-7.0)
    face, ids = (C.c_uint32 * 1)(7), (C.c_uint32 * 1)(7)
    closest, uv = (C.c_double * 3)(-7.0, -7.0, -7.0), (C.c_double * 2)(-7.0, -7.0)
    feature = (C.c_uint8 * 1)(7)
    pinfo = mi355cd.CdPointInfo(5, 5, 5)
    for axis, flags in ((2, 0), (3, 0), (-1, 0), (2, 2), (0, mi355cd.CD_INSIDE_PARITY)):      # a NULL context, whatever else is passed
        assert lib.cd_points_inside(None, pts, 1, axis, flags, inside, *cnt, C.byref(info)) == mi355cd.CD_ERR_ARG
        assert lib.cd_signed_distance(None, pts, 1, axis, flags, sd, face, ids, closest, uv, feature, inside, C.byref(pinfo)) == mi355cd.CD_ERR_ARG
    assert inside[0] == 7 and [c[0] for c in cnt] == [7, 7, 7, 7]                             # nothing is written
    assert (info.n_inside, info.node_visits, info.tri_tests) == (5, 5, 5)
    assert sd[0] == -7.0 and face[0] == 7 and ids[0] == 7 and list(closest) == [-7.0] * 3 and list(uv) == [-7.0] * 2 and feature[0] == 7
    assert (pinfo.n_found, pinfo.node_visits, pinfo.tri_tests) == (5, 5, 5)


def test_column_tri_points_argument_errors():
    lib = mi355cd.load_library()
    pts = (C.c_double * 3)(0.25, 0.25, 0.25)
    tri = (C.c_double * 9)(*([0.0] * 9))
    cover = (C.c_int8 * 1)(7)
    assert lib.cd_column_tri_points(pts, tri, 1, 3, cover, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_column_tri_points(pts, tri, 1, -1, cover, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_column_tri_points(None, tri, 1, 2, cover, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_column_tri_points(pts, tri, 1, 2, None, None, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_column_tri_points(pts, tri, 0, 2, cover, None, None, None, None) == mi355cd.CD_OK
    assert cover[0] == 7
