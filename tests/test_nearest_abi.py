"""cd_nearest_between's C-ABI surface, without a GPU: the symbol is exported and bound, its argument errors need no device, and the
info record has the header's layout."""
import ctypes as C

import mi355cd


def test_symbol_is_exported_and_bound():
    assert "cd_nearest_between" in mi355cd.EXPORTS
    lib = mi355cd.load_library()
    assert lib.cd_nearest_between.restype is C.c_int
    assert mi355cd.CD_NEAREST_MIN == 1 and mi355cd.NEAREST_NONE == 0xFFFFFFFF
    assert mi355cd.Nearest._fields == ("faces", "ids", "dist", "witness", "info")


def test_null_contexts_are_an_argument_error_without_a_device():
    lib = mi355cd.load_library()
    faces = (C.c_uint32 * 2)(7, 7)
    info = mi355cd.CdNearestInfo(5, 5, 5)
    for flags in (0, mi355cd.CD_NEAREST_MIN, 2):
        assert lib.cd_nearest_between(None, None, 1.0, flags, faces, None, None, None, C.byref(info)) == mi355cd.CD_ERR_ARG
    assert list(faces) == [7, 7] and (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)      # nothing is written


def test_info_layout():
    assert C.sizeof(mi355cd.CdNearestInfo) == 24
    assert [f[0] for f in mi355cd.CdNearestInfo._fields_] == ["n_found", "node_visits", "tri_tests"]
