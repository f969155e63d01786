"""cd_nearest_self's C-ABI surface, without a GPU: the symbol is exported and bound, and its argument errors need no device."""
import ctypes as C

import mi355cd


def test_symbol_is_exported_and_bound():
    assert "cd_nearest_self" in mi355cd.EXPORTS
    lib = mi355cd.load_library()
    assert lib.cd_nearest_self.restype is C.c_int
    assert len(lib.cd_nearest_self.argtypes) == 8
    assert callable(mi355cd.CollisionDetector.nearest_self)


def test_null_context_is_an_argument_error_without_a_device():
    lib = mi355cd.load_library()
    faces = (C.c_uint32 * 2)(7, 7)
    ids = (C.c_uint32 * 2)(7, 7)
    dist = (C.c_double * 1)(-7.0)
    info = mi355cd.CdNearestInfo(5, 5, 5)
    for flags in (0, mi355cd.CD_NEAREST_MIN, 2):
        assert lib.cd_nearest_self(None, 1.0, flags, faces, ids, dist, None, C.byref(info)) == mi355cd.CD_ERR_ARG
    assert list(faces) == [7, 7] and list(ids) == [7, 7] and dist[0] == -7.0      # nothing is written
    assert (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)
