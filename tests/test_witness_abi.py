"""The witness entry points' argument errors that need no device (the pattern of tests/test_abi.py)."""
import ctypes as C

import numpy as np

import mi355cd


def test_witness_argument_errors_do_not_need_a_device():
    lib = mi355cd.load_library()
    faces = np.zeros((4, 2), dtype=np.uint32)
    w = mi355cd.CdWitnessOut(faces.ctypes.data, None, None, None)
    n = C.c_uint64(0)
    pairs = np.zeros((4, 2), dtype=np.uint32)
    for wp in (None, C.byref(w)):
        assert lib.cd_find_proximity_witness(None, 0.1, pairs.ctypes.data, None, 4, C.byref(n), None, wp) == mi355cd.CD_ERR_ARG
        assert lib.cd_find_ccd_witness(None, None, 0.1, pairs.ctypes.data, None, None, 4, C.byref(n), None, wp) == mi355cd.CD_ERR_ARG
        assert lib.cd_find_proximity_between_witness(None, None, 0.1, pairs.ctypes.data, None, 4, C.byref(n), None, wp) == mi355cd.CD_ERR_ARG
        assert lib.cd_find_ccd_between_witness(None, None, None, None, 0.1, pairs.ctypes.data, None, None, 4, C.byref(n), None, wp) == mi355cd.CD_ERR_ARG
    assert lib.cd_tri_witness_points(None, 4, None, None, None, None) == mi355cd.CD_ERR_ARG
    tri = np.zeros((4, 18))
    assert lib.cd_tri_witness_points(tri.ctypes.data, 4, None, None, None, None) == mi355cd.CD_ERR_ARG     # dist is not optional
    d = np.zeros(4)
    assert lib.cd_tri_witness_points(tri.ctypes.data, 0, d.ctypes.data, None, None, None) == mi355cd.CD_OK  # n = 0: nothing to do
    assert C.sizeof(mi355cd.CdWitnessOut) == 4 * C.sizeof(C.c_void_p)
    assert not faces.any()
