"""The C-ABI surface of the all-results item queries (cd_points_within, cd_cast_rays_all) that needs no GPU: the layout of the row
structs, the exported names, and the argument errors that are decided before a device is touched."""
import ctypes as C
import os
import re

import numpy as np

import mi355cd
from conftest import ROOT


def test_row_structs_are_plain_pointer_records():
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(mi355cd.CdPointRows) == 6 * p and C.sizeof(mi355cd.CdRayRows) == 4 * p
    for k, name in enumerate(("ids", "dist", "closest", "uv", "feature", "side")):
        assert getattr(mi355cd.CdPointRows, name).offset == k * p, name
    for k, name in enumerate(("ids", "t", "uv", "side")):
        assert getattr(mi355cd.CdRayRows, name).offset == k * p, name
    text = open(os.path.join(ROOT, "include", "mi355cd.h")).read()              # the header's member order is the bindings'
    for struct, cls in (("cd_point_rows", mi355cd.CdPointRows), ("cd_ray_rows", mi355cd.CdRayRows)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
        assert re.findall(r"\*(\w+);", body) == [f[0] for f in cls._fields_], struct


def test_names_are_exported_and_bound():
    lib = mi355cd.load_library()
    for name in ("cd_points_within", "cd_cast_rays_all"):
        assert name in mi355cd.EXPORTS and getattr(lib, name).restype is C.c_int
    assert hasattr(mi355cd.CollisionDetector, "points_within") and hasattr(mi355cd.CollisionDetector, "cast_rays_all")
    text = open(os.path.join(ROOT, "gpu-computing-course_amd", "csrc", "cd_within.h")).read()
    first = re.search(r"constexpr unsigned long long WITHIN_SHARD_FIRST = 1ull << (\d+);", text)
    assert first and 1 << int(first.group(1)) == mi355cd.WITHIN_SHARD_FIRST     # the Python mirror of the named initial capacity


def test_argument_errors_do_not_need_a_device():
    lib = mi355cd.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    pts, rays = np.zeros((4, 4)), np.ones((4, 7))
    rows = np.full((8, 2), 7, dtype=np.uint32)
    n, tested = C.c_uint64(77), C.c_uint64(77)
    prow, rrow = mi355cd.CdPointRows(), mi355cd.CdRayRows()
    assert lib.cd_points_within(None, vp(pts), 4, vp(rows), 8, C.byref(n), C.byref(tested), C.byref(prow)) == mi355cd.CD_ERR_ARG
    assert lib.cd_cast_rays_all(None, vp(rays), 4, vp(rows), 8, C.byref(n), C.byref(tested), C.byref(rrow)) == mi355cd.CD_ERR_ARG
    assert lib.cd_points_within(None, None, 0, None, 0, None, None, None) == mi355cd.CD_ERR_ARG
    assert lib.cd_cast_rays_all(None, None, 0, None, 0, None, None, None) == mi355cd.CD_ERR_ARG
    assert n.value == 77 and tested.value == 77 and (rows == 7).all()          # nothing is written
