"""The swept-point queries' C surface, without a GPU: cd_sweep_rows against the header, the three names exported and bound, and the
argument errors that are decided before a device is touched -- which write nothing."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

import mi355cd
from conftest import ROOT

NAMES = ("cd_sweep_points_all", "cd_sweep_points", "cd_pt_advance_points")
SENTINEL = 7


def _header():
    return open(os.path.join(ROOT, "include", "mi355cd.h")).read()


def test_cd_sweep_rows_member_order_matches_the_header():
    m = re.search(r"typedef struct cd_sweep_rows \{(.*?)\} cd_sweep_rows;", _header(), flags=re.S)
    assert m
    members = [re.sub(r".*\*", "", part).strip() for part in m.group(1).split(";") if part.strip()]
    assert members == [name for name, _ in mi355cd.CdSweepRows._fields_] == ["ids", "toi", "dist", "closest", "uv", "feature", "side"]
    assert all(t is C.c_void_p for _, t in mi355cd.CdSweepRows._fields_) and C.sizeof(mi355cd.CdSweepRows) == 7 * C.sizeof(C.c_void_p)


def test_the_three_names_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", mi355cd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = mi355cd.load_library()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in mi355cd.EXPORTS and re.search(r" T %s$" % name, out, flags=re.M), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.cd_sweep_points_all.argtypes) == 10 and len(lib.cd_sweep_points.argtypes) == 15 and len(lib.cd_pt_advance_points.argtypes) == 10
    for name in ("pack_sweeps", "pt_advance_points", "CdSweepRows"):
        assert hasattr(mi355cd, name), name
    for name in ("sweep_points_all", "sweep_points"):
        assert callable(getattr(mi355cd.CollisionDetector, name)), name


def test_pack_sweeps_layout():
    p0, p1 = np.arange(6.0).reshape(2, 3), 10 + np.arange(6.0).reshape(2, 3)
    it = mi355cd.pack_sweeps(p0, p1, [0.5, 0.25])
    assert it.dtype == np.float64 and it.flags.c_contiguous and it.shape == (2, 7)
    assert np.array_equal(it[:, 0:3], p0) and np.array_equal(it[:, 3:6], p1) and it[:, 6].tolist() == [0.5, 0.25]
    assert mi355cd.pack_sweeps(p0, p1, 0.125)[:, 6].tolist() == [0.125, 0.125]


class _Out:
    def __init__(self, n):
        shapes = (("toi", np.float64, ()), ("dist", np.float64, ()), ("closest", np.float64, (3,)), ("uv", np.float64, (2,)), ("feature", np.uint8, ()),
                  ("side", np.uint8, ()), ("evals", np.uint32, ()))
        self.a = [np.full((n,) + s, SENTINEL, dtype=dt) for _, dt, s in shapes]

    def ptrs(self):
        return [x.ctypes.data_as(C.c_void_p) for x in self.a]

    def untouched(self):
        return all((x == SENTINEL).all() for x in self.a)


def test_argument_errors_before_a_device_write_nothing():
    lib = mi355cd.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    items = np.zeros((4, 7)); items[:, 6] = 0.1
    tri = np.zeros((4, 18))
    o = _Out(4)
    assert lib.cd_pt_advance_points(None, vp(tri), 4, *o.ptrs()) == mi355cd.CD_ERR_ARG and o.untouched()
    assert lib.cd_pt_advance_points(vp(items), None, 4, *o.ptrs()) == mi355cd.CD_ERR_ARG and o.untouched()
    assert lib.cd_pt_advance_points(vp(items), vp(tri), 4, None, *o.ptrs()[1:]) == mi355cd.CD_ERR_ARG and o.untouched()   # toi is required
    for col, val in ((6, 0.0), (6, -1.0), (6, np.nan), (6, np.inf), (0, np.nan), (2, np.inf), (3, -np.inf), (5, np.nan)):
        bad = items.copy(); bad[3, col] = val                              # the LAST item
        assert lib.cd_pt_advance_points(vp(bad), vp(tri), 4, *o.ptrs()) == mi355cd.CD_ERR_ARG and o.untouched(), (col, val)
    assert lib.cd_pt_advance_points(vp(items), vp(tri), 0, *o.ptrs()) == mi355cd.CD_OK and o.untouched()                 # n = 0

    rows = np.full((8, 2), SENTINEL, dtype=np.uint32)
    n, info = C.c_uint64(SENTINEL), mi355cd.CdCcdInfo(SENTINEL, SENTINEL, SENTINEL, SENTINEL)
    vals = _Out(8)
    out = mi355cd.CdSweepRows(*(x.ctypes.data for x in (np.full(8, SENTINEL, dtype=np.uint32), *vals.a[:6])))
    assert lib.cd_sweep_points_all(None, None, vp(items), 4, None, vp(rows), 8, C.byref(n), C.byref(out), C.byref(info)) == mi355cd.CD_ERR_ARG   # no context
    assert (rows == SENTINEL).all() and n.value == SENTINEL and info.n_tested == SENTINEL and vals.untouched()
    face = np.full(4, SENTINEL, dtype=np.uint32)
    pinfo = mi355cd.CdPointInfo(SENTINEL, SENTINEL, SENTINEL)
    assert lib.cd_sweep_points(None, None, vp(items), 4, None, 0, vp(face), None, None, None, None, None, None, None, C.byref(pinfo)) == mi355cd.CD_ERR_ARG
    assert (face == SENTINEL).all() and pinfo.n_found == SENTINEL
