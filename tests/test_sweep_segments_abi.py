"""The swept-segment queries' C surface, without a GPU: cd_sweep_segment_rows against the header, the three names exported and bound,
and the argument errors that are decided before a device is touched -- which write nothing."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

import mi355cd
from conftest import ROOT

NAMES = ("cd_sweep_segments_all", "cd_sweep_segments", "cd_seg_advance_points")
MEMBERS = ["ids", "toi", "dist", "s", "on_seg", "on_tri", "uv", "feature", "end", "cross", "side"]
SENTINEL = 7


def _header():
    return open(os.path.join(ROOT, "include", "mi355cd.h")).read()


def test_cd_sweep_segment_rows_member_order_matches_the_header():
    m = re.search(r"typedef struct cd_sweep_segment_rows \{(.*?)\} cd_sweep_segment_rows;", _header(), flags=re.S)
    assert m
    members = [re.sub(r".*\*", "", part).strip() for part in m.group(1).split(";") if part.strip()]
    assert members == [name for name, _ in mi355cd.CdSweepSegmentRows._fields_] == MEMBERS
    assert all(t is C.c_void_p for _, t in mi355cd.CdSweepSegmentRows._fields_) and C.sizeof(mi355cd.CdSweepSegmentRows) == 11 * C.sizeof(C.c_void_p)


def test_the_three_names_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", mi355cd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = mi355cd.load_library()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in mi355cd.EXPORTS and re.search(r" T %s$" % name, out, flags=re.M), name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes, name
    assert len(lib.cd_sweep_segments_all.argtypes) == 10 and len(lib.cd_sweep_segments.argtypes) == 9 and len(lib.cd_seg_advance_points.argtypes) == 14
    for name in ("pack_swept_segments", "seg_advance_points", "CdSweepSegmentRows"):
        assert hasattr(mi355cd, name), name
    for name in ("sweep_segments_all", "sweep_segments"):
        assert callable(getattr(mi355cd.CollisionDetector, name)), name


def test_pack_swept_segments_layout():
    pts = [10 * k + np.arange(6.0).reshape(2, 3) for k in range(4)]
    it = mi355cd.pack_swept_segments(*pts, [0.5, 0.25])
    assert it.dtype == np.float64 and it.flags.c_contiguous and it.shape == (2, 13)
    for k in range(4):
        assert np.array_equal(it[:, 3 * k:3 * k + 3], pts[k])
    assert it[:, 12].tolist() == [0.5, 0.25]
    assert mi355cd.pack_swept_segments(*pts, 0.125)[:, 12].tolist() == [0.125, 0.125]


class _Out:
    """toi, seg_tri's values, evals: the outputs of cd_seg_advance_points in its order, filled with the sentinel"""
    SHAPES = (("toi", np.float64, ()), ("dist", np.float64, ()), ("s", np.float64, ()), ("on_seg", np.float64, (3,)), ("on_tri", np.float64, (3,)),
              ("uv", np.float64, (2,)), ("feature", np.uint8, ()), ("end", np.uint8, ()), ("cross", np.uint8, ()), ("side", np.uint8, ()), ("evals", np.uint32, ()))

    def __init__(self, n):
        self.a = [np.full((n,) + s, SENTINEL, dtype=dt) for _, dt, s in self.SHAPES]

    def ptrs(self):
        return [x.ctypes.data_as(C.c_void_p) for x in self.a]

    def untouched(self):
        return all((x == SENTINEL).all() for x in self.a)


BAD_ITEMS = [(12, 0.0), (12, -1.0), (12, np.nan), (12, np.inf), (12, -np.inf)] + [(c, v) for c in range(12) for v in (np.nan, np.inf, -np.inf)]


def test_argument_errors_before_a_device_write_nothing():
    lib = mi355cd.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    items = np.zeros((4, 13)); items[:, 12] = 0.1
    tri = np.zeros((4, 18))
    o = _Out(4)
    assert lib.cd_seg_advance_points(None, vp(tri), 4, *o.ptrs()) == mi355cd.CD_ERR_ARG and o.untouched()
    assert lib.cd_seg_advance_points(vp(items), None, 4, *o.ptrs()) == mi355cd.CD_ERR_ARG and o.untouched()
    assert lib.cd_seg_advance_points(vp(items), vp(tri), 4, None, *o.ptrs()[1:]) == mi355cd.CD_ERR_ARG and o.untouched()   # toi is required
    for col, val in BAD_ITEMS:
        bad = items.copy(); bad[3, col] = val                              # the LAST item
        assert lib.cd_seg_advance_points(vp(bad), vp(tri), 4, *o.ptrs()) == mi355cd.CD_ERR_ARG and o.untouched(), (col, val)
    assert lib.cd_seg_advance_points(vp(items), vp(tri), 0, *o.ptrs()) == mi355cd.CD_OK and o.untouched()                 # n = 0

    rows = np.full((8, 2), SENTINEL, dtype=np.uint32)
    n, info = C.c_uint64(SENTINEL), mi355cd.CdCcdInfo(SENTINEL, SENTINEL, SENTINEL, SENTINEL)
    vals = _Out(8)
    ids = np.full(8, SENTINEL, dtype=np.uint32)
    out = mi355cd.CdSweepSegmentRows(*(x.ctypes.data for x in (ids, *vals.a[:10])))
    face = np.full(4, SENTINEL, dtype=np.uint32)
    pinfo = mi355cd.CdPointInfo(SENTINEL, SENTINEL, SENTINEL)
    clean = lambda: (rows == SENTINEL).all() and n.value == SENTINEL and info.n_tested == SENTINEL and vals.untouched() and (ids == SENTINEL).all() and \
        (face == SENTINEL).all() and pinfo.n_found == SENTINEL
    assert lib.cd_sweep_segments_all(None, None, vp(items), 4, None, vp(rows), 8, C.byref(n), C.byref(out), C.byref(info)) == mi355cd.CD_ERR_ARG   # no context
    assert lib.cd_sweep_segments(None, None, vp(items), 4, None, 0, vp(face), C.byref(out), C.byref(pinfo)) == mi355cd.CD_ERR_ARG
    assert clean()
    # the errors of the context calls themselves (each is CD_ERR_ARG on its own; tests/test_sweep_segments_gpu.py repeats them on a live context)
    for col, val in BAD_ITEMS:
        bad = items.copy(); bad[3, col] = val
        assert lib.cd_sweep_segments_all(None, None, vp(bad), 4, None, vp(rows), 8, C.byref(n), C.byref(out), C.byref(info)) == mi355cd.CD_ERR_ARG
        assert lib.cd_sweep_segments(None, None, vp(bad), 4, None, 0, vp(face), C.byref(out), C.byref(pinfo)) == mi355cd.CD_ERR_ARG
    assert lib.cd_sweep_segments(None, None, vp(items), 4, None, 0, None, C.byref(out), C.byref(pinfo)) == mi355cd.CD_ERR_ARG          # NULL face
    assert lib.cd_sweep_segments(None, None, vp(items), 4, None, 1, vp(face), C.byref(out), C.byref(pinfo)) == mi355cd.CD_ERR_ARG      # flags
    assert lib.cd_sweep_segments(None, None, vp(items), 1 << 32, None, 0, vp(face), C.byref(out), C.byref(pinfo)) == mi355cd.CD_ERR_ARG   # n > 0xFFFFFFFF: the items are not read
    assert lib.cd_sweep_segments_all(None, None, vp(items), 1 << 32, None, vp(rows), 8, C.byref(n), C.byref(out), C.byref(info)) == mi355cd.CD_ERR_ARG
    assert lib.cd_sweep_segments_all(None, None, vp(items), 4, None, vp(rows), 8, None, C.byref(out), C.byref(info)) == mi355cd.CD_ERR_ARG   # NULL n_rows
    assert clean()


def test_argument_errors_with_a_context_that_has_no_tree():
    """The rules on n, the pointers, the flags and the items come before the context is looked into, so a zeroed block stands in for a
    context here (a real one needs a device; tests/test_sweep_segments_gpu.py repeats the checks on one).  If a rule let a call
    through, the call would read the block's stage -- 0, a context with no tree -- and answer CD_ERR_ORDER: the well-formed calls do."""
    lib = mi355cd.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    block = C.create_string_buffer(1 << 20)
    ctx = C.cast(block, C.c_void_p)
    items = np.zeros((4, 13)); items[:, 3] = 1.0; items[:, 12] = 0.1
    rows = np.full((8, 2), SENTINEL, dtype=np.uint32)
    n, info = C.c_uint64(SENTINEL), mi355cd.CdCcdInfo(SENTINEL, SENTINEL, SENTINEL, SENTINEL)
    vals = _Out(8)
    ids = np.full(8, SENTINEL, dtype=np.uint32)
    out = mi355cd.CdSweepSegmentRows(*(x.ctypes.data for x in (ids, *vals.a[:10])))
    face = np.full(4, SENTINEL, dtype=np.uint32)
    pinfo = mi355cd.CdPointInfo(SENTINEL, SENTINEL, SENTINEL)
    clean = lambda: (rows == SENTINEL).all() and n.value == SENTINEL and info.n_tested == SENTINEL and vals.untouched() and (ids == SENTINEL).all() and \
        (face == SENTINEL).all() and pinfo.n_found == SENTINEL
    rows_call = lambda it, count, r=rows, cap=8, nr=n: lib.cd_sweep_segments_all(ctx, None, None if it is None else vp(it), count, None, None if r is None else vp(r), cap,
                                                                                 None if nr is None else C.byref(nr), C.byref(out), C.byref(info))
    first_call = lambda it, count, flags=0, f=face: lib.cd_sweep_segments(ctx, None, None if it is None else vp(it), count, None, flags, None if f is None else vp(f),
                                                                          C.byref(out), C.byref(pinfo))
    ERR, ORDER = mi355cd.CD_ERR_ARG, mi355cd.CD_ERR_ORDER
    assert rows_call(items, 4) == ORDER and first_call(items, 4) == ORDER and clean()          # well-formed: no tree
    point = items.copy(); point[:, 3] = 0.0                                                   # a segment of zero length at both ends is a value
    assert rows_call(point, 4) == ORDER and first_call(point, 4) == ORDER and clean()
    for col, val in BAD_ITEMS:
        bad = items.copy(); bad[3, col] = val                                                 # the LAST item
        assert rows_call(bad, 4) == ERR and first_call(bad, 4) == ERR and clean(), (col, val)
    assert rows_call(items, 1 << 32) == ERR and first_call(items, 1 << 32) == ERR             # (the items are not read)
    assert rows_call(None, 4) == ERR and first_call(None, 4) == ERR                           # NULL items with n > 0
    assert rows_call(items, 4, nr=None) == ERR                                                # NULL n_rows
    assert rows_call(items, 4, r=None) == ERR                                                 # NULL rows with cap_rows > 0
    assert rows_call(items, 4, r=None, cap=0) == ORDER                                        # (the count-only form is well-formed)
    assert first_call(items, 4, f=None) == ERR                                                # NULL face
    assert first_call(items, 4, flags=1) == ERR and first_call(items, 4, flags=-1) == ERR     # flags other than 0
    assert clean()
