"""The C-ABI surface of cd_segments_within, cd_segments_closest and cd_seg_tri_points, without a GPU: the symbols are declared,
exported and bound, the structures have the header's member order, and every argument error that is decided before a device is
touched returns CD_ERR_ARG and writes nothing."""
import ctypes as C
import os
import re

import numpy as np

import mi355cd

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mi355cd.h")
ERR = mi355cd.CD_ERR_ARG


def test_symbols_are_declared_exported_and_bound():
    lib = mi355cd.load_library()
    text = open(HEADER).read()
    for name, nargs in (("cd_segments_within", 8), ("cd_segments_closest", 7), ("cd_seg_tri_points", 12)):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in mi355cd.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert callable(mi355cd.CollisionDetector.segments_within) and callable(mi355cd.CollisionDetector.segments_closest)
    assert callable(mi355cd.seg_tri_points) and callable(mi355cd.pack_segments)
    assert re.search(r"enum \{ CD_SEGMENT_ANY = 1 \};", text) and mi355cd.CD_SEGMENT_ANY == 1 and mi355cd.SEGMENT_NONE == 0xFFFFFFFF


def _members(text, name):
    body = re.search(r"typedef struct %s \{([^}]*)\} %s;" % (name, name), text).group(1)
    return [m for decl in body.split(";") for m in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split(" ", 1)[1] if decl.strip() else "")]


def test_struct_member_order_is_the_headers():
    text = open(HEADER).read()
    vp = C.sizeof(C.c_void_p)
    rows = [n for n, _ in mi355cd.CdSegmentRows._fields_]
    assert rows == ["ids", "dist", "s", "on_seg", "on_tri", "uv", "feature", "end", "cross", "side"] == _members(text, "cd_segment_rows")
    assert [getattr(mi355cd.CdSegmentRows, n).offset for n in rows] == [k * vp for k in range(10)] and C.sizeof(mi355cd.CdSegmentRows) == 10 * vp
    info = [n for n, _ in mi355cd.CdSegmentInfo._fields_]
    assert info == ["n_found", "node_visits", "tri_tests"] == _members(text, "cd_segment_info")
    assert [getattr(mi355cd.CdSegmentInfo, n).offset for n in info] == [0, 8, 16] and C.sizeof(mi355cd.CdSegmentInfo) == 24
    s = mi355cd.pack_segments([[0.0, 1.0, 2.0]], [[3.0, 4.0, 5.0]], 6.0)
    assert s.shape == (1, 7) and s.tolist() == [[0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]              # (a, b, r)


class _Out:
    """Sentinel-filled outputs of one row."""

    def __init__(self):
        self.rows = (C.c_uint32 * 2)(7, 7)
        self.face = (C.c_uint32 * 1)(7)
        self.arrays = [np.full(k, 7, dtype=dt) for k, dt in ((1, np.uint32), (1, np.float64), (1, np.float64), (3, np.float64), (3, np.float64), (2, np.float64),
                                                            (1, np.uint8), (1, np.uint8), (1, np.uint8), (1, np.uint8))]
        self.out = mi355cd.CdSegmentRows(*(a.ctypes.data for a in self.arrays))
        self.n_rows, self.n_tested = C.c_uint64(7), C.c_uint64(7)
        self.info = mi355cd.CdSegmentInfo(5, 5, 5)

    def untouched(self):
        return (list(self.rows) == [7, 7] and self.face[0] == 7 and all((a == 7).all() for a in self.arrays) and self.n_rows.value == 7 and
                self.n_tested.value == 7 and (self.info.n_found, self.info.node_visits, self.info.tri_tests) == (5, 5, 5))


def test_argument_errors_write_nothing_without_a_device():
    """Everything decided before the context is looked into: a NULL context with any other arguments.  (A real context needs a
    device; tests/test_segments_gpu.py repeats the item checks on one.)"""
    lib = mi355cd.load_library()
    seg = (C.c_double * 7)(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5)
    o = _Out()
    assert lib.cd_segments_within(None, seg, 1, o.rows, 1, C.byref(o.n_rows), C.byref(o.n_tested), C.byref(o.out)) == ERR
    assert lib.cd_segments_within(None, None, 0, None, 0, None, None, None) == ERR
    assert lib.cd_segments_closest(None, seg, 1, 0, o.face, C.byref(o.out), C.byref(o.info)) == ERR
    assert lib.cd_segments_closest(None, seg, 1, mi355cd.CD_SEGMENT_ANY, o.face, None, C.byref(o.info)) == ERR
    assert o.untouched()


def test_argument_errors_with_a_context_that_has_no_tree():
    """The rules on n, the pointers, the flags and the items come before the context is looked into, so a zeroed block stands in for a
    context here (a real one needs a device; tests/test_segments_gpu.py repeats the checks on one).  If a rule let a call through,
    the call would read the block's stage -- 0, a context with no tree -- and answer CD_ERR_ORDER: the well-formed call below does."""
    lib = mi355cd.load_library()
    block = C.create_string_buffer(1 << 20)
    ctx = C.cast(block, C.c_void_p)
    seg = (C.c_double * 7)(0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5)
    o = _Out()
    within = lambda items, n, rows, cap, n_rows: lib.cd_segments_within(ctx, items, n, rows, cap, n_rows, C.byref(o.n_tested), C.byref(o.out))
    closest = lambda items, n, flags, face, out: lib.cd_segments_closest(ctx, items, n, flags, face, out, C.byref(o.info))
    assert within(seg, 1, o.rows, 1, C.byref(o.n_rows)) == mi355cd.CD_ERR_ORDER and o.untouched()                        # well-formed: no tree
    assert closest(seg, 1, 0, o.face, C.byref(o.out)) == mi355cd.CD_ERR_ORDER and o.untouched()
    for at, bad in ((0, float("nan")), (2, float("inf")), (4, float("-inf")), (6, float("nan")), (6, -1.0), (6, float("-inf"))):
        x = (C.c_double * 14)(*seg, *seg)
        x[7 + at] = bad                                                    # the LAST item
        assert within(x, 2, o.rows, 1, C.byref(o.n_rows)) == ERR and o.untouched(), (at, bad)
        assert closest(x, 2, 0, o.face, C.byref(o.out)) == ERR and o.untouched(), (at, bad)
        assert closest(x, 2, mi355cd.CD_SEGMENT_ANY, o.face, None) == ERR and o.untouched(), (at, bad)
    assert within(seg, 1 << 32, o.rows, 1, C.byref(o.n_rows)) == ERR                                                     # (the items are not read)
    assert within(seg, 1, o.rows, 1, None) == ERR                                                                        # NULL n_rows
    assert within(None, 1, o.rows, 1, C.byref(o.n_rows)) == ERR                                                          # NULL items with n > 0
    assert within(seg, 1, None, 1, C.byref(o.n_rows)) == ERR                                                             # NULL rows with cap_rows > 0
    assert closest(seg, 1 << 32, 0, o.face, None) == ERR
    assert closest(seg, 1, 2, o.face, None) == ERR and closest(seg, 1, -1, o.face, None) == ERR                          # bad flags
    assert closest(seg, 1, mi355cd.CD_SEGMENT_ANY, o.face, C.byref(o.out)) == ERR                                        # out given with CD_SEGMENT_ANY
    assert closest(None, 1, 0, o.face, None) == ERR and closest(seg, 1, 0, None, None) == ERR                            # NULL items, NULL face
    assert o.untouched()
    inf = (C.c_double * 7)(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, float("inf"))                                                   # r = +inf and a == b are values
    assert within(inf, 1, o.rows, 1, C.byref(o.n_rows)) == mi355cd.CD_ERR_ORDER and o.untouched()


def test_seg_tri_points_argument_errors():
    lib = mi355cd.load_library()
    seg = (C.c_double * 6)(0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    tri = (C.c_double * 9)(*([0.5] * 9))
    dist, s = (C.c_double * 1)(7.0), (C.c_double * 1)(7.0)
    rest = [None] * 7
    assert lib.cd_seg_tri_points(None, tri, 1, dist, s, *rest) == ERR
    assert lib.cd_seg_tri_points(seg, None, 1, dist, s, *rest) == ERR
    assert lib.cd_seg_tri_points(seg, tri, 1, None, s, *rest) == ERR
    assert lib.cd_seg_tri_points(seg, tri, 0, dist, s, *rest) == mi355cd.CD_OK
    assert lib.cd_seg_tri_points(None, None, 0, None, None, *rest) == mi355cd.CD_OK
    assert dist[0] == 7.0 and s[0] == 7.0
