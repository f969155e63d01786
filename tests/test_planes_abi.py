"""The C-ABI surface of cd_planes_cut_all, cd_planes_count and cd_plane_tri_points, without a GPU: the symbols are exported and
bound, the structures and constants have the header's layout and values, and their argument errors need no device."""
import ctypes as C
import os
import re

import mi355cd
import plane_ref as plr

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mi355cd.h")


def test_symbols_are_exported_and_bound():
    lib = mi355cd.load_library()
    for name, nargs in (("cd_planes_cut_all", 8), ("cd_planes_count", 7), ("cd_plane_tri_points", 8)):
        assert name in mi355cd.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert callable(mi355cd.CollisionDetector.planes_cut_all) and callable(mi355cd.CollisionDetector.planes_count)
    assert callable(mi355cd.plane_tri_points) and callable(mi355cd.pack_planes)


def test_header_declares_the_calls_and_the_constants_agree():
    text = open(HEADER).read()
    for decl in (r"int cd_planes_cut_all\(cd_ctx \*ctx, const double \*planes /\* n x 4 \*/, uint64_t n, uint32_t \*rows, uint64_t cap_rows,\s+uint64_t \*n_rows, uint64_t \*n_tested, const cd_plane_rows \*out\);",
                 r"int cd_planes_count\(cd_ctx \*ctx, const double \*planes /\* n x 4 \*/, uint64_t n, uint32_t \*n_cut, uint32_t \*n_below,\s+uint32_t \*n_above, cd_plane_info \*info\);",
                 r"int cd_plane_tri_points\(const double \*planes, const double \*tri, uint64_t n, uint8_t \*cls, double \*seg, uint8_t \*edge,\s+double \*t, uint8_t \*on\);",
                 r"typedef struct cd_plane_rows \{ uint32_t \*ids; double \*seg; uint8_t \*edge; double \*t; uint8_t \*on; \} cd_plane_rows;",
                 r"typedef struct cd_plane_info \{ uint64_t n_found, node_visits, tri_tests; \} cd_plane_info;",
                 r"enum \{ CD_PLANE_ABOVE = 0, CD_PLANE_BELOW = 1, CD_PLANE_CUT = 2 \};"):
        assert re.search(decl, text), decl
    slab = int(re.search(r"#define CD_PLANE_SLAB (\d+)", text).group(1))
    assert slab == mi355cd.CD_PLANE_SLAB == plr.L and slab >= 1 and slab & (slab - 1) == 0       # a power of two
    assert (mi355cd.CD_PLANE_ABOVE, mi355cd.CD_PLANE_BELOW, mi355cd.CD_PLANE_CUT) == (plr.ABOVE, plr.BELOW, plr.CUT) == (0, 1, 2)


def test_struct_layouts():
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(mi355cd.CdPlaneInfo) == 24
    assert [(n, getattr(mi355cd.CdPlaneInfo, n).offset) for n, _ in mi355cd.CdPlaneInfo._fields_] == [("n_found", 0), ("node_visits", 8), ("tri_tests", 16)]
    assert C.sizeof(mi355cd.CdPlaneRows) == 5 * vp
    assert [(n, getattr(mi355cd.CdPlaneRows, n).offset) for n, _ in mi355cd.CdPlaneRows._fields_] == [("ids", 0), ("seg", vp), ("edge", 2 * vp), ("t", 3 * vp), ("on", 4 * vp)]
    p = mi355cd.pack_planes([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]], [6.0, 7.0])
    assert p.shape == (2, 4) and p.tolist() == [[0.0, 1.0, 2.0, 6.0], [3.0, 4.0, 5.0, 7.0]]       # {nx, ny, nz, d}


def test_argument_errors_write_nothing_without_a_device():
    lib = mi355cd.load_library()
    plane = (C.c_double * 4)(0.0, 0.0, 1.0, 0.5)
    rows = (C.c_uint32 * 2)(7, 7)
    ids, on = (C.c_uint32 * 1)(7), (C.c_uint8 * 1)(7)
    seg, edge, t = (C.c_double * 6)(*([7.0] * 6)), (C.c_uint8 * 2)(7, 7), (C.c_double * 2)(7.0, 7.0)
    out = mi355cd.CdPlaneRows(C.addressof(ids), C.addressof(seg), C.addressof(edge), C.addressof(t), C.addressof(on))
    n_rows, n_tested = C.c_uint64(7), C.c_uint64(7)
    counts = [(C.c_uint32 * 1)(7) for _ in range(3)]
    info = mi355cd.CdPlaneInfo(5, 5, 5)
    assert lib.cd_planes_cut_all(None, plane, 1, rows, 1, C.byref(n_rows), C.byref(n_tested), C.byref(out)) == mi355cd.CD_ERR_ARG   # a NULL context, whatever else is passed
    assert lib.cd_planes_count(None, plane, 1, *counts, C.byref(info)) == mi355cd.CD_ERR_ARG
    assert lib.cd_planes_count(None, plane, 1, counts[0], None, None, None) == mi355cd.CD_ERR_ARG
    assert list(rows) == [7, 7] and ids[0] == 7 and on[0] == 7 and list(seg) == [7.0] * 6 and list(edge) == [7, 7] and list(t) == [7.0, 7.0]
    assert n_rows.value == 7 and n_tested.value == 7                                               # nothing is written
    assert all(c[0] == 7 for c in counts) and (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)


def test_plane_tri_points_argument_errors():
    lib = mi355cd.load_library()
    plane = (C.c_double * 4)(0.0, 0.0, 1.0, 0.5)
    tri = (C.c_double * 9)(*([0.5] * 9))
    cls, on = (C.c_uint8 * 1)(7), (C.c_uint8 * 1)(7)
    assert lib.cd_plane_tri_points(None, tri, 1, cls, None, None, None, on) == mi355cd.CD_ERR_ARG
    assert lib.cd_plane_tri_points(plane, None, 1, cls, None, None, None, on) == mi355cd.CD_ERR_ARG
    assert lib.cd_plane_tri_points(plane, tri, 1, None, None, None, None, on) == mi355cd.CD_ERR_ARG
    assert lib.cd_plane_tri_points(plane, tri, 0, cls, None, None, None, on) == mi355cd.CD_OK
    assert lib.cd_plane_tri_points(None, None, 0, None, None, None, None, None) == mi355cd.CD_OK
    assert cls[0] == 7 and on[0] == 7
