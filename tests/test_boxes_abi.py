"""The C-ABI surface of cd_boxes_overlap_all, cd_boxes_count and cd_box_tri_points, without a GPU: the symbols are exported and
bound, the structures have the header's layout, and their argument errors need no device."""
import ctypes as C

import mi355cd


def test_symbols_are_exported_and_bound():
    lib = mi355cd.load_library()
    for name, nargs in (("cd_boxes_overlap_all", 8), ("cd_boxes_count", 7), ("cd_box_tri_points", 6)):
        assert name in mi355cd.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, name
    assert callable(mi355cd.CollisionDetector.boxes_overlap_all) and callable(mi355cd.CollisionDetector.boxes_count)
    assert callable(mi355cd.box_tri_points) and mi355cd.CD_BOX_ANY == 1


def test_struct_layouts():
    assert C.sizeof(mi355cd.CdBoxInfo) == 24
    assert [(n, getattr(mi355cd.CdBoxInfo, n).offset) for n, _ in mi355cd.CdBoxInfo._fields_] == [("n_found", 0), ("node_visits", 8), ("tri_tests", 16)]
    assert C.sizeof(mi355cd.CdBoxRows) == 2 * C.sizeof(C.c_void_p)
    assert [(n, getattr(mi355cd.CdBoxRows, n).offset) for n, _ in mi355cd.CdBoxRows._fields_] == [("ids", 0), ("inside", C.sizeof(C.c_void_p))]
    b = mi355cd.pack_boxes([[0.0, 1.0, 2.0]], [[3.0, 4.0, 5.0]])
    assert b.shape == (1, 6) and b.tolist() == [[0.0, 3.0, 1.0, 4.0, 2.0, 5.0]]                 # {x1, x2, y1, y2, z1, z2}, cd_root_box's layout


def test_argument_errors_write_nothing_without_a_device():
    lib = mi355cd.load_library()
    box = (C.c_double * 6)(0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    rows = (C.c_uint32 * 2)(7, 7)
    ids, inside = (C.c_uint32 * 1)(7), (C.c_uint8 * 1)(7)
    out = mi355cd.CdBoxRows(C.addressof(ids), C.addressof(inside))
    n_rows, n_tested = C.c_uint64(7), C.c_uint64(7)
    count, n_inside = (C.c_uint32 * 1)(7), (C.c_uint32 * 1)(7)
    info = mi355cd.CdBoxInfo(5, 5, 5)
    assert lib.cd_boxes_overlap_all(None, box, 1, rows, 1, C.byref(n_rows), C.byref(n_tested), C.byref(out)) == mi355cd.CD_ERR_ARG
    for flags, nin in ((0, n_inside), (mi355cd.CD_BOX_ANY, None), (2, None), (-1, None), (mi355cd.CD_BOX_ANY, n_inside)):   # a NULL context, whatever else is passed
        assert lib.cd_boxes_count(None, box, 1, flags, count, nin, C.byref(info)) == mi355cd.CD_ERR_ARG
    assert list(rows) == [7, 7] and ids[0] == 7 and inside[0] == 7 and n_rows.value == 7 and n_tested.value == 7   # nothing is written
    assert count[0] == 7 and n_inside[0] == 7 and (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)


def test_box_tri_points_argument_errors():
    lib = mi355cd.load_library()
    box = (C.c_double * 6)(0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
    tri = (C.c_double * 9)(*([0.5] * 9))
    hit, inside, code = (C.c_uint8 * 1)(7), (C.c_uint8 * 1)(7), (C.c_uint8 * 1)(7)
    assert lib.cd_box_tri_points(None, tri, 1, hit, inside, code) == mi355cd.CD_ERR_ARG
    assert lib.cd_box_tri_points(box, None, 1, hit, inside, code) == mi355cd.CD_ERR_ARG
    assert lib.cd_box_tri_points(box, tri, 1, None, inside, code) == mi355cd.CD_ERR_ARG
    assert lib.cd_box_tri_points(box, tri, 0, hit, inside, code) == mi355cd.CD_OK
    assert lib.cd_box_tri_points(None, None, 0, None, None, None) == mi355cd.CD_OK
    assert hit[0] == 7 and inside[0] == 7 and code[0] == 7
