"""The static tree's fp32 records (NodeRec32 halves, named by split), the query boxes (LeafBox32) and the cell table behind their
encoding, against a restatement computed off the device (records_ref.py, checked on the CPU by test_records_ref.py): bit for bit, on
every build path, on the meshes of records_inputs.py.  Until now the records were only compared device against device (the fused
build's bytes against the stage-wise build's): an error in enc_box32 / enc_leaf32 / amb_lookup / k_amb_insert common to both would
have passed.  The key order is compared first, so that a mismatch points at the right stage.

Who fills the query boxes: the default fused build does not store qbox[] (nothing on the half traversal's path reads it); asking
cd_debug_records for them fills them on request (k_fill_qbox through ensure_qbox, as for the readers of
test_readers_of_the_query_boxes_get_them_on_request).  With CD_DBG_STORE_QBOX the build's own k_build_block writes them, and the
stage-wise refit always does: the three writers are each compared here.

One context is alive at a time."""
import numpy as np
import pytest

import mi355_synth as synth
import mi355cd
import oracle
import records_inputs as ri
import records_ref as rr

pytestmark = pytest.mark.gpu

BUILDS = ["fused", "stagewise", "split_cross", "store_qbox", "staged"]
FUSED, STAGEWISE = "minmax", "rightmost"                        # records_ref.same_records: the sign of a zero bound with both signs below it, by build


def _read(cd):
    return cd.debug_records() + (cd.root_box(),)


def _check(cd, want, step, what, zeros, theorem=True):
    """Key order, then records / query boxes / root / root box against the restatement; then, up to BRUTE_MAX leaves, the theorem by brute
    force on what the DEVICE wrote (its fp32 leaf boxes and CERTAIN flags against the oracle's FP64 leaf boxes): a restatement with the
    kernel's own mistake would not hide a lost pair from that; it runs whether or not the comparison passed, and a failure reports both.  zeros: whose sign a zero bound of an internal child carries where the leaves
    under it hold both (records_ref.py) -- FUSED ("minmax") for every tree of the fused build, split cross and stored qbox included, STAGEWISE
    ("rightmost") for the stage-wise build and the staged entries.  Each build path is held to its own; `zeros` is the mesh that has such words."""
    n = want["n"]
    keys, perm = cd.export_keys()
    assert np.array_equal(keys, step["keys"]) and np.array_equal(perm, step["perm"]), f"{what}: the key order differs from the oracle's -- the sort, not the records"
    got = _read(cd)
    failed = []                                                                # both checks run: the second does not depend on the restatement
    try:
        rr.same_records(got, want, n, zeros=zeros)
    except AssertionError as e:
        failed.append(f"{what}: {e}")
    if theorem and n <= ri.BRUTE_MAX and got[2].shape == (n, 8):
        qb = got[2]
        l64 = want["leaf64"]
        try:
            rr.check_theorem(l64[:, 0::2], l64[:, 1::2], qb[:, 0:3].copy().view(np.float32), qb[:, 3:6].copy().view(np.float32), (qb[:, 6] & rr.LB_CERTAIN) != 0, what=f"{what} (device)")
        except AssertionError as e:
            failed.append(f"the theorem on the device's leaf boxes: {e}")
    assert not failed, "\n".join(failed)
    return got


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ri.MESHES)
def test_records_match_restatement(name, build):
    verts, vidx = ri.mesh(name)
    want, step = ri.want(name), ri.step(name)
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        if build == "staged":
            cd.morton_sort(); cd.build_hierarchy(); cd.refit_boxes()
            assert cd.debug_get(mi355cd.CD_DBG_GET_TREE_WAS_FUSED) == 0
            _check(cd, want, step, f"{name}, the staged entries", STAGEWISE)
            cd.build_tree()                                                    # ... and the fused entry over the tree they left
            assert cd.debug_get(mi355cd.CD_DBG_GET_TREE_WAS_FUSED) == 1
            _check(cd, want, step, f"{name}, build_tree after the staged entries", FUSED, theorem=False)
            return
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 1 if build == "stagewise" else 0)
        cd.debug_set(mi355cd.CD_DBG_SPLIT_CROSS, 1 if build == "split_cross" else 0)
        cd.debug_set(mi355cd.CD_DBG_STORE_QBOX, 1 if build == "store_qbox" else 0)
        cd.build_tree()
        assert cd.debug_get(mi355cd.CD_DBG_GET_TREE_WAS_FUSED) == (0 if build == "stagewise" else 1)     # the build that was asked for is the build that ran
        _check(cd, want, step, f"{name}, {build}", STAGEWISE if build == "stagewise" else FUSED)


def test_cell_table_modes():
    """CD_OPT_CELL_TABLE 1 -> 0 -> 1 on one context, rebuilt each time.  Off: every hi that is not an fp32 value is moved (checked on the
    device's bits directly, beside the restatement); the two modes differ in records and query boxes."""
    name = "cloth_double"
    verts, vidx = ri.mesh(name)
    step, on, off = ri.step(name), ri.want(name, "table"), ri.want(name, "off")
    m = on["n"] - 1
    assert not np.array_equal(on["qb"], off["qb"]) and not np.array_equal(on["rr"][:m], off["rr"][:m]) and not np.array_equal(on["rl"][:m], off["rl"][:m])
    hi64 = off["leaf64"][:, 1::2]
    inexact = ~rr.is_f32(hi64)
    assert inexact.mean() > 0.9 and np.array_equal(off["leaf"]["moved"], inexact) and on["leaf"]["moved"].sum() < inexact.sum()      # (restatement) off moves them all, the table does not
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        for value, want in ((1, on), (0, off), (1, on)):
            cd.set_option(mi355cd.CD_OPT_CELL_TABLE, value)
            cd.build_tree()
            got = _check(cd, want, step, f"{name}, CD_OPT_CELL_TABLE {value}", FUSED)
            if value == 0:
                assert np.array_equal(got[2][:, 3:6], rr.bits(np.where(inexact, rr.next_up(rr.rd32(hi64)), rr.rd32(hi64))))


def test_update_vertices_rebuilds_the_table():
    """The table is a function of the vertices alone: float mesh -> full doubles -> the same doubles with ONE vertex nudged inside its cell
    -> back to float, through cd_update_vertices on one context.  A column of the cloth shares one x, alone in its cell; the nudged vertex
    puts a second double there: the cell becomes ambiguous, and the hi of every box that ends at that column moves."""
    d, vidx = synth.cloth_pair(12, round_f32=False)
    f = np.ascontiguousarray(d.astype(np.float32).astype(np.float64))
    col = d[:, 0] == d[5 * 13, 0]                                              # column 5 of sheet A
    k = int(np.nonzero(col)[0][3])
    nudged = d.copy()
    nudged[k, 0] = np.nextafter(np.nextafter(d[k, 0], np.inf), np.inf)
    assert rr.cell(nudged[k, 0]) == rr.cell(d[k, 0]) and col.sum() == 13 and not rr.is_f32(d[k, 0])
    seq = [("float", f), ("double", d), ("nudged", nudged), ("float again", f)]
    wants = {}
    for what, v in seq[:3]:
        st = oracle.pipeline(v, vidx)
        wants[what] = (rr.expected_records(v, vidx, st), st)
    wants["float again"] = wants["float"]
    t_d, t_n = wants["double"][0]["table"], wants["nudged"][0]["table"]
    assert wants["float"][0]["table"].mode == "none" and t_d.mode == "table"
    assert not t_d.ambiguous(0, d[k, 0]) and t_n.ambiguous(0, d[k, 0])         # a cell ambiguous that was not
    assert wants["nudged"][0]["leaf"]["moved"][:, 0].sum() > wants["double"][0]["leaf"]["moved"][:, 0].sum()
    with mi355cd.CollisionDetector(f, vidx) as cd:
        cd.build_tree()
        _check(cd, *wants["float"], "float (as created)", FUSED)
        for what, v in seq[1:]:
            cd.update_vertices(v)
            cd.build_tree()
            _check(cd, *wants[what], f"after update_vertices: {what}", FUSED)


def test_auto_frame_changes_order_not_encoding():
    """CD_FRAME_AUTO: the oracle runs in the frame it forms itself (oracle.auto_frame, as test_auto_frame_is_the_oracles_on_every_shape_of_mesh).
    Another order of the leaves, another tree -- the same box for every triangle."""
    name = "cloth_double"
    verts, vidx = ri.mesh(name)
    off, span, lay = oracle.auto_frame(verts, vidx)
    step = oracle.pipeline(verts, vidx, None, off=off, span=span, layout=lay)
    want = rr.expected_records(verts, vidx, step)
    ref_step, ref = ri.step(name), ri.want(name)
    assert not np.array_equal(step["perm"], ref_step["perm"])
    assert np.array_equal(want["qb"][np.argsort(step["perm"])], ref["qb"][np.argsort(ref_step["perm"])])          # per triangle: the same query box
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.set_morton_frame(mi355cd.CD_FRAME_AUTO)
        cd.build_tree()
        goff, gspan, glay = cd.get_morton_frame()
        assert glay == lay and np.array_equal(goff, off) and np.array_equal(gspan, span)
        _check(cd, want, step, f"{name}, CD_FRAME_AUTO", FUSED)


def test_custom_ids_and_unreferenced_vertices():
    """Custom triangle IDs change nothing in the records.  Vertices no triangle references DO: the table is built from all nv vertices, so
    an unreferenced vertex in the cell of a bound makes that cell ambiguous and the bound move."""
    name = "a double soup of 600"
    verts, vidx = ri.soup_double(600, 0.2, 1601)                               # (no cell of it is ambiguous: asserted below)
    step = oracle.pipeline(verts, vidx)
    without = rr.expected_records(verts, vidx, step)
    n = without["n"]
    ids = (np.arange(n, dtype=np.uint32)[::-1] * 3 + 7).astype(np.uint32)
    # for every third triangle one unreferenced vertex a few doubles above the triangle's hi, in its cell, on every axis where there is room
    hi = verts[vidx.astype(np.int64)].max(axis=1)[::3]
    extra = hi.copy()
    for _ in range(3):
        extra = np.nextafter(extra, np.inf)
    extra = np.where(rr.cell(extra) == rr.cell(hi), extra, hi)
    more = np.ascontiguousarray(np.concatenate([verts, extra]))
    with_ = rr.expected_records(more, vidx, step)
    assert all(len(a) == 0 for a in without["table"].amb) and all(len(a) > 150 for a in with_["table"].amb)
    assert int(without["leaf"]["moved"].sum()) == 0 and int(with_["leaf"]["moved"].sum()) > 450
    m = n - 1
    assert not np.array_equal(with_["qb"], without["qb"]) and not np.array_equal(with_["rr"][:m], without["rr"][:m])
    st_ids = oracle.pipeline(verts, vidx, ids)
    assert np.array_equal(st_ids["perm"], step["perm"])                        # (IDs are not part of the tree)
    for what, v, want in (("custom IDs", verts, without), ("custom IDs and unreferenced vertices", more, with_)):
        with mi355cd.CollisionDetector(v, vidx, ids) as cd:
            cd.build_tree()
            assert cd.debug_get(mi355cd.CD_DBG_GET_TREE_WAS_FUSED) == 1
            _check(cd, want, step, f"{name}, {what}", FUSED)
