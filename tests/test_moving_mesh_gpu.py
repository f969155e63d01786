"""Every query on a mesh that MOVES, through every rebuild path: one long-lived context per sequence of tests/moving_inputs.py (two
for the queries between meshes); per frame cd_update_vertices, ONE rebuild entry, then every query in a seeded order that changes from
frame to frame.  Each result is compared bit for bit with the CPU restatement of that frame (the reference) and with a fresh context
created on that frame's vertices and built with cd_build_tree (a differential check: it also covers what the restatements do not
restate).  tests/test_moving_inputs.py shows, without a GPU, that the previous frame's result fails every comparison used here.

The witness, contour and nearest-triangle calls go through the same frames: cd_find_proximity_witness, cd_find_ccd_witness and
cd_find_collisions_contour in the permuted list of every sequence and entry, their between-mesh forms and cd_nearest_between (per
triangle and CD_NEAREST_MIN, at two radii and at +inf) in both roles of every schedule of the two sheets.  Their rows are ordered by
(face a, face b) and every column is compared by its bytes; their buffers get twice the frame's row count, so they grow on a dense
frame and are reused, oversized, on the sparse frames after it.

So do the all-results item queries and the swept points: cd_points_within ("all within": the frame's points at radius edge, every 16th
at +inf), cd_cast_rays_all ("every hit") and cd_sweep_points_all / cd_sweep_points ("swept points": the points moving by 0.6 edges,
three dists by i % 3, the mesh moving to the CCD queries' end positions -- the x1 cd_self_ccd has just refit swept[0] to in that entry,
another x1 or none in the others -- once more with the mesh at rest behind every entry but self_ccd, and on `slide` and `float_double`
the mesh's own first 1000 vertices with skip_vertex) are in the permuted list, against within_ref's and sweep_ref's all-pairs
restatements: the set of (item, face), then every column bit for bit.  Their smallest row per item is the device's own
cd_closest_points / cd_cast_rays answer; cd_sweep_points is sweep_ref.first_of of the restatement's rows; cd_debug_swept reads the same
bytes after the sweeps as before them.  On jitter's dense frame one whole 64-item block at the collapsed cluster has more rows than its
shard of the first candidate buffer holds (WITHIN_SHARD_FIRST): the pass grows the buffer and runs again, with CD_OK and the exact rows,
and the sparse frames after it run on the grown buffers.

And the mesh against itself and the points inside it: cd_nearest_self ("nearest self": per triangle and CD_NEAREST_MIN at a radius of one
edge, against the proximity witness restatement of that frame reduced per face; at +inf byte for byte against the fresh context,
against nearest_self_ref's all-pairs rows on the frames that have them, and elsewhere its MIN row against the radius' -- the clearance
is within an edge), cd_points_inside ("inside": the frame's points and 300 of its vertices moved half an edge down the axis, where
column_tri's tie rule decides, on all three axes and with parity on axis (f + seed) % 3, against column_ref's sums over all faces: the
five arrays and n_inside) and cd_signed_distance ("signed distance": on that axis, inside from the restatement, everything else the
device's own cd_closest_points answer byte for byte, the sign where inside and dist > 0) are in the permuted list too.  They read
recs32, root, leaf, the vertices, the root box for the pad, the sort's flags, and cd_nearest_self perm[0] and the Morton neighbours:
whatever an entry leaves stale of those shows here.  Between cd_update_vertices and the entry all three (and CD_NEAREST_MIN) return
CD_ERR_ORDER and write nothing.  Their node_visits and tri_tests are compared with nothing (tiny1's node_visits of
cd_points_inside is 0: there is no record to walk).

And the boxes, planes, segments and swept segments: cd_boxes_overlap_all / cd_boxes_count ("boxes": 258 boxes of box_ref.make_boxes on
the frame's vertices, the frame's root box exactly -- every triangle a row, all inside -- 16 point boxes on vertices, and 32 small
boxes beside the surface, which meet a face or not by where this frame's faces lie: CD_BOX_ANY's answer changes with the frame),
cd_planes_cut_all / cd_planes_count ("planes": 24 of plane_ref.make_planes), cd_segments_within / cd_segments_closest ("segments": 250 at
the frame's points, three radii by i % 3, every eighth a point, two at +inf) and cd_sweep_segments_all / cd_sweep_segments ("swept
segments": 250 free segments moving by 0.6 edges, the mesh moving to the CCD queries' end positions, once more at rest behind every
entry but self_ccd, and on `slide` and `float_double` every fifth edge of the mesh itself with skip_vertices) are in the permuted list,
against box_ref's, plane_ref's, segment_ref's and swept_segment_ref's all-pairs restatements: the set of (item, face), then every
column by its bytes, and the same against the fresh context's rows.  Their row buffers get twice the frame's row count; on jitter's
dense frame the growth block, as items 256 .. 319 of the segments and swept segments, overflows its shard of the candidate buffer, and
the frame has more than twice the rows of the one before.  What links the calls is held to the DEVICE's own rows: cd_boxes_count (plain
and ANY) is their per-box sum, cd_planes_count's n_cut their per-plane count (all three counts are counts_of_classes of the
restatement's classes and add up to nt), cd_segments_closest is closest_of of them, ANY "has a row" with a face that is one, its point
items cd_closest_points of the same point and radius byte for byte, and cd_sweep_segments is first_of of them.  cd_debug_swept reads the
same bytes after the swept-segment calls as before them; tiny1's count calls report node_visits == 0; between cd_update_vertices and
the entry all eight return CD_ERR_ORDER and write nothing.  boxes_tested, planes_tested, segments_tested and the bytes of
sweep_segments_info are compared with the fresh context's, (n_tested, n_evals, n_unresolved) with swept_segment_ref's counts; node_visits
and tri_tests of cd_boxes_count, cd_planes_count, cd_segments_closest and cd_sweep_segments with nothing: they count the walk.

Counters that are NOT compared with the fresh context's: node_visits and tri_tests of cd_cast_rays / cd_closest_points /
cd_sweep_points / cd_nearest_between / cd_nearest_self / cd_points_inside / cd_signed_distance (cd_nearest_between and cd_nearest_self
also not with a restatement: nearest_ref has no walk), and the collision step's node_visits and
wave_steps -- they count the walk, which may legitimately differ with the options the entry left behind (traversal bookkeeping, the
order hint; cd_nearest_between's shared bound makes them differ from run to run: test_nearest_gpu.py).  pairs_tested of a collision step is
compared with the oracle's, proximity's and CCD's evaluation counts with the restatement's and the fresh context's, n_candidates with
swept_ref's count and the fresh context's, the contour calls' n_tested with isect_ref's, cd_nearest_between's n_found with nearest_ref's;
cd_nearest_self's n_found and cd_points_inside's n_inside with their restatements' and the fresh context's;
within_tested and rays_all_tested with the fresh context's; cd_sweep_points_all's n_tested, n_evals and n_unresolved with sweep_ref's counts
and the fresh context's, its n_candidates -- a function of the swept records and the items -- with the fresh context's."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ccd_ref as cr
import mi355cd
import moving_inputs as mi
import nearest_self_ref as ns
import proximity_ref as pr
import swept_ref as sr
import within_ref as wn
from test_boxes_gpu import _Raw as RawBoxes
from test_inside_gpu import _raw as raw_inside
from test_nearest_self_gpu import _raw as raw_nearest_self, _untouched as untouched_nearest_self
from test_planes_gpu import _Raw as RawPlanes
from test_segments_gpu import _Raw as RawSegments
from test_sweep_segments_gpu import _Raw as RawSweepSegments

pytestmark = pytest.mark.gpu

CAP = 1 << 20
INF = float("inf")
ENTRIES = ("build_tree", "self_collide", "graph", "self_proximity", "self_ccd", "stagewise")
FRAME = {"reference": mi355cd.CD_FRAME_REFERENCE, "auto": mi355cd.CD_FRAME_AUTO}


def _enter(cd, entry, x1, prox_d, ccd_d):
    """One rebuild entry on the vertices the context holds.  -> the entry's own result: (pairs, n, rc) of a collision step,
    find_proximity's / find_ccd's tuple of cd_self_proximity / cd_self_ccd, None of cd_build_tree."""
    cd.set_option(mi355cd.CD_OPT_GRAPH, 1 if entry == "graph" else 0)
    if entry == "build_tree":
        cd.build_tree()
        return None
    if entry == "self_collide":
        return cd.self_collide(cap=CAP)
    if entry == "stagewise":
        cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 1)
        try:
            got = cd.self_collide(cap=CAP)
            assert cd.debug_get(mi355cd.CD_DBG_GET_TREE_WAS_FUSED) == 0
        finally:
            cd.debug_set(mi355cd.CD_DBG_STAGEWISE_BUILD, 0)
        return got
    if entry == "graph":                                                       # what a captured step needs; the frame's step is a replay
        cd.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)
        cd.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
        for _ in range(2):                                                     # capture (again, if the sort changed its form), a replay
            cd.self_collide(cap=CAP)
        rep0 = cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
        got = cd.self_collide(cap=CAP)
        # A context whose sort has gone to its half-key or full form (one long run of equal keys: `collapse`) stays with it for good and
        # captures nothing (graph_eligible in csrc/mi355cd.hip): there the step with the option on is the stream's, and must say so.
        replayed = 1 if cd.debug_get(mi355cd.CD_DBG_GET_SORT_FORM) <= 1 else 0
        assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + replayed, "the frame's step is not a replay: nothing of the graph path would be tested"
        return got
    if entry == "self_proximity":
        return cd.self_proximity(prox_d, cap=CAP)
    assert entry == "self_ccd"
    return cd.self_ccd(x1, ccd_d, cap=CAP)


def _rebuild(cd, entry, name, f):
    """The entry, with its own result against the frame's reference where it has one."""
    what = f"{name} frame {f}: {entry}'s own result"
    got = _enter(cd, entry, mi.x1(name, f), mi.prox_dist(name, f), mi.ccd_dist(name, f))
    if entry in ("self_collide", "graph", "stagewise"):
        mi.same_step(*got, cd.stats().pairs_tested, mi.want_step(name, f), what)
    elif entry == "self_proximity":
        mi.same_prox(got, mi.want_prox(name, f), what)
    elif entry == "self_ccd":
        want, counts = mi.want_ccd(name, f)
        mi.same_ccd(got, want, what, cd.ccd_info, counts)


def _equal_bytes(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, k)


def _queries(cd, fresh, name, f, entry=None):
    """The queries of frame f as (label, callable): each compares the long-lived context with the reference and with the fresh one.
    entry: the rebuild entry the frame went through (the sweep's extra call at rest is made behind every entry but self_ccd)."""
    s = mi.seq(name)
    v, vidx = s.frames[f], s.vidx
    what = f"{name} frame {f}"
    rays, pts, rm = mi.rays(name, f), mi.points(name, f), mi.radii(name, f)
    cast = lambda c, **kw: c.cast_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6], **kw)

    def proximity():
        d = mi.prox_dist(name, f)
        got = cd.find_proximity(d, cap=CAP)
        mi.same_prox(got, mi.want_prox(name, f), what + " proximity")
        tested = cd.proximity_tested
        gf = fresh.find_proximity(d, cap=CAP)
        mi.same_prox(got, pr.sort_pairs(gf[0], gf[1]), what + " proximity against the fresh context")
        assert tested == fresh.proximity_tested, (what, tested, fresh.proximity_tested)

    def ccd():
        d, e = mi.ccd_dist(name, f), mi.x1(name, f)
        want, counts = mi.want_ccd(name, f)
        got = cd.find_ccd(e, d, cap=CAP)
        info = cd.ccd_info
        mi.same_ccd(got, want, what + " ccd", info, counts)
        sr.compare_count(info.n_candidates, mi.want_candidates(name, f), what + " ccd")
        t = mi.read_swept(cd)                                                  # right after the CCD call: records, up[], M bits, the pad
        mi.same_swept(t, v, e, vidx, sr.m_bits(v, e, vidx), d, what + " swept tree")
        gf = fresh.find_ccd(e, d, cap=CAP)
        mi.same_ccd(got, cr.sort_pairs(*gf[:3]), what + " ccd against the fresh context")
        fi = fresh.ccd_info
        assert bytes(info) == bytes(fi), (what, [(k, getattr(info, k), getattr(fi, k)) for k, _ in mi355cd.CdCcdInfo._fields_])
        tf = mi.read_swept(fresh)
        # slot n - 1 of the records names no split: nothing writes it.  Word 7 is the range word: its low 30 bits; bits 30 / 31 are the static
        # records' CERTAIN / EXACT flags, copied along, defined only where a child is a leaf, and differ between the stage-wise and the fused
        # build elsewhere (test_cd_gpu.py's _compare_records) -- no walk of the swept tree reads them (REC_LAST_MASK)
        m = max(s.nt - 1, 0)
        part = lambda r: (r["srr"][:m, :7], r["srl"][:m, :7], r["srr"][:m, 7] & sr.REC_MASK, r["srl"][:m, 7] & sr.REC_MASK, r["up"], r["perm"])
        _equal_bytes(part(t), part(tf), what + " swept tree against the fresh context")
        assert t["m_bits"] == tf["m_bits"] and sr.bits1(t["pad"]) == sr.bits1(tf["pad"]), what

    def ray_queries():
        want = mi.want_rays(name, f)
        got = cast(cd)
        mi.same_rays(got, want, what + " rays")
        gf = cast(fresh)
        mi.same_rays(got[:5], gf[:5], what + " rays against the fresh context")
        assert got[5].n_hits == gf[5].n_hits
        face, info = cast(cd, any_hit=True)
        mi.same_any_hit(face, info.n_hits, rays, v, vidx, want, what + " any hit")

    def point_queries():
        got = cd.closest_points(pts)
        mi.same_points(got, mi.want_points(name, f), what + " points")
        got = cd.closest_points(pts, rm)
        mi.same_points(got, mi.want_points_r(name, f), what + " points with radii")
        gf = fresh.closest_points(pts, rm)
        mi.same_points(got[:7], gf[:7], what + " points against the fresh context")
        assert got[7].n_found == gf[7].n_found
        face, info = cd.closest_points(pts, rm, any_within=True)
        mi.same_any_within(face, info.n_found, pts, rm, v, vidx, mi.want_points_r(name, f), what + " any within")

    def box():
        got = cd.root_box()
        mi.same_root_box(got, mi.want_root_box(name, f), what + " root box")
        mi.same_root_box(got, fresh.root_box(), what + " root box against the fresh context")

    twice = lambda rows: max(1, 2 * rows.faces.shape[0])                       # the witness / contour buffers: grown on the dense frame, oversized after it

    def proximity_witness():
        d, want = mi.prox_dist(name, f), mi.want_prox_witness(name, f)
        got = cd.find_proximity_witness(d, cap=twice(want))
        tested = cd.proximity_tested
        mi.same_witness(got, want, what + " proximity witness")
        mi.same_prox(got[:4], mi.want_prox(name, f), what + " proximity witness: the plain call's pairs and distances")
        gf = fresh.find_proximity_witness(d, cap=twice(want))
        assert gf[3] == mi355cd.CD_OK, what
        mi.same_witness(got, mi.witness_rows(gf), what + " proximity witness against the fresh context")
        assert tested == fresh.proximity_tested, (what, tested, fresh.proximity_tested)
        mi.same_as_plain(got[:4], cd.find_proximity(d, cap=CAP), what + " proximity witness against the plain call")

    def ccd_witness():
        d, e, want = mi.ccd_dist(name, f), mi.x1(name, f), mi.want_ccd_witness(name, f)
        plain, counts = mi.want_ccd(name, f)
        got = cd.find_ccd_witness(e, d, cap=twice(want))
        info = cd.ccd_info
        mi.same_witness(got, want, what + " ccd witness")
        mi.same_ccd(got[:5], plain, what + " ccd witness: the plain call's pairs, toi and distances", info, counts)
        sr.compare_count(info.n_candidates, mi.want_candidates(name, f), what + " ccd witness")
        gf = fresh.find_ccd_witness(e, d, cap=twice(want))
        assert gf[4] == mi355cd.CD_OK, what
        mi.same_witness(got, mi.witness_rows(gf), what + " ccd witness against the fresh context")
        fi = fresh.ccd_info
        assert bytes(info) == bytes(fi), (what, [(k, getattr(info, k), getattr(fi, k)) for k, _ in mi355cd.CdCcdInfo._fields_])
        mi.same_as_plain(got[:5], cd.find_ccd(e, d, cap=CAP), what + " ccd witness against the plain call")

    def contour():
        want = mi.want_contour(name, f)
        got = cd.find_collisions_contour(cap=twice(want))
        tested = cd.contour_tested
        mi.same_contour(got, want, what + " contour", tested)
        mi.same_pair_set(got[0], mi.want_step(name, f)["pairs"], what + " contour: the collision step's pair set")
        gf = fresh.find_collisions_contour(cap=twice(want))
        assert gf[2] == mi355cd.CD_OK, what
        mi.same_contour(got, mi.contour_rows(gf, fresh.contour_tested), what + " contour against the fresh context", tested)

    room = lambda rows: max(1, 2 * rows.rows.shape[0])                         # the item queries' row buffers, in the same way

    def all_within():
        pts, rad = mi.within_items(name, f)
        want = mi.want_within(name, f)
        got = cd.points_within(pts, rad, cap=room(want))
        tested = cd.within_tested
        mi.same_item_rows(got, want, what + " all within")
        gf = fresh.points_within(pts, rad, cap=room(want))
        mi.same_item_rows(got, mi.item_rows(gf), what + " all within against the fresh context")
        assert tested == fresh.within_tested and tested >= got[-2], (what, tested, fresh.within_tested)
        single = cd.closest_points(pts, rad)                                    # (pinned by point_queries) per point the smallest row
        _equal_bytes(wn.closest_of(mi.item_rows(got), pts.shape[0]), single[:7], what + " all within: the smallest row a point against closest_points")
        if pts.shape[0] > mi.NQ:                                                # the dense frame: the growth block alone overflows its shard
            assert int((got[0][:, 0] >= mi.GROWTH_AT).sum()) > mi355cd.WITHIN_SHARD_FIRST, what

    def every_hit():
        want = mi.want_rays_all(name, f)
        call = lambda c: c.cast_rays_all(rays[:, 0:3], rays[:, 3:6], rays[:, 6], cap=room(want))
        got = call(cd)
        tested = cd.rays_all_tested
        mi.same_item_rows(got, want, what + " every hit")
        mi.same_item_rows(got, mi.item_rows(call(fresh)), what + " every hit against the fresh context")
        assert tested == fresh.rays_all_tested and tested >= got[-2], (what, tested, fresh.rays_all_tested)
        _equal_bytes(wn.first_hit_of(mi.item_rows(got), rays.shape[0]), cast(cd)[:5], what + " every hit: the smallest row a ray against cast_rays")

    def swept_points():
        it, e = mi.sweep_items(name, f), mi.x1(name, f)
        n = it.shape[0]
        want, counts = mi.want_sweep(name, f)
        before = _swept(cd)
        sweep = lambda c, items, end, rows, skip=None: c.sweep_points_all(items[:, 0:3], items[:, 3:6], items[:, 6], verts_end=end, skip_vertex=skip, cap=room(rows))
        tally = lambda i: (i.n_tested, i.n_evals, i.n_unresolved)
        got = sweep(cd, it, e, want)
        info = cd.sweep_info
        mi.same_item_rows(got, want, what + " swept points")
        assert tally(info) == counts and info.n_candidates >= info.n_tested, (what, tally(info), counts, info.n_candidates)
        gf = sweep(fresh, it, e, want)
        fi = fresh.sweep_info
        mi.same_item_rows(got, mi.item_rows(gf), what + " swept points against the fresh context")
        assert bytes(info) == bytes(fi), (what, [(k, getattr(info, k), getattr(fi, k)) for k, _ in mi355cd.CdCcdInfo._fields_])
        if n > mi.NQ:
            assert int((got[0][:, 0] >= mi.GROWTH_AT).sum()) > mi355cd.WITHIN_SHARD_FIRST, what
        first = cd.sweep_points(it[:, 0:3], it[:, 3:6], it[:, 6], verts_end=e)
        mi.same_first_contact(first, want, n, what + " swept points")
        ff = fresh.sweep_points(it[:, 0:3], it[:, 3:6], it[:, 6], verts_end=e)
        _equal_bytes(first[:8], ff[:8], what + " first contact against the fresh context")
        assert first[8].n_found == ff[8].n_found, what
        if entry != "self_ccd":                                                 # the mesh at rest: the swept records of the vertices themselves
            still, still_counts = mi.want_sweep_still(name, f)
            got = sweep(cd, it, None, still)
            mi.same_item_rows(got, still, what + " swept points, the mesh at rest")
            assert tally(cd.sweep_info) == still_counts, (what, tally(cd.sweep_info), still_counts)
        if name in mi.SELF_SWEEP:                                               # the mesh's own vertices against its own faces
            (items, skip), (own, own_counts) = mi.self_sweep_items(name, f), mi.want_self_sweep(name, f)
            got = sweep(cd, items, e, own, skip)
            mi.same_item_rows(got, own, what + " swept points, the mesh's own vertices")
            assert tally(cd.sweep_info) == own_counts, (what, tally(cd.sweep_info), own_counts)
            mi.same_item_rows(got, mi.item_rows(sweep(fresh, items, e, own, skip)), what + " the mesh's own vertices against the fresh context")
            mi.same_first_contact(cd.sweep_points(items[:, 0:3], items[:, 3:6], items[:, 6], verts_end=e, skip_vertex=skip), own, items.shape[0],
                                  what + " the mesh's own vertices")
        after = _swept(cd)                                                      # swept[0] is the CCD pass's: no sweep may touch it
        assert (before is None) == (after is None), what
        if before is not None:
            _equal_bytes(before[:3], after[:3], what + " the CCD pass's swept tree after the sweeps")
            assert before[3] == after[3] and sr.bits1(before[4]) == sr.bits1(after[4]), what

    def nearest_self():
        r, want = mi.nearest_self_r(name, f), mi.want_nearest_self(name, f)
        least = ns.nearest_min(want)
        mi.same_nearest_self(cd.nearest_self(r, witness=True), want, what + " nearest self")
        mi.same_nearest_self(cd.nearest_self(r, minimum=True, witness=True), least, what + " nearest self, MIN")
        flat = lambda g: (g.faces, g.ids, g.dist, g.witness.faces, g.witness.points, g.witness.bary, g.witness.feature)
        rows, one = cd.nearest_self(INF, witness=True), cd.nearest_self(INF, minimum=True, witness=True)
        for got, minimum in ((rows, False), (one, True)):
            gf = fresh.nearest_self(INF, minimum=minimum, witness=True)
            _equal_bytes(flat(got), flat(gf), f"{what} nearest self at +inf{', MIN' if minimum else ''} against the fresh context")
            assert got.info.n_found == gf.info.n_found, (what, got.info.n_found, gf.info.n_found)
        if mi.has_nearest_self_inf(name, f):
            every = mi.want_nearest_self_inf(name, f)
            mi.same_nearest_self(rows, every, what + " nearest self at +inf")
            mi.same_nearest_self(one, ns.nearest_min(every), what + " nearest self at +inf, MIN")
        else:                                                                   # the clearance is within the radius, so it is the radius' MIN row
            assert least[0].faces[0, 0] != ns.NONE, what
            mi.same_nearest_self(one, least, what + " nearest self at +inf, MIN")

    turn = (f + s.seed) % 3                                                     # the axis of the parity call and of the signed distance

    def inside():
        for axis, parity in ((0, False), (1, False), (2, False), (turn, True)):
            w = f"{what} inside, axis {axis}{', parity' if parity else ''}"
            p = mi.inside_points(name, f, axis)
            got = cd.points_inside(p, axis, parity=parity)
            mi.same_inside(got, mi.want_inside(name, f, axis, parity), w)
            gf = fresh.points_inside(p, axis, parity=parity)
            _equal_bytes(got[:5], gf[:5], w + " against the fresh context")
            assert got[5].n_inside == gf[5].n_inside, (w, got[5].n_inside, gf[5].n_inside)
            if s.nt == 1:                                                       # no record to walk
                assert got[5].node_visits == 0, (w, got[5].node_visits)

    def signed_distance():
        p = mi.inside_points(name, f, turn)
        sdist, face, ids, closest, uv, feature, ins, info = cd.signed_distance(p, turn)
        near = cd.closest_points(p)                                             # (pinned by point_queries)
        w = f"{what} signed distance, axis {turn}"
        assert np.array_equal(ins, mi.want_inside(name, f, turn)[0]), w
        _equal_bytes((face, ids, np.abs(sdist), closest, uv, feature), near[:6], w + " against closest_points")
        assert np.array_equal(np.signbit(sdist), ins & (near[2] > 0)), w
        assert info.n_found == p.shape[0], (w, info.n_found)

    def boxes():
        b = mi.box_items(name, f)
        lo, hi, n = b[:, 0::2], b[:, 1::2], b.shape[0]
        want = mi.want_boxes(name, f)
        got = cd.boxes_overlap_all(lo, hi, cap=room(want))
        tested = cd.boxes_tested
        mi.same_item_rows(got, want, what + " boxes")
        mi.same_item_rows(got, mi.item_rows(fresh.boxes_overlap_all(lo, hi, cap=room(want))), what + " boxes against the fresh context")
        assert tested == fresh.boxes_tested and tested >= got[-2], (what, tested, fresh.boxes_tested)
        own = mi.item_rows(got)                                                 # the count calls are the per-item sums of the DEVICE's rows
        for any_ in (False, True):
            c, cf = cd.boxes_count(lo, hi, any=any_), fresh.boxes_count(lo, hi, any=any_)
            mi.same_box_counts(c, own, n, f"{what} boxes count{', ANY' if any_ else ''}", any_)
            _equal_bytes(c[:1 if any_ else 2], cf[:1 if any_ else 2], what + " boxes count against the fresh context")
            assert c[2].n_found == cf[2].n_found, what
            if s.nt == 1:                                                       # no record to walk
                assert c[2].node_visits == 0, (what, c[2].node_visits)
            elif not any_:
                assert c[0][mi.NBOX] == s.nt == c[1][mi.NBOX], what             # the root box: the whole mesh, all of it inside

    def planes():
        p = mi.plane_items(name, f)
        nrm, d = p[:, :3], p[:, 3]
        want, cls = mi.want_planes(name, f), mi.want_plane_classes(name, f)
        got = cd.planes_cut_all(nrm, d, cap=room(want))
        tested = cd.planes_tested
        mi.same_item_rows(got, want, what + " planes")
        mi.same_item_rows(got, mi.item_rows(fresh.planes_cut_all(nrm, d, cap=room(want))), what + " planes against the fresh context")
        assert tested == fresh.planes_tested and tested >= got[-2], (what, tested, fresh.planes_tested)
        c, cf = cd.planes_count(nrm, d), fresh.planes_count(nrm, d)
        mi.same_plane_counts(c, cls, what + " planes count")                    # (... and the three add up to nt)
        assert np.array_equal(c[0], wn.rows_per_item(mi.item_rows(got), p.shape[0])), what + " planes count: n_cut is the device's own rows a plane"
        _equal_bytes(c[:3], cf[:3], what + " planes count against the fresh context")
        assert c[3].n_found == cf[3].n_found, what
        if s.nt == 1:
            assert c[3].node_visits == 0, (what, c[3].node_visits)

    def segments():
        it = mi.segment_items(name, f)
        a, b, r, n = it[:, 0:3], it[:, 3:6], it[:, 6], it.shape[0]
        want = mi.want_segments(name, f)
        got = cd.segments_within(a, b, r, cap=room(want))
        tested = cd.segments_tested
        mi.same_item_rows(got, want, what + " segments")
        mi.same_item_rows(got, mi.item_rows(fresh.segments_within(a, b, r, cap=room(want))), what + " segments against the fresh context")
        assert tested == fresh.segments_tested and tested >= got[-2], (what, tested, fresh.segments_tested)
        if n > mi.NI:                                                           # the dense frame: the growth block alone overflows its shard
            assert int((got[0][:, 0] >= mi.SEG_GROWTH_AT).sum()) > mi355cd.WITHIN_SHARD_FIRST, what
        own = mi.item_rows(got)
        single = cd.segments_closest(a, b, r)
        mi.same_segment_closest(single, own, n, what + " segments: the smallest row a segment")
        sf = fresh.segments_closest(a, b, r)
        _equal_bytes(single[:11], sf[:11], what + " segments closest against the fresh context")
        assert single[11].n_found == sf[11].n_found, what
        face, info = cd.segments_closest(a, b, r, any_within=True)
        mi.same_segment_any(face, info, own, n, what + " segments, ANY")
        pt = np.arange(0, mi.NI, mi.SEG_POINT_EVERY)                            # b == a: cd_closest_points (pinned by point_queries) byte for byte
        assert np.array_equal(a[pt], b[pt])
        near = cd.closest_points(a[pt], r[pt])
        _equal_bytes(tuple(single[k][pt] for k in (0, 1, 2, 5, 6, 7, 10)), near[:7], what + " segments: the point items against closest_points")

    def swept_segments():
        it, e = mi.swept_segment_items(name, f), mi.x1(name, f)
        n = it.shape[0]
        want, counts = mi.want_swept_segments(name, f)
        before = _swept(cd)
        ends = lambda x: (x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12], x[:, 12])
        sweep = lambda c, items, end, rows, skip=None: c.sweep_segments_all(*ends(items), verts_end=end, skip_vertices=skip, cap=room(rows))
        tally = lambda i: (i.n_tested, i.n_evals, i.n_unresolved)
        got = sweep(cd, it, e, want)
        info = cd.sweep_segments_info
        mi.same_item_rows(got, want, what + " swept segments")
        assert tally(info) == counts and info.n_candidates >= info.n_tested, (what, tally(info), counts, info.n_candidates)
        gf = sweep(fresh, it, e, want)
        fi = fresh.sweep_segments_info
        mi.same_item_rows(got, mi.item_rows(gf), what + " swept segments against the fresh context")
        assert bytes(info) == bytes(fi), (what, [(k, getattr(info, k), getattr(fi, k)) for k, _ in mi355cd.CdCcdInfo._fields_])
        if n > mi.NI:
            assert int((got[0][:, 0] >= mi.SEG_GROWTH_AT).sum()) > mi355cd.WITHIN_SHARD_FIRST, what
        first = cd.sweep_segments(*ends(it), verts_end=e)
        mi.same_sweep_segments(first, mi.item_rows(got), n, what + " swept segments: the first row an item")
        ff = fresh.sweep_segments(*ends(it), verts_end=e)
        _equal_bytes(first[:12], ff[:12], what + " swept segments, first contact against the fresh context")
        assert first[12].n_found == ff[12].n_found, what
        if entry != "self_ccd":                                                 # the mesh at rest
            still, still_counts = mi.want_swept_segments_still(name, f)
            got = sweep(cd, it, None, still)
            mi.same_item_rows(got, still, what + " swept segments, the mesh at rest")
            assert tally(cd.sweep_segments_info) == still_counts, (what, tally(cd.sweep_segments_info), still_counts)
            mi.same_sweep_segments(cd.sweep_segments(*ends(it)), mi.item_rows(got), n, what + " swept segments, the mesh at rest: the first row an item")
        if name in mi.SELF_SWEEP:                                               # the mesh's own edges against its own faces
            (items, skip), (own, own_counts) = mi.self_swept_segment_items(name, f), mi.want_self_swept_segments(name, f)
            got = sweep(cd, items, e, own, skip)
            mi.same_item_rows(got, own, what + " swept segments, the mesh's own edges")
            assert tally(cd.sweep_segments_info) == own_counts, (what, tally(cd.sweep_segments_info), own_counts)
            mi.same_item_rows(got, mi.item_rows(sweep(fresh, items, e, own, skip)), what + " the mesh's own edges against the fresh context")
            mi.same_sweep_segments(cd.sweep_segments(*ends(items), verts_end=e, skip_vertices=skip), own, items.shape[0], what + " the mesh's own edges")
        after = _swept(cd)                                                      # swept[0] is the CCD pass's: no swept segment may touch it
        assert (before is None) == (after is None), what
        if before is not None:
            _equal_bytes(before[:3], after[:3], what + " the CCD pass's swept tree after the swept segments")
            assert before[3] == after[3] and sr.bits1(before[4]) == sr.bits1(after[4]), what

    return [("proximity", proximity), ("ccd", ccd), ("rays", ray_queries), ("points", point_queries), ("root box", box),
            ("proximity witness", proximity_witness), ("ccd witness", ccd_witness), ("contour", contour),
            ("all within", all_within), ("every hit", every_hit), ("swept points", swept_points),
            ("nearest self", nearest_self), ("inside", inside), ("signed distance", signed_distance),
            ("boxes", boxes), ("planes", planes), ("segments", segments), ("swept segments", swept_segments)]


def _swept(cd):
    """cd_debug_swept of the context's own swept tree, or None before its first CCD pass (CD_ERR_ORDER)."""
    try:
        return cd.debug_swept()
    except mi355cd.CdError as e:
        assert e.rc == mi355cd.CD_ERR_ORDER
        return None


def _order_errors_items(cd, name, f):
    """The same for the box, plane, segment and swept-segment calls, all eight, on the frame's own items (the first 64): CD_ERR_ORDER,
    and nothing written into the canary-filled rows, values, counts, faces and info structs."""
    lib, E = cd.lib, mi355cd.CD_ERR_ORDER
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    first = lambda items: np.ascontiguousarray(items[:64])
    canary = lambda: np.full(64, 7, dtype=np.uint32)
    untouched = lambda arrays, info: all((a == 7).all() for a in arrays) and (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)
    boxes, planes, segs, sweeps = first(mi.box_items(name, f)), first(mi.plane_items(name, f)), first(mi.segment_items(name, f)), first(mi.swept_segment_items(name, f))
    x1 = np.ascontiguousarray(mi.x1(name, f), dtype=np.float64)
    r = RawBoxes(cd, 256)
    assert r.call(boxes, 256) == E and r.nothing_written(), "cd_boxes_overlap_all"
    for flags in (0, mi355cd.CD_BOX_ANY):
        count, n_inside, info = canary(), canary(), mi355cd.CdBoxInfo(5, 5, 5)
        rc = lib.cd_boxes_count(cd._ctx, vp(boxes), boxes.shape[0], flags, vp(count), None if flags else vp(n_inside), C.byref(info))
        assert rc == E and untouched((count, n_inside), info), ("cd_boxes_count", flags, rc)
    r = RawPlanes(cd, 256)
    assert r.call(planes, 256) == E and r.nothing_written(), "cd_planes_cut_all"
    counts, info = [canary() for _ in range(3)], mi355cd.CdPlaneInfo(5, 5, 5)
    rc = lib.cd_planes_count(cd._ctx, vp(planes), planes.shape[0], *map(vp, counts), C.byref(info))
    assert rc == E and untouched(counts, info), ("cd_planes_count", rc)
    r = RawSegments(cd, 256)
    assert r.call(segs, 256) == E and r.closest(segs) == E and r.nothing_written(), "cd_segments_within, cd_segments_closest"
    assert r.closest(segs, flags=mi355cd.CD_SEGMENT_ANY, out=False) == E and r.nothing_written(), "cd_segments_closest, ANY"
    for end in (x1, None):
        r = RawSweepSegments(cd, 256)
        assert r.call(sweeps, 256, end) == E and r.nothing_written(), "cd_sweep_segments_all"
        assert tuple(getattr(r.info, k) for k, _ in mi355cd.CdCcdInfo._fields_) == (7,) * 4, "cd_sweep_segments_all wrote into its info"
        face, info = canary(), mi355cd.CdPointInfo(5, 5, 5)
        rc = lib.cd_sweep_segments(cd._ctx, None if end is None else vp(end), vp(sweeps), sweeps.shape[0], None, 0, vp(face), C.byref(r.out), C.byref(info))
        assert rc == E and untouched((face,), info) and r.nothing_written(), ("cd_sweep_segments", rc)


def _order_errors_self(cd, pts, rmax, name, f):
    """The vertices moved and the tree was not rebuilt: cd_nearest_self (both flags), cd_points_inside and cd_signed_distance return
    CD_ERR_ORDER and write nothing -- not a row of the canary-filled outputs, not a field of the info structs.  Neither do the eight
    box, plane, segment and swept-segment calls (_order_errors_items)."""
    _order_errors_items(cd, name, f)
    lib, E = cd.lib, mi355cd.CD_ERR_ORDER
    info = mi355cd.CdNearestInfo(5, 5, 5)
    for r in (rmax, INF):
        for flags in (0, mi355cd.CD_NEAREST_MIN):
            rc, arr = raw_nearest_self(lib, cd._ctx, r, flags, cd.nt, info=info)
            assert rc == E, (r, flags, rc)
            untouched_nearest_self(arr)
    assert (info.n_found, info.node_visits, info.tri_tests) == (5, 5, 5)
    for axis in (0, 1, 2):
        for flags in (0, mi355cd.CD_INSIDE_PARITY):
            assert raw_inside(lib, cd._ctx, pts, axis, flags) == (E, E, True), (axis, flags)


def _new(verts, vidx, mode):
    cd = mi355cd.CollisionDetector(verts, vidx)
    if mode != "reference":
        cd.set_morton_frame(FRAME[mode])
    return cd


def _run(name, schedule):
    s = mi.seq(name)
    order = np.random.default_rng(s.seed)
    used = []
    with _new(s.frames[0], s.vidx, s.frame_mode) as cd:
        for f, v in enumerate(s.frames):
            entry = ENTRIES[(f + s.seed) % len(ENTRIES)] if schedule == "rotate" else schedule
            if name == "frame_exit" and f == len(s) - 1:                       # back inside for a frame already: after 64 more sorts the first form gets its try
                for _ in range(70):
                    cd.build_tree()
            cd.update_vertices(v)
            _order_errors_self(cd, mi.inside_points(name, f, 2), mi.nearest_self_r(name, f), name, f)
            _rebuild(cd, entry, name, f)
            used.append(entry)
            if name == "frame_exit":
                form = cd.debug_get(mi355cd.CD_DBG_GET_SORT_FORM)
                assert form == (1 if f in mi.FRAME_EXIT_OUT else 0) or (f == len(s) - 2 and form == 1), (f, form)
            with _new(v, s.vidx, s.frame_mode) as fresh:
                fresh.build_tree()
                qs = _queries(cd, fresh, name, f, entry)
                for k in order.permutation(len(qs)):                           # no query's result depends on which one ran before it
                    qs[k][1]()
    if schedule == "rotate" and len(s) >= len(ENTRIES):
        assert set(used) == set(ENTRIES)
    assert all(a != b for a, b in zip(used, used[1:])) or schedule != "rotate"


@pytest.mark.parametrize("entry", ENTRIES)
def test_jitter_through_one_entry_every_frame(entry):
    """The same rebuild entry every frame; frame 2 is the dense one (a shard of the first candidate buffers overflows: the passes grow
    their buffers), the later frames are sparse again and still exact, with CD_OK (same_prox / same_ccd assert the return code)."""
    assert mi.ccd_shard_load("jitter", mi.JITTER_DENSE_FRAME) > mi.SHARD_FIRST
    _run("jitter", entry)


@pytest.mark.parametrize("name", mi.NAMES)
def test_every_sequence_through_rotating_entries(name):
    """Consecutive frames go through different entries; a sequence of six frames or more goes through all six."""
    _run(name, "rotate")


# ---------------------------------------------------------------- between two meshes
SENTINEL = 0xDEADBEEF


def _order_errors(a, b):
    """A mesh moved and its tree was not rebuilt: every query between the two, in both roles, returns CD_ERR_ORDER and writes nothing."""
    lib = a.lib
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    p = lambda x: x.ctypes.data
    pairs, toi, d = np.full((16, 2), SENTINEL, dtype=np.uint32), np.full(16, -7.0), np.full(16, -7.0)
    n, t, info = C.c_uint64(0), C.c_uint64(0), mi355cd.CdCcdInfo()
    rows = max(a.nt, b.nt)                                                      # cd_nearest_between writes a row per triangle of its first mesh
    u32 = {k: np.full((r, 2), SENTINEL, dtype=np.uint32) for k, r in (("witness faces", 16), ("contour faces", 16), ("faces", rows), ("ids", rows), ("nearest faces", rows))}
    f64 = {k: np.full(shape, -7.0) for k, shape in (("points", (16, 2, 3)), ("bary", (16, 2, 2)), ("param", (16, 2, 3)), ("contour points", (16, 2, 3)),
                                                    ("dist", (rows,)), ("nearest points", (rows, 2, 3)), ("nearest bary", (rows, 2, 2)))}
    u8 = {k: np.full(shape, 0xEE, dtype=np.uint8) for k, shape in (("feature", (16, 2)), ("code", (16, 3)), ("nearest feature", (rows, 2)))}
    wit = mi355cd.CdWitnessOut(p(u32["witness faces"]), p(f64["points"]), p(f64["bary"]), p(u8["feature"]))
    con = mi355cd.CdContourOut(p(u32["contour faces"]), p(u8["code"]), p(f64["param"]), p(f64["contour points"]))
    nwit = mi355cd.CdWitnessOut(p(u32["nearest faces"]), p(f64["nearest points"]), p(f64["nearest bary"]), p(u8["nearest feature"]))
    ninfo = mi355cd.CdNearestInfo(5, 5, 5)
    E = mi355cd.CD_ERR_ORDER
    for x, y in ((a, b), (b, a)):
        assert lib.cd_find_collisions_between(x._ctx, y._ctx, vp(pairs), 16, C.byref(n), C.byref(t)) == E
        assert lib.cd_find_proximity_between(x._ctx, y._ctx, mi.BETWEEN_DIST, vp(pairs), vp(d), 16, C.byref(n), C.byref(t)) == E
        assert lib.cd_find_ccd_between(x._ctx, None, y._ctx, None, mi.BETWEEN_CCD_DIST, vp(pairs), vp(toi), vp(d), 16, C.byref(n), C.byref(info)) == E
        assert lib.cd_find_proximity_between_witness(x._ctx, y._ctx, mi.BETWEEN_DIST, vp(pairs), vp(d), 16, C.byref(n), C.byref(t), C.byref(wit)) == E
        assert lib.cd_find_ccd_between_witness(x._ctx, None, y._ctx, None, mi.BETWEEN_CCD_DIST, vp(pairs), vp(toi), vp(d), 16, C.byref(n), C.byref(info),
                                               C.byref(wit)) == E
        assert lib.cd_find_collisions_between_contour(x._ctx, y._ctx, vp(pairs), 16, C.byref(n), C.byref(t), C.byref(con)) == E
        for flags, r in ((0, mi.NEAREST_R), (0, float("inf")), (mi355cd.CD_NEAREST_MIN, mi.NEAREST_R), (mi355cd.CD_NEAREST_MIN, float("inf"))):
            assert lib.cd_nearest_between(x._ctx, y._ctx, r, flags, vp(u32["faces"]), vp(u32["ids"]), vp(f64["dist"]), C.byref(nwit), C.byref(ninfo)) == E
    assert (pairs == SENTINEL).all() and (toi == -7.0).all() and (d == -7.0).all()
    assert all((x == SENTINEL).all() for x in u32.values()) and all((x == -7.0).all() for x in f64.values()) and all((x == 0xEE).all() for x in u8.values())
    assert (ninfo.n_found, ninfo.node_visits, ninfo.tri_tests) == (5, 5, 5)


def _new_between_queries(x, y, schedule, f, swap, w, ends, what):
    """The witness, contour and nearest-triangle calls of x against y on frame f, each against the frame's reference w (mi.want_between)."""
    twice = lambda rows: max(1, 2 * rows.faces.shape[0])
    ex, ey = ends
    g = x.find_proximity_between_witness(y, mi.BETWEEN_DIST, cap=twice(w["prox_witness"]))
    mi.same_witness(g, w["prox_witness"], what + " proximity witness")
    mi.same_between_prox(g[:4], w["prox"], what + " proximity witness: the plain call's pairs and distances")
    # the end positions of this schedule: None for the mesh that never moves -- the call before or after it (the plain CCD query of this
    # frame, the witness call of the frame before) left a swept tree of y under other end positions in x
    g = x.find_ccd_between_witness(y, mi.BETWEEN_CCD_DIST, ex, ey, cap=twice(w["ccd_witness"]))
    mi.same_witness(g, w["ccd_witness"], what + " ccd witness")
    mi.same_as_plain(g[:5], x.find_ccd_between(y, mi.BETWEEN_CCD_DIST, ex, ey, cap=CAP), what + " ccd witness against the plain call")
    g = x.find_collisions_between_contour(y, cap=twice(w["contour"]))
    mi.same_contour(g, w["contour"], what + " contour", x.between_tested)
    mi.same_between_contact(g[:3], w["contact"][0], what + " contour: the plain call's pair set")
    assert (schedule == mi.APART) == (w["contour"].faces.shape[0] == 0), what
    for rmax, rows, least in ((mi.NEAREST_R, w["near"], w["near_min"]), (mi.NEAREST_R / 4, w["near_q"], w["near_q_min"])):
        mi.same_nearest(x.nearest_between(y, rmax, witness=True), rows, f"{what} nearest within {rmax:g}")
        mi.same_nearest(x.nearest_between(y, rmax, minimum=True, witness=True), least, f"{what} nearest within {rmax:g}, MIN")
    assert (w["near"].faces[:, 0] != mi355cd.NEAREST_NONE).any(), what        # ... so the closest pair of all is within NEAREST_R
    mi.same_nearest(x.nearest_between(y, float("inf"), minimum=True, witness=True), w["near_min"], what + " nearest, MIN at +inf")
    if schedule == mi.APART and not swap and f in mi.APART_INF_FRAMES:
        mi.same_nearest(x.nearest_between(y, float("inf"), witness=True), mi.want_between_inf(f), what + " nearest at +inf")


@pytest.mark.parametrize("schedule", mi.BETWEEN_SCHEDULES)
def test_between_two_meshes_that_move(schedule):
    """Context a is one sheet of `slide`, b the other; only a moves, only b moves, or both (and with both_move_apart b is also lifted
    off a by another amount every frame: the sheets do not touch and their separation distance changes).  A context that did not move
    is neither updated nor rebuilt: what a keeps of b from the last CCD call (and b of a) is the previous frame's and must not be used."""
    va, ia, vb, ib = mi.between_meshes()
    pos = mi.between_positions(schedule)
    with mi355cd.CollisionDetector(pos[0][0], ia) as a, mi355cd.CollisionDetector(pos[0][1], ib) as b:
        for f, (wa, wb, ma, mb) in enumerate(pos):
            ea, eb = mi.between_x1(schedule, f)
            ema, emb = mi.between_x1_moving(schedule, f)
            if ma:
                a.update_vertices(wa)
            if mb:
                b.update_vertices(wb)
            if ma or mb:
                _order_errors(a, b)
            for cd, moved, e, k in ((a, ma, ea, f), (b, mb, eb, f + 3)):
                if moved or f == 0:
                    _enter(cd, ENTRIES[k % len(ENTRIES)], e, mi.BETWEEN_DIST, mi.BETWEEN_CCD_DIST)
            for x, y, swap in ((a, b, False), (b, a, True)):
                what = f"{schedule} frame {f}, roles {'(b, a)' if swap else '(a, b)'}"
                w = mi.want_between(schedule, f, swap)
                (vx, ex, ix), (vy, ey, iy) = ((wb, eb, ib), (wa, ea, ia)) if swap else ((wa, ea, ia), (wb, eb, ib))
                ends = (emb, ema) if swap else (ema, emb)
                if f % 2:                                                       # before the plain calls in the odd frames, after them in the even ones
                    _new_between_queries(x, y, schedule, f, swap, w, ends, what)
                mi.same_between_contact(x.find_collisions_between(y, cap=CAP), w["contact"][0], what + " contact")
                assert x.between_tested == w["contact"][1], (what, x.between_tested, w["contact"][1])
                mi.same_between_prox(x.find_proximity_between(y, mi.BETWEEN_DIST, cap=CAP), w["prox"], what + " proximity")
                mi.same_between_ccd(x.find_ccd_between(y, mi.BETWEEN_CCD_DIST, ex, ey, cap=CAP), w["ccd"], what + " ccd")
                t = mi.read_swept(x, y)                                        # what x holds of y after the CCD call
                mi.same_swept(t, vy, ey, iy, sr.m_bits_between(vx, ex, ix, vy, ey, iy), mi.BETWEEN_CCD_DIST, what + " swept tree",
                              a=(vx, ex, ix, x.export_keys()[1]), n_candidates=x.ccd_info.n_candidates)
                if not f % 2:
                    _new_between_queries(x, y, schedule, f, swap, w, ends, what)
