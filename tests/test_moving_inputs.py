"""The motion sequences of tests/moving_inputs.py can catch stale state, shown on the CPU: consecutive frames have different right
answers, each sequence does what it is named for, and every comparison helper of tests/test_moving_mesh_gpu.py raises when it is fed
frame f - 1's expected result against frame f's (the planted error: a device that kept the previous frame's state), and the
comparisons of the witness, contour, nearest-triangle, all-within, every-hit and swept-point rows also when one field of one row of the
right frame's result is changed.  The conditions the all-results and swept-point queries need of their items -- items without a row,
items with several, contacts strictly inside the step, a block that overflows its shard -- are asserted here too.  So are those of
the self-nearest and inside references: rows with a partner, points with a face over them, points inside, covers the tie rule decided;
and the two routes to the self-nearest rows (the reduced proximity restatement, all pairs cut to the radius) agree column by column.
The box, plane, segment and swept-segment comparisons are held to the same three things at the end of the file: the previous frame's
result fails each of them, one changed value of any column, count or output fails them, and in every frame of the large sequences the
items include some without a row, some with several, planes with faces on both sides and planes that cut nothing, contacts strictly
inside the step, and on jitter's dense frame a block that overflows its shard in a frame with more than twice the rows of the last."""
from __future__ import annotations

import numpy as np
import pytest

import box_ref as bx
import moving_inputs as mi
import nearest_ref as nr
import nearest_self_ref as ns
import oracle
import plane_ref as plr
import proximity_ref as pr
import scale_inputs as si
import segment_ref as sg
import sweep_ref as sw
import swept_ref as sr
import within_ref as wn
import witness_ref as wr


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _share(a, b):
    """The part of the union of two pair sets that is in one of them only."""
    return np.setxor1d(a, b).size / max(1, np.union1d(a, b).size)


def test_every_sequence_has_the_frames_triangles_and_queries_the_gpu_tests_rely_on():
    assert set(mi.LARGE) == {"jitter", "slide", "scale_walk", "frame_exit", "float_double", "collapse"}
    assert mi.NQ % 64 != 0 and mi.NQ > 64 and mi.NQ >= 500
    for name in mi.NAMES:
        s = mi.seq(name)
        if name in mi.LARGE:
            assert 6 <= len(s) <= 8 and 1000 <= s.nt <= 10_000, (name, len(s), s.nt)       # (more than one 512-leaf block of the build)
        else:
            assert len(s) == 4 and s.nt in mi.TINY
        assert mi.rays(name, 1).shape == (mi.NQ, 7) and mi.points(name, 1).shape == (mi.NQ, 3)
        print(f"{name}: {len(s)} frames, {s.nt} triangles, {mi.NQ} rays and {mi.NQ} points a frame, seed {s.seed}, edge {s.edge:g}")


@pytest.mark.parametrize("name", mi.NAMES)
def test_consecutive_frames_have_different_right_answers(name):
    s = mi.seq(name)
    tiny = name not in mi.LARGE
    low = dict(rays=1.0, points=1.0, prox=1.0, ccd=1.0)
    for f in range(1, len(s)):
        r0, r1 = mi.want_rays(name, f - 1), mi.want_rays(name, f)
        p0, p1 = mi.want_points_r(name, f - 1), mi.want_points_r(name, f)
        dr = float(((r0[0] != r1[0]) | (_bits(r0[2]) != _bits(r1[2]))).mean())
        dp = float(((p0[0] != p1[0]) | (_bits(p0[2]) != _bits(p1[2]))).mean())
        assert dr >= 0.25 and dp >= 0.25, (name, f, dr, dp)
        low["rays"], low["points"] = min(low["rays"], dr), min(low["points"], dp)
        if not tiny:
            dx = _share(oracle.pair_set(mi.want_prox(name, f - 1)[0]), oracle.pair_set(mi.want_prox(name, f)[0]))
            dc = _share(oracle.pair_set(mi.want_ccd(name, f - 1)[0][0]), oracle.pair_set(mi.want_ccd(name, f)[0][0]))
            assert dx >= 0.10 and dc >= 0.10, (name, f, dx, dc)
            assert mi.want_prox(name, f)[0].shape[0] > 0 and mi.want_ccd(name, f)[0][0].shape[0] > 0
            low["prox"], low["ccd"] = min(low["prox"], dx), min(low["ccd"], dc)
        # the order: a jitter can leave one, two or three triangles in the order they had, so the condition is on the meshes with an order to lose
        if s.nt >= 63:
            assert not np.array_equal(mi.want_step(name, f - 1)["perm"], mi.want_step(name, f)["perm"]), (name, f)
    print(f"{name}: smallest share that changes between consecutive frames: " + ", ".join(f"{k} {v:.2f}" for k, v in low.items() if not (tiny and k in ("prox", "ccd"))))


def _exponent(v):
    return int(np.frexp(np.abs(v).max())[1])


def test_scale_walk_walks_the_scale():
    s = mi.seq("scale_walk")
    ex = [_exponent(v) for v in s.frames]
    d = np.sign(np.diff(ex))
    assert (d > 0).any() and (d < 0).any() and np.flatnonzero(d > 0)[0] < np.flatnonzero(d < 0)[0], ex
    assert all(min(si.SCALES) <= k <= max(si.SCALES) for k in mi.SCALE_WALK_K)
    assert ex[mi.SCALE_WALK_OFFSET_FRAME] == 21 and ex[mi.SCALE_WALK_OFFSET_FRAME + 1] < 21 and ex[mi.SCALE_WALK_OFFSET_FRAME - 1] < 21
    # M and the root box follow
    m = [sr.m_bits(v, mi.x1("scale_walk", f), s.vidx) for f, v in enumerate(s.frames)]
    box = [float(np.abs(mi.want_root_box("scale_walk", f)).max()) for f in range(len(s))]
    for q in (m, box):
        d = np.sign(np.diff(np.asarray(q, dtype=np.float64)))
        assert (d > 0).any() and (d < 0).any(), q


def test_float_double_alternates():
    s = mi.seq("float_double")
    for f, v in enumerate(s.frames):
        same = np.array_equal(v.astype(np.float32).astype(np.float64), v)
        assert same == (f % 2 == 0), f


def test_collapse_puts_every_centroid_in_one_cell():
    s = mi.seq("collapse")
    for f in range(len(s)):
        k = np.unique(mi.want_step("collapse", f)["keys"]).size
        assert (k == 1) == (f in mi.COLLAPSE_FRAMES), (f, k)
        assert f in mi.COLLAPSE_FRAMES or k > s.nt // 2
    assert 0 < min(mi.COLLAPSE_FRAMES) and max(mi.COLLAPSE_FRAMES) < len(s) - 1                 # ... and back out


def test_frame_exit_leaves_the_frame_and_returns():
    s = mi.seq("frame_exit")
    above = [int((mi.want_step("frame_exit", f)["keys"] >> np.uint64(60)).max()) > 0 for f in range(len(s))]   # (as test_cd_gpu.py tells a key beyond the sort's digits)
    assert above == [f in mi.FRAME_EXIT_OUT for f in range(len(s))], above
    assert not above[0] and not above[-1] and not above[-2]


def test_jitter_stays_inside_the_frame_and_its_dense_frame_overflows_a_shard():
    s = mi.seq("jitter")
    for f in range(len(s)):
        assert int((mi.want_step("jitter", f)["keys"] >> np.uint64(60)).max()) == 0, f
    loads = [mi.ccd_shard_load("jitter", f) for f in range(len(s))]
    print("jitter: the fullest shard of the CCD candidate buffer, frame by frame:", loads, "of", mi.SHARD_FIRST)
    assert loads[mi.JITTER_DENSE_FRAME] > mi.SHARD_FIRST and max(loads[:mi.JITTER_DENSE_FRAME]) <= mi.SHARD_FIRST
    assert all(x < loads[mi.JITTER_DENSE_FRAME] // 4 for x in loads[mi.JITTER_DENSE_FRAME + 1:])     # sparse again afterwards


# ---------------------------------------------------------------- the helpers can fail
def _fake_any(want):
    """An any-hit / any-within answer a correct device may give: the closest one's face."""
    return want[0].copy(), int((want[0] != mi.MISS).sum())


@pytest.mark.parametrize("name", ["jitter", "slide", "scale_walk", "collapse", "tiny2", "tiny65"])
def test_every_comparison_raises_on_the_previous_frames_result(name):
    s = mi.seq(name)
    for f in range(1, len(s)):
        v, v0 = s.frames[f], s.frames[f - 1]
        what = f"{name} frame {f}"
        # each helper passes on the frame's own expected result ...
        mi.same_rays(mi.want_rays(name, f), mi.want_rays(name, f), what)
        mi.same_points(mi.want_points_r(name, f), mi.want_points_r(name, f), what)
        mi.same_any_hit(*_fake_any(mi.want_rays(name, f)), mi.rays(name, f), v, s.vidx, mi.want_rays(name, f), what)
        mi.same_any_within(*_fake_any(mi.want_points_r(name, f)), mi.points(name, f), mi.radii(name, f), v, s.vidx, mi.want_points_r(name, f), what)
        wp, (wc, counts) = mi.want_prox(name, f), mi.want_ccd(name, f)
        mi.same_prox((wp[0], wp[1], wp[0].shape[0], 0), wp, what)
        mi.same_ccd((wc[0], wc[1], wc[2], wc[0].shape[0], 0), wc, what)
        t = mi.want_swept(name, f)
        mi.same_swept(t, v, mi.x1(name, f), s.vidx, t["m_bits"], mi.ccd_dist(name, f), what, n_candidates=mi.want_candidates(name, f))
        mi.same_root_box(mi.want_root_box(name, f), mi.want_root_box(name, f), what)
        st = mi.want_step(name, f)
        mi.same_step(st["pairs"], st["stats"].n_pairs, 0, st["stats"].pairs_tested, st, what)
        pw, cw, ct = mi.want_prox_witness(name, f), mi.want_ccd_witness(name, f), mi.want_contour(name, f)
        plain_p, plain_c = (wp[0], wp[1], wp[0].shape[0], 0), (wc[0], wc[1], wc[2], wc[0].shape[0], 0)
        mi.same_witness(mi.witness_call(pw), pw, what)
        mi.same_witness(mi.witness_call(cw), cw, what)
        mi.same_as_plain(mi.witness_call(pw)[:4], plain_p, what)            # (the restatements agree: the witness rows are the plain calls' pairs)
        mi.same_as_plain(mi.witness_call(cw)[:5], plain_c, what)
        mi.same_contour(mi.contour_call(ct), ct, what, ct.tested)
        mi.same_pair_set(ct.pairs, st["pairs"], what)
        # ... and raises on the one before it
        pw0, cw0, ct0 = mi.want_prox_witness(name, f - 1), mi.want_ccd_witness(name, f - 1), mi.want_contour(name, f - 1)
        if pw0.faces.shape[0] or pw.faces.shape[0]:
            with pytest.raises(AssertionError):
                mi.same_witness(mi.witness_call(pw0), pw, what)
            with pytest.raises(AssertionError):
                mi.same_as_plain(mi.witness_call(pw0)[:4], plain_p, what)
        if cw0.faces.shape[0] or cw.faces.shape[0]:
            with pytest.raises(AssertionError):
                mi.same_witness(mi.witness_call(cw0), cw, what)
            with pytest.raises(AssertionError):
                mi.same_as_plain(mi.witness_call(cw0)[:5], plain_c, what)
        if ct0.faces.shape[0] or ct.faces.shape[0]:
            with pytest.raises(AssertionError):
                mi.same_contour(mi.contour_call(ct0), ct, what)
            with pytest.raises(AssertionError):
                mi.same_pair_set(ct0.pairs, st["pairs"], what)
        if ct0.tested != ct.tested:
            with pytest.raises(AssertionError):                                 # this frame's rows with the previous frame's n_tested
                mi.same_contour(mi.contour_call(ct), ct, what, ct0.tested)
        with pytest.raises(AssertionError):
            mi.same_rays(mi.want_rays(name, f - 1), mi.want_rays(name, f), what)
        with pytest.raises(AssertionError):
            mi.same_points(mi.want_points_r(name, f - 1), mi.want_points_r(name, f), what)
        with pytest.raises(AssertionError):                                     # the previous frame's faces against this frame's rays and mesh
            mi.same_any_hit(*_fake_any(mi.want_rays(name, f - 1)), mi.rays(name, f), v, s.vidx, mi.want_rays(name, f), what)
        with pytest.raises(AssertionError):
            mi.same_any_within(*_fake_any(mi.want_points_r(name, f - 1)), mi.points(name, f), mi.radii(name, f), v, s.vidx, mi.want_points_r(name, f), what)
        wp0, (wc0, counts0) = mi.want_prox(name, f - 1), mi.want_ccd(name, f - 1)
        if wp0[0].shape[0] or wp[0].shape[0]:
            with pytest.raises(AssertionError):
                mi.same_prox((wp0[0], wp0[1], wp0[0].shape[0], 0), wp, what)
        if wc0[0].shape[0] or wc[0].shape[0]:
            with pytest.raises(AssertionError):
                mi.same_ccd((wc0[0], wc0[1], wc0[2], wc0[0].shape[0], 0), wc, what)
        t0 = mi.want_swept(name, f - 1)
        with pytest.raises(AssertionError):                                     # the previous frame's swept tree, M and pad
            mi.same_swept(t0, v, mi.x1(name, f), s.vidx, t["m_bits"], mi.ccd_dist(name, f), what)
        if t0["m_bits"] != t["m_bits"]:                                      # (slide: sheet A holds the largest coordinate in every frame)
            with pytest.raises(AssertionError):                                 # this frame's records under the previous frame's M alone
                mi.same_swept(dict(t, m_bits=t0["m_bits"], pad=t0["pad"]), v, mi.x1(name, f), s.vidx, t["m_bits"], mi.ccd_dist(name, f), what)
        with pytest.raises(AssertionError):
            mi.same_root_box(mi.want_root_box(name, f - 1), mi.want_root_box(name, f), what)
        st0 = mi.want_step(name, f - 1)
        if st0["stats"].n_pairs or st["stats"].n_pairs:
            with pytest.raises(AssertionError):
                mi.same_step(st0["pairs"], st0["stats"].n_pairs, 0, st0["stats"].pairs_tested, st, what)


@pytest.mark.parametrize("name", mi.NAMES)
def test_item_row_comparisons_raise_on_the_previous_frames_result(name):
    """cd_points_within, cd_cast_rays_all, cd_sweep_points_all and cd_sweep_points: same_item_rows and same_first_contact pass on the
    frame's own restatement and raise on the one of the frame before it, in every frame of every sequence."""
    s = mi.seq(name)
    for f in range(1, len(s)):
        what = f"{name} frame {f}"
        n = mi.sweep_items(name, f).shape[0]
        sets = [(mi.want_within(name, f - 1), mi.want_within(name, f)), (mi.want_rays_all(name, f - 1), mi.want_rays_all(name, f)),
                (mi.want_sweep(name, f - 1)[0], mi.want_sweep(name, f)[0]), (mi.want_sweep_still(name, f - 1)[0], mi.want_sweep_still(name, f)[0])]
        if name in mi.SELF_SWEEP:
            sets.append((mi.want_self_sweep(name, f - 1)[0], mi.want_self_sweep(name, f)[0]))
        for w0, w1 in sets:
            mi.same_item_rows(mi.item_call(w1), w1, what)
            mi.same_item_rows(mi.item_call(w1), mi.item_rows(mi.item_call(w1)), what)      # (the form the fresh context's result is compared in)
            if w0.rows.shape[0] or w1.rows.shape[0]:
                with pytest.raises(AssertionError):
                    mi.same_item_rows(mi.item_call(w0), w1, what)
            with pytest.raises(AssertionError):                                 # the return code
                mi.same_item_rows(mi.item_call(w1, rc=1), w1, what)
        w0, w1 = mi.want_sweep(name, f - 1)[0], mi.want_sweep(name, f)[0]
        mi.same_first_contact(mi.first_contact_call(w1, n), w1, n, what)
        if w0.rows.shape[0] or w1.rows.shape[0]:
            with pytest.raises(AssertionError):
                mi.same_first_contact(mi.first_contact_call(w0, mi.sweep_items(name, f - 1).shape[0]), w1, n, what)
        assert mi.want_sweep(name, f - 1)[1] != mi.want_sweep(name, f)[1], what     # ... and so do the counts compared beside the rows
    # the swept rows depend on the end positions: the same items against the mesh at rest are another row set
    assert any(mi.want_sweep(name, f)[0].rows.shape != mi.want_sweep_still(name, f)[0].rows.shape
               or not np.array_equal(mi.want_sweep(name, f)[0].toi, mi.want_sweep_still(name, f)[0].toi) for f in range(len(s))), name


def test_one_corrupted_field_of_an_item_row_raises():
    """The right frame's rows with one bit of one value, one ID, or one face of one row changed; one row dropped; a first contact that
    is the item's SECOND row."""
    name, f = "jitter", 1
    for rows in (mi.want_within(name, f), mi.want_rays_all(name, f), mi.want_sweep(name, f)[0]):
        k = rows.rows.shape[0] // 2
        for field in rows._fields[1:]:
            bad = _copy(rows)
            a = getattr(bad, field)
            if a.dtype == np.float64:
                _flip_lowest_bit(a.reshape(a.shape[0], -1), (k, 0))
            else:
                a[k] ^= 1
            with pytest.raises(AssertionError):
                mi.same_item_rows(mi.item_call(bad), rows, field)
        bad = _copy(rows)
        bad.rows[k, 1] ^= 1
        with pytest.raises(AssertionError):
            mi.same_item_rows(mi.item_call(bad), rows, "face")
        with pytest.raises(AssertionError):
            mi.same_item_rows(mi.item_call(type(rows)(*(np.delete(a, k, axis=0) for a in rows))), rows, "a row less")
    rows, n = mi.want_sweep(name, f)[0], mi.sweep_items(name, f).shape[0]
    first = sw.first_of(rows, n)
    item = int(np.flatnonzero(wn.rows_per_item(rows, n) >= 2)[0])
    rest = type(rows)(*(a[~((rows.rows[:, 0] == item) & (rows.rows[:, 1] == first[0][item]))] for a in rows))     # the rows without that item's first
    with pytest.raises(AssertionError):
        mi.same_first_contact(mi.first_contact_call(rest, n), rows, n, "the second row")
    got = mi.first_contact_call(rows, n)
    with pytest.raises(AssertionError):                                         # n_found alone
        mi.same_first_contact(got[:8] + (mi.mi355cd.CdPointInfo(got[8].n_found + 1, 0, 0),), rows, n, "n_found")


@pytest.mark.parametrize("name", mi.LARGE)
def test_item_queries_have_items_without_rows_and_items_with_several(name):
    """Per sequence, pooled over its frames (F frames of n items): at least F n / 8 items with no row and at least F n / 16 with two or
    more, for each of the three row sets; at least 4 swept rows with 0 < toi < 1; nothing unresolved."""
    s = mi.seq(name)
    none, several, items = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
    inside = unresolved = 0
    for f in range(len(s)):
        sweep, counts = mi.want_sweep(name, f)
        for k, (rows, n) in enumerate(((mi.want_within(name, f), mi.within_items(name, f)[0].shape[0]), (mi.want_rays_all(name, f), mi.NQ),
                                       (sweep, mi.sweep_items(name, f).shape[0]))):
            c = wn.rows_per_item(rows, n)
            none[k] += (c == 0).sum(); several[k] += (c >= 2).sum(); items[k] += n
        inside += int(((sweep.toi > 0) & (sweep.toi < 1)).sum())
        unresolved += counts[2] + mi.want_sweep_still(name, f)[1][2]
        if name in mi.SELF_SWEEP:
            own, own_counts = mi.want_self_sweep(name, f)
            assert own.rows.shape[0] > 100 and own_counts[2] == 0 and ((own.toi > 0) & (own.toi < 1)).sum() >= 4, (name, f)
            assert not (s.vidx[own.rows[:, 1]] == own.rows[:, 0:1]).any()       # no face of the vertex itself
        r = mi.within_items(name, f)[1]
        assert np.isinf(r[:mi.NQ:mi.INF_EVERY]).all() and (wn.rows_per_item(mi.want_within(name, f), r.shape[0])[:mi.NQ:mi.INF_EVERY] == s.nt).all()
        d = mi.sweep_items(name, f)[:mi.NQ, 6]
        assert len({*d[0:3]}) == 3 and (d[3:] == d[:-3]).all()                 # three dists, by i % 3
    print(f"{name}: (all within, every hit, swept points) items with no row {none.tolist()}, with several {several.tolist()}, of {items.tolist()}; "
          f"{inside} swept rows with 0 < toi < 1")
    assert (none * 8 >= items).all() and (several * 16 >= items).all(), (name, none, several, items)
    assert inside >= 4 and unresolved == 0, (name, inside, unresolved)


def test_tiny_sequences_have_item_rows_in_some_frame():
    for n in mi.TINY:
        name = f"tiny{n}"
        rows = [(mi.want_within(name, f).rows.shape[0], mi.want_rays_all(name, f).rows.shape[0], mi.want_sweep(name, f)[0].rows.shape[0])
                for f in range(len(mi.seq(name)))]
        print(f"{name}: (all within, every hit, swept points) rows a frame: {rows}")
        assert all(max(r[k] for r in rows) > 0 for k in range(3)), (name, rows)


def test_the_growth_block_has_more_rows_than_a_shard_of_the_first_candidate_buffer():
    """Items GROWTH_AT .. GROWTH_AT + 63 of jitter's dense frame are ONE block of the descent (one shard), and their rows alone -- rows
    never exceed candidates -- are more than the shard's first WITHIN_SHARD_FIRST slots: the pass must grow its buffer and run again.
    A condition on the inputs; the restatement gives 18 325 all-within rows and 18 842 swept rows."""
    f = mi.JITTER_DENSE_FRAME
    assert mi.GROWTH_AT % 64 == 0 and mi.GROWTH_ITEMS == 64 and mi.GROWTH_AT >= mi.NQ
    pts, r = mi.within_items("jitter", f)
    it = mi.sweep_items("jitter", f)
    assert pts.shape[0] == it.shape[0] == mi.GROWTH_AT + mi.GROWTH_ITEMS
    figures = []
    for rows in (mi.want_within("jitter", f), mi.want_sweep("jitter", f)[0], mi.want_sweep_still("jitter", f)[0]):
        blk = int((rows.rows[:, 0] >= mi.GROWTH_AT).sum())
        fill = int(((rows.rows[:, 0] >= mi.NQ) & (rows.rows[:, 0] < mi.GROWTH_AT)).sum())
        figures.append(blk)
        assert blk > mi.mi355cd.WITHIN_SHARD_FIRST and fill == 0, (blk, fill)
    print("jitter's growth block: rows (all within, swept points, swept points at rest)", figures, "of", mi.mi355cd.WITHIN_SHARD_FIRST, "slots")
    for g in range(len(mi.seq("jitter"))):                                      # no other frame has the block: its buffers stay as the dense frame left them
        assert (mi.within_items("jitter", g)[0].shape[0] == mi.NQ) == (mi.sweep_items("jitter", g).shape[0] == mi.NQ) == (g != f)


# ---------------------------------------------------------------- the mesh against itself and points inside it
def _found(res):
    return res[0].faces[:, 0] != ns.NONE


@pytest.mark.parametrize("name", mi.NAMES)
def test_nearest_self_and_inside_comparisons_raise_on_the_previous_frames_result(name):
    """cd_nearest_self (rows and CD_NEAREST_MIN, at an edge and at +inf) and cd_points_inside (three axes, and parity): same_nearest_self
    and same_inside pass on the frame's own restatement and raise on the one of the frame before it.  cd_signed_distance is held to
    want_inside's first array, so the same holds for it."""
    s = mi.seq(name)
    min_rows_that_change = 0
    for f in range(1, len(s)):
        what = f"{name} frame {f}"
        sets = [(mi.want_nearest_self(name, f - 1), mi.want_nearest_self(name, f))]
        before = [k for k in range(f) if mi.has_nearest_self_inf(name, k)]     # (the last frame before this one that has the rows at +inf)
        if mi.has_nearest_self_inf(name, f) and before:
            sets.append((mi.want_nearest_self_inf(name, before[-1]), mi.want_nearest_self_inf(name, f)))
        for w0, w1 in sets:
            mi.same_nearest_self(mi.nearest_self_call(w1), w1, what)
            mi.same_nearest_self(mi.nearest_self_call(ns.nearest_min(w1)), ns.nearest_min(w1), what)
            if _found(w0).any() or _found(w1).any():                            # (tiny1 has no pair at all)
                with pytest.raises(AssertionError):
                    mi.same_nearest_self(mi.nearest_self_call(w0), w1, what)
            # the MIN row of a mesh in contact is the pair in contact with the smallest IDs, with no witness: the same row in both frames
            # where that pair stays in contact
            m0, m1 = ns.nearest_min(w0), ns.nearest_min(w1)
            if any(x.tobytes() != y.tobytes() for x, y in zip(m0[0] + (m0[1],), m1[0] + (m1[1],))):
                min_rows_that_change += 1
                with pytest.raises(AssertionError):
                    mi.same_nearest_self(mi.nearest_self_call(m0), m1, what)
        for axis, parity in ((0, False), (1, False), (2, False), ((f + s.seed) % 3, True)):
            w0, w1 = mi.want_inside(name, f - 1, axis, parity), mi.want_inside(name, f, axis, parity)
            assert mi.inside_points(name, f, axis).shape == mi.inside_points(name, f - 1, axis).shape
            mi.same_inside(mi.inside_call(w1), w1, what)
            crossed = lambda w: int(((w[1] + w[2]) > 0).sum())
            if name in mi.LARGE or crossed(w0) + crossed(w1) >= 8:              # (a handful of triangles: few of the points have one over them)
                with pytest.raises(AssertionError):
                    mi.same_inside(mi.inside_call(w0), w1, what)
                with pytest.raises(AssertionError):                             # the first array alone: what the signed distance is held to
                    assert np.array_equal(w0[0], w1[0])
    assert min_rows_that_change > 0 or s.nt == 1, name


def test_one_corrupted_field_of_a_nearest_self_row_or_an_inside_count_raises():
    name, f = "collapse", 1
    res = mi.want_nearest_self(name, f)
    k = int(np.flatnonzero(_found(res) & (res[0].feature != wr.FEATURE_NONE).all(axis=1))[100])
    for field, bad in _corrupted_nearest(res[0], k).items():
        with pytest.raises(AssertionError):
            mi.same_nearest_self(mi.nearest_self_call((bad, res[1])), res, field)
    played = res[1].copy()
    played[k] = played[k, ::-1]
    with pytest.raises(AssertionError):
        mi.same_nearest_self(mi.nearest_self_call((res[0], played)), res, "played faces exchanged")
    with pytest.raises(AssertionError):                                         # n_found alone
        mi.same_nearest_self(mi.nearest_self_call(res)._replace(info=mi.mi355cd.CdNearestInfo(0, 0, 0)), res, "n_found")
    want = mi.want_inside(name, f, 1)
    k = int(np.flatnonzero(want[1] > 0)[10])
    for j in range(5):
        bad = [a.copy() for a in want]
        bad[j][k] = not bad[j][k] if j == 0 else bad[j][k] + 1
        with pytest.raises(AssertionError):
            mi.same_inside(mi.inside_call(bad), want, j)
    with pytest.raises(AssertionError):                                         # n_inside alone
        mi.same_inside(want + (mi.mi355cd.CdInsideInfo(int(want[0].sum()) + 1, 0, 0),), want, "n_inside")


def test_reduced_proximity_rows_are_the_all_pairs_rows_within_the_radius():
    """want_nearest_self -- the proximity witness restatement at one edge, reduced per face -- is nearest_self_ref.within of the brute
    force over every admissible pair, column by column, on every frame that has the brute force; and its minimum is the clearance
    wherever it finds a row (what the GPU test takes for CD_NEAREST_MIN at +inf on the other frames)."""
    frames = [(name, f) for name in mi.NAMES for f in range(len(mi.seq(name))) if mi.has_nearest_self_inf(name, f)]
    assert sum(name in mi.LARGE for name, f in frames) == 4 and len(frames) == 4 + 4 * len(mi.TINY)
    assert all(mi.seq(name).nt <= 1000 for name, f in frames)
    assert mi.SCALE_WALK_K[mi.NEAREST_SELF_INF["scale_walk"][0]] == 60 and mi.NEAREST_SELF_INF["scale_walk"][1] == mi.SCALE_WALK_OFFSET_FRAME
    assert mi.NEAREST_SELF_INF["collapse"] == (mi.COLLAPSE_FRAMES[0], mi.COLLAPSE_FRAMES[0] + 1)
    for name, f in frames:
        every, got = mi.want_nearest_self_inf(name, f), mi.want_nearest_self(name, f)
        want = ns.within(every, mi.nearest_self_r(name, f))
        for k, x, y in zip(every[0]._fields + ("played",), got[0] + (got[1],), want[0] + (want[1],)):
            mi._same_bytes(x, y, (name, f, k))
        if _found(got).any():
            mi.same_nearest_self(mi.nearest_self_call(ns.nearest_min(got)), ns.nearest_min(every), (name, f))


def test_nearest_self_and_inside_references_cannot_pass_vacuously():
    """Conditions, for every LARGE sequence, frame and axis: of the about 1300 inside points at least 200 have a face over or under
    them and at least 100 are inside; at least 30 of the under-vertex points are covered by a face with an exact zero of E (the tie
    rule decided); want_nearest_self finds a partner for at least half of the rows."""
    low = dict(crossed=(1 << 30,), inside=(1 << 30,), ties=(1 << 30,), partner=(2.0,))
    for name in mi.LARGE:
        s = mi.seq(name)
        for f in range(len(s)):
            found = int(_found(mi.want_nearest_self(name, f)).sum())
            assert 2 * found >= s.nt, (name, f, found)
            low["partner"] = min(low["partner"], (found / s.nt, found, s.nt, name, f))
            for axis in range(3):
                p = mi.inside_points(name, f, axis)
                inside, na, nb, wa, wb = mi.want_inside(name, f, axis)
                crossed, ties = int(((na + nb) > 0).sum()), mi.inside_tie_covers(name, f, axis)
                assert mi.NQ + 250 <= p.shape[0] <= mi.NQ + 350 and np.array_equal(p[:mi.NQ], mi.points(name, f)), (name, f, axis)
                under = p[mi.NQ:]
                v = s.frames[f][::max(1, s.frames[f].shape[0] // mi.UNDER_VERTICES)]
                rest = [a for a in range(3) if a != axis]
                assert np.array_equal(_bits(under[:, rest]), _bits(v[:, rest])) and (under[:, axis] < v[:, axis]).all(), (name, f, axis)
                assert crossed >= 200 and int(inside.sum()) >= 100 and ties >= 30, (name, f, axis, crossed, int(inside.sum()), ties)
                for k, x in (("crossed", crossed), ("inside", int(inside.sum())), ("ties", ties)):
                    low[k] = min(low[k], (x, name, f, axis))
    print("the smallest over every LARGE sequence, frame and axis:", low)
    v, f0 = mi.want_inside("jitter", 1, 1, True), mi.want_inside("jitter", 1, 1)     # parity is another answer on these open meshes
    assert not np.array_equal(v[0], f0[0]) and all(np.array_equal(a, b) for a, b in zip(v[1:], f0[1:]))


def test_tiny_sequences_have_nearest_self_rows_and_crossings_in_some_frame():
    for n in mi.TINY:
        name = f"tiny{n}"
        frames = range(len(mi.seq(name)))
        rows = [int(_found(mi.want_nearest_self_inf(name, f)).sum()) for f in frames]
        crossed = [sum(int(((w[1] + w[2]) > 0).sum()) for w in (mi.want_inside(name, f, axis) for axis in range(3))) for f in frames]
        print(f"{name}: nearest-self rows with a partner a frame {rows}, inside points with a face over or under them (three axes) {crossed}")
        assert rows == [0 if n == 1 else n] * len(frames) and max(crossed) > 0, (name, rows, crossed)


def test_between_comparisons_raise_on_the_previous_frames_result():
    for schedule in mi.BETWEEN_SCHEDULES:
        for f in range(1, 3):
            w0, w1 = mi.want_between(schedule, f - 1), mi.want_between(schedule, f)
            what = f"{schedule} frame {f}"
            c, p, q = w1["contact"][0], w1["prox"], w1["ccd"]
            mi.same_between_contact((c, c.shape[0], 0), c, what)
            mi.same_between_prox((p[0], p[1], p[0].shape[0], 0), p, what)
            mi.same_between_ccd((q[0], q[1], q[2], q[0].shape[0], 0), q, what)
            c0, p0, q0 = w0["contact"][0], w0["prox"], w0["ccd"]
            assert (c.shape[0] > 0 or schedule == mi.APART) and p[0].shape[0] > 0 and q[0].shape[0] > 0
            if schedule != mi.APART:                                            # (sheets that do not touch: no pairs in contact in either frame)
                with pytest.raises(AssertionError):
                    mi.same_between_contact((c0, c0.shape[0], 0), c, what)
            with pytest.raises(AssertionError):
                mi.same_between_prox((p0[0], p0[1], p0[0].shape[0], 0), p, what)
            with pytest.raises(AssertionError):
                mi.same_between_ccd((q0[0], q0[1], q0[2], q0[0].shape[0], 0), q, what)
            for k in ("prox_witness", "ccd_witness"):
                assert w1[k].faces.shape[0] > 0, (what, k)
                mi.same_witness(mi.witness_call(w1[k]), w1[k], what)
                with pytest.raises(AssertionError):
                    mi.same_witness(mi.witness_call(w0[k]), w1[k], what)
            mi.same_as_plain(mi.witness_call(w1["prox_witness"])[:4], (p[0], p[1], p[0].shape[0], 0), what)
            mi.same_contour(mi.contour_call(w1["contour"]), w1["contour"], what, w1["contour"].tested)
            mi.same_between_contact(mi.contour_call(w1["contour"])[:3], c, what)
            if schedule != mi.APART:
                with pytest.raises(AssertionError):
                    mi.same_contour(mi.contour_call(w0["contour"]), w1["contour"], what)
                assert w0["contour"].tested != w1["contour"].tested
                with pytest.raises(AssertionError):                             # this frame's rows with the previous frame's n_tested
                    mi.same_contour(mi.contour_call(w1["contour"]), w1["contour"], what, w0["contour"].tested)
            for k in ("near", "near_q", "near_min", "near_q_min"):
                mi.same_nearest(mi.nearest_call(w1[k]), w1[k], what)
                with pytest.raises(AssertionError):
                    mi.same_nearest(mi.nearest_call(w0[k]), w1[k], what)


# ---------------------------------------------------------------- one field of the right frame's rows
def _copy(rows):
    return type(rows)(*(x.copy() if isinstance(x, np.ndarray) else x for x in rows))


def _flip_lowest_bit(a, at):
    a.view(np.uint64)[at] ^= np.uint64(1)


def _corrupted_witness(rows, k):
    """name -> a copy of witness_ref's Rows with ONE field of row k changed."""
    out = {}
    for name, at in (("bary", (k, 1, 0)), ("points", (k, 0, 2)), ("dists", (k,))) + ((("toi", (k,)),) if rows.toi is not None else ()):
        out[name + " bit"] = r = _copy(rows)
        _flip_lowest_bit(getattr(r, name), at)
    out["feature code"] = r = _copy(rows)
    r.feature[k, 0] = (int(r.feature[k, 0]) + 1) % 7
    out["faces swapped within the pair"] = r = _copy(rows)
    r.faces[k] = r.faces[k, ::-1]
    out["pair"] = r = _copy(rows)
    r.pairs[k, 1] ^= 1
    return out


def _corrupted_contour(rows, k):
    out = {}
    for name, at in (("param", (k, 1)), ("points", (k, 5))):
        out[name + " bit"] = r = _copy(rows)
        _flip_lowest_bit(getattr(r, name), at)
    out["endpoint code"] = r = _copy(rows)
    r.code[k, 0] ^= 8                                                           # the side bit of endpoint 0
    out["mask"] = r = _copy(rows)
    r.code[k, 2] ^= 1
    out["faces swapped within the pair"] = r = _copy(rows)
    r.faces[k] = r.faces[k, ::-1]
    out["pair"] = r = _copy(rows)
    r.pairs[k, 1] ^= 1
    return out


def _second_nearest(rows, k, place):
    """rows with row k replaced by a's face k against the SECOND nearest triangle of b, with that pair's own distance and witness."""
    wa, ia, _, wb, ib, _ = mi._roles(place, False)
    nb = ib.shape[0]
    tri = np.concatenate([np.repeat(wa[ia[k].astype(np.int64)][None], nb, axis=0), wb[ib.astype(np.int64)]], axis=1)
    d = pr.tri_distance_np(tri)
    o = np.lexsort((np.arange(nb), d))
    assert o[0] == rows.faces[k, 1] and d[o[0]] == rows.dist[k]
    j = int(o[1])
    w = wr.tri_witness_np(tri[j:j + 1])
    r = _copy(rows)
    r.faces[k], r.ids[k], r.dist[k], r.points[k], r.bary[k], r.feature[k] = (k, j), (k, j), d[j], w.points[0], w.bary[0], w.feature[0]
    return r


def _corrupted_nearest(rows, k, place=None):
    out = {}
    for name, at in (("bary", (k, 0, 1)), ("points", (k, 1, 0)), ("dist", (k,))):
        out[name + " bit"] = r = _copy(rows)
        _flip_lowest_bit(getattr(r, name), at)
    out["feature code"] = r = _copy(rows)
    r.feature[k, 1] = (int(r.feature[k, 1]) + 1) % 7
    out["faces swapped within the pair"] = r = _copy(rows)
    r.faces[k] = r.faces[k, ::-1]
    out["id"] = r = _copy(rows)
    r.ids[k, 1] ^= 1
    if place is not None:
        out["the second nearest triangle"] = _second_nearest(rows, k, place)
    return out


def test_every_new_comparison_raises_on_one_corrupted_field():
    """The right frame's rows with one field of one row changed: one bit of a barycentric, a point, a distance, a toi or a parameter,
    one feature or endpoint code, the two faces of one pair exchanged, one ID, one nearest row replaced by the second nearest triangle's."""
    name, f, schedule = "jitter", 1, "both_move"
    place = mi.between_place(schedule, f)
    w = mi.want_between(schedule, f)
    for what, rows in (("proximity", mi.want_prox_witness(name, f)), ("ccd", mi.want_ccd_witness(name, f)), ("between proximity", w["prox_witness"]),
                       ("between ccd", w["ccd_witness"])):
        ok = np.flatnonzero((rows.feature != wr.FEATURE_NONE).all(axis=1) & (rows.faces[:, 0] != rows.faces[:, 1]))     # (rows with a witness to corrupt)
        k = int(ok[ok.size // 2])
        for field, bad in _corrupted_witness(rows, k).items():
            with pytest.raises(AssertionError):
                mi.same_witness(mi.witness_call(bad), rows, (what, field))
        with pytest.raises(AssertionError):                                     # the return code
            mi.same_witness(mi.witness_call(rows, rc=1), rows, what)
    for what, rows in (("contour", mi.want_contour(name, f)), ("between contour", w["contour"])):
        k = rows.faces.shape[0] // 2
        for field, bad in _corrupted_contour(rows, k).items():
            with pytest.raises(AssertionError):
                mi.same_contour(mi.contour_call(bad), rows, (what, field))
        with pytest.raises(AssertionError):
            mi.same_contour(mi.contour_call(rows, rc=1), rows, what)
    rows = w["near"]
    k = int(np.flatnonzero((rows.faces[:, 0] != nr.NONE) & (rows.feature[:, 1] != wr.FEATURE_NONE))[rows.faces.shape[0] // 3])
    for field, bad in _corrupted_nearest(rows, k, place).items():
        with pytest.raises(AssertionError):
            mi.same_nearest(mi.nearest_call(bad), rows, ("nearest", field))
    least = mi.want_between(mi.APART, f)["near_min"]                            # (sheets that do not touch: a row with a witness)
    assert (least.feature != wr.FEATURE_NONE).all()
    for field, bad in _corrupted_nearest(least, 0).items():
        with pytest.raises(AssertionError):
            mi.same_nearest(mi.nearest_call(bad), least, ("nearest MIN", field))
    with pytest.raises(AssertionError):                                         # n_found alone
        mi.same_nearest(mi.nearest_call(rows)._replace(info=mi.mi355cd.CdNearestInfo(0, 0, 0)), rows, "nearest")


# ---------------------------------------------------------------- the new references are not empty, and the sheets that do not touch
def test_witness_and_contour_references_have_rows_in_every_frame_of_the_large_sequences():
    for name in mi.LARGE:
        n = [(mi.want_prox_witness(name, f).faces.shape[0], mi.want_ccd_witness(name, f).faces.shape[0], mi.want_contour(name, f).faces.shape[0])
             for f in range(len(mi.seq(name)))]
        print(f"{name}: (proximity witness, ccd witness, contour) rows a frame: {n}")
        assert min(min(x) for x in n) > 0, (name, n)
    d = mi.JITTER_DENSE_FRAME
    for k, want in enumerate((mi.want_prox_witness, mi.want_ccd_witness, mi.want_contour)):
        assert want("jitter", d).faces.shape[0] > 4 * want("jitter", d - 1).faces.shape[0], k      # the buffers of twice the rows grow there


def test_between_schedules_cross_in_every_frame_but_the_apart_one_which_never_touches():
    seps = []
    for schedule in mi.BETWEEN_SCHEDULES:
        for f in range(mi.BETWEEN_FRAMES):
            w = mi.want_between(schedule, f)
            rows, near = w["contour"].faces.shape[0], w["near"]
            found = near.faces[:, 0] != nr.NONE
            assert found.any(), (schedule, f)                                   # the precondition of near_min standing for rmax = +inf
            sep = float(w["near_min"].dist[0])
            if schedule == mi.APART:
                assert rows == 0 and w["contact"][0].shape[0] == 0 and sep > 0.0 and not (near.dist == 0.0).any(), (f, rows, sep)
                assert sep < mi.BETWEEN_CCD_DIST and w["prox_witness"].faces.shape[0] > 0 and w["ccd_witness"].faces.shape[0] > 0, (f, sep)
                seps.append(sep)
            else:
                assert rows > 0 and sep == 0.0, (schedule, f, rows, sep)
    print("both_move_apart: the separation distance, frame by frame:", [x.hex() for x in seps])
    assert all(_bits(x) != _bits(y) for x, y in zip(seps, seps[1:])) and len(set(seps)) == len(seps), seps
    assert 0.004 < min(seps) and max(seps) < 0.009, seps
    lift = mi.APART_LIFT
    assert len(lift) == mi.BETWEEN_FRAMES and all(x != y for x, y in zip(lift, lift[1:]))
    assert 1 <= len(mi.APART_INF_FRAMES) <= 3


def test_the_two_routes_to_the_nearest_rows_agree_on_a_frame_of_the_apart_schedule():
    """nearest_ref.nearest_rows at +inf (every a x b pair) cut to NEAREST_R is rows_of_all_pairs at NEAREST_R (the grid's candidates), and
    its minimum is near_min: what the GPU test takes for CD_NEAREST_MIN at +inf."""
    f = mi.APART_INF_FRAMES[0]
    w, rows = mi.want_between(mi.APART, f), mi.want_between_inf(f)
    assert (rows.faces[:, 0] == np.arange(rows.faces.shape[0])).all()
    mi.same_nearest(mi.nearest_call(nr.within(rows, mi.NEAREST_R)), w["near"], "apart")
    mi.same_nearest(mi.nearest_call(nr.nearest_min(rows)), w["near_min"], "apart")
    f0 = mi.APART_INF_FRAMES[1]
    with pytest.raises(AssertionError):                                         # the rows at +inf of one frame against another's
        mi.same_nearest(mi.nearest_call(nr.within(rows, mi.NEAREST_R)), mi.want_between(mi.APART, f0)["near"], "apart")


# ---------------------------------------------------------------- boxes, planes, segments and swept segments
def _tuple_differs(a, b):
    return any(x.shape != y.shape or x.tobytes() != y.tobytes() for x, y in zip(a, b))


def _new_row_sets(name, f):
    """(label, rows of frame f - 1, rows of frame f) of the four new all-results calls as test_moving_mesh_gpu.py makes them."""
    sets = [("boxes", mi.want_boxes(name, f - 1), mi.want_boxes(name, f)), ("planes", mi.want_planes(name, f - 1), mi.want_planes(name, f)),
            ("segments", mi.want_segments(name, f - 1), mi.want_segments(name, f)),
            ("swept segments", mi.want_swept_segments(name, f - 1)[0], mi.want_swept_segments(name, f)[0]),
            ("swept segments, the mesh at rest", mi.want_swept_segments_still(name, f - 1)[0], mi.want_swept_segments_still(name, f)[0])]
    if name in mi.SELF_SWEEP:
        sets.append(("the mesh's own edges", mi.want_self_swept_segments(name, f - 1)[0], mi.want_self_swept_segments(name, f)[0]))
    return sets


@pytest.mark.parametrize("name", mi.NAMES)
def test_box_plane_segment_and_swept_segment_comparisons_raise_on_the_previous_frames_result(name):
    """cd_boxes_overlap_all / cd_boxes_count, cd_planes_cut_all / cd_planes_count, cd_segments_within / cd_segments_closest and
    cd_sweep_segments_all / cd_sweep_segments: every comparison test_moving_mesh_gpu.py makes passes on the frame's own restatement and
    raises on the one of the frame before it, in every frame of every sequence -- the count calls included, plain and CD_BOX_ANY:
    the kinds of box_ref.make_boxes meet the mesh or miss it by construction, but whether a near box of moving_inputs.box_items does
    depends on the frame.  The box counts also raise on what a device that kept the previous frame's TREE would answer for this
    frame's boxes (moving_inputs.stale_boxes), ANY included.  (On a tiny mesh two frames' PLANE counts can be the same numbers: that
    comparison must raise whenever the expected counts differ, and they do differ in some frame of every sequence.)"""
    s = mi.seq(name)
    large = name in mi.LARGE
    planes_changed = 0
    for f in range(1, len(s)):
        what = f"{name} frame {f}"
        for label, w0, w1 in _new_row_sets(name, f):
            w = f"{what} {label}"
            mi.same_item_rows(mi.item_call(w1), w1, w)
            mi.same_item_rows(mi.item_call(w1), mi.item_rows(mi.item_call(w1)), w)      # (the form the fresh context's result is compared in)
            if w0.rows.shape[0] or w1.rows.shape[0]:
                with pytest.raises(AssertionError):
                    mi.same_item_rows(mi.item_call(w0), w1, w)
            with pytest.raises(AssertionError):                                 # the return code
                mi.same_item_rows(mi.item_call(w1, rc=1), w1, w)
        nb0, nb = mi.box_items(name, f - 1).shape[0], mi.box_items(name, f).shape[0]
        b0, b1 = mi.want_boxes(name, f - 1), mi.want_boxes(name, f)
        for any_ in (False, True):
            mi.same_box_counts(mi.box_count_call(b1, nb, any_), b1, nb, what, any_)
            with pytest.raises(AssertionError):                                 # the previous frame's expected counts
                mi.same_box_counts(mi.box_count_call(b0, nb0, any_), b1, nb, what, any_)
            with pytest.raises(AssertionError):                                 # this frame's boxes on the previous frame's tree
                mi.same_box_counts(mi.box_count_call(mi.stale_boxes(name, f), nb, any_), b1, nb, what, any_)
        with pytest.raises(AssertionError):
            mi.same_item_rows(mi.item_call(mi.stale_boxes(name, f)), b1, what + " boxes on the previous frame's tree")
        c0, c1 = mi.want_plane_classes(name, f - 1), mi.want_plane_classes(name, f)
        mi.same_plane_counts(mi.plane_count_call(c1), c1, what)
        if large or _tuple_differs(mi.plane_count_call(c0)[:3], mi.plane_count_call(c1)[:3]):
            planes_changed += 1
            with pytest.raises(AssertionError):
                mi.same_plane_counts(mi.plane_count_call(c0), c1, what)
        g0, g1 = mi.want_segments(name, f - 1), mi.want_segments(name, f)
        n0, n1 = mi.segment_items(name, f - 1).shape[0], mi.segment_items(name, f).shape[0]
        mi.same_segment_closest(mi.segment_closest_call(g1, n1), g1, n1, what)
        with pytest.raises(AssertionError):                                     # (the segments with r = +inf have a row in every frame)
            mi.same_segment_closest(mi.segment_closest_call(g0, n0), g1, n1, what)
        face = mi.segment_closest_call(g1, n1)
        mi.same_segment_any(face[0], face[11], g1, n1, what)
        with pytest.raises(AssertionError):                                     # the previous frame's faces against this frame's rows
            stale = mi.segment_closest_call(g0, n0)
            mi.same_segment_any(stale[0], stale[11], g1, n1, what)
        firsts = [("swept segments", mi.want_swept_segments, mi.swept_segment_items),
                  ("swept segments, the mesh at rest", mi.want_swept_segments_still, mi.swept_segment_items)]
        if name in mi.SELF_SWEEP:
            firsts.append(("the mesh's own edges", mi.want_self_swept_segments, lambda n_, k: mi.self_swept_segment_items(n_, k)[0]))
        for label, want, items in firsts:
            w0, w1 = want(name, f - 1)[0], want(name, f)[0]
            m0, m1 = items(name, f - 1).shape[0], items(name, f).shape[0]
            mi.same_sweep_segments(mi.sweep_segments_call(w1, m1), w1, m1, f"{what} {label}")
            if w0.rows.shape[0] or w1.rows.shape[0]:
                with pytest.raises(AssertionError):
                    mi.same_sweep_segments(mi.sweep_segments_call(w0, m0), w1, m1, f"{what} {label}")
        assert mi.want_swept_segments(name, f - 1)[1] != mi.want_swept_segments(name, f)[1], what     # ... and so do the counts compared beside the rows
    assert planes_changed > 0, name
    # the swept rows depend on the end positions: the same items against the mesh at rest are another row set
    assert any(mi.want_swept_segments(name, f)[0].rows.shape != mi.want_swept_segments_still(name, f)[0].rows.shape
               or not np.array_equal(mi.want_swept_segments(name, f)[0].toi, mi.want_swept_segments_still(name, f)[0].toi) for f in range(len(s))), name


def _corrupt(a, k):
    """One value of row k of a column changed: the lowest bit of a double, bit 0 of anything else."""
    if a.dtype == np.float64:
        _flip_lowest_bit(a.reshape(a.shape[0], -1), (k, 0))
    else:
        a.reshape(a.shape[0], -1)[k, 0] ^= 1


def test_one_corrupted_field_of_a_box_plane_segment_or_swept_segment_result_raises():
    """The right frame's result with ONE value changed: every column of every new row type, one face, one row dropped; every count
    array of cd_boxes_count (plain and ANY) and cd_planes_count and their n_found; every output of cd_segments_closest and of
    cd_sweep_segments and their n_found."""
    name, f = "jitter", 1
    for rows in (mi.want_boxes(name, f), mi.want_planes(name, f), mi.want_segments(name, f), mi.want_swept_segments(name, f)[0]):
        k = rows.rows.shape[0] // 2
        assert k > 0
        for field in rows._fields[1:]:
            bad = _copy(rows)
            _corrupt(getattr(bad, field), k)
            with pytest.raises(AssertionError):
                mi.same_item_rows(mi.item_call(bad), rows, (type(rows).__name__, field))
        bad = _copy(rows)
        bad.rows[k, 1] ^= 1
        with pytest.raises(AssertionError):
            mi.same_item_rows(mi.item_call(bad), rows, "face")
        with pytest.raises(AssertionError):
            mi.same_item_rows(mi.item_call(type(rows)(*(np.delete(a, k, axis=0) for a in rows))), rows, "a row less")
    boxes, nb = mi.want_boxes(name, f), mi.box_items(name, f).shape[0]
    for any_ in (False, True):
        good = mi.box_count_call(boxes, nb, any_)
        for j in range(1 if any_ else 2):
            bad = [a if a is None else a.copy() for a in good[:2]]
            bad[j][nb // 2] ^= 1
            with pytest.raises(AssertionError):
                mi.same_box_counts((bad[0], bad[1], good[2]), boxes, nb, ("count", j), any_)
        with pytest.raises(AssertionError):                                     # n_found alone
            mi.same_box_counts(good[:2] + (mi.mi355cd.CdBoxInfo(good[2].n_found + 1, 0, 0),), boxes, nb, "n_found", any_)
    cls = mi.want_plane_classes(name, f)
    good = mi.plane_count_call(cls)
    for j in range(3):
        bad = [a.copy() for a in good[:3]]
        bad[j][mi.NPLANES // 2] += 1
        with pytest.raises(AssertionError):
            mi.same_plane_counts(tuple(bad) + (good[3],), cls, ("plane count", j))
    with pytest.raises(AssertionError):
        mi.same_plane_counts(good[:3] + (mi.mi355cd.CdPlaneInfo(good[3].n_found + 1, 0, 0),), cls, "n_found")
    for rows, n, call, same, info in ((mi.want_segments(name, f), mi.segment_items(name, f).shape[0], mi.segment_closest_call, mi.same_segment_closest, mi.mi355cd.CdSegmentInfo),
                                      (mi.want_swept_segments(name, f)[0], mi.swept_segment_items(name, f).shape[0], mi.sweep_segments_call, mi.same_sweep_segments, mi.mi355cd.CdPointInfo)):
        good = call(rows, n)
        item = int(np.flatnonzero(wn.rows_per_item(rows, n) >= 2)[3])
        for j in range(len(good) - 1):
            bad = [a.copy() for a in good[:-1]]
            _corrupt(bad[j], item)
            with pytest.raises(AssertionError):
                same(tuple(bad) + (good[-1],), rows, n, ("output", j))
        with pytest.raises(AssertionError):                                     # n_found alone
            same(good[:-1] + (info(good[-1].n_found + 1, 0, 0),), rows, n, "n_found")
        rest = type(rows)(*(a[~((rows.rows[:, 0] == item) & (rows.rows[:, 1] == good[0][item]))] for a in rows))      # the rows without that item's first
        with pytest.raises(AssertionError):
            same(call(rest, n), rows, n, "the second row")
    segs, n = mi.want_segments(name, f), mi.segment_items(name, f).shape[0]
    good = mi.segment_closest_call(segs, n)
    none = int(np.flatnonzero(good[0] == sg.NONE)[0])
    face = good[0].copy(); face[none] = 0
    with pytest.raises(AssertionError):                                         # ANY: a face for a segment that has no row
        mi.same_segment_any(face, good[11], segs, n, "any")
    has = int(np.flatnonzero(good[0] != sg.NONE)[5])
    face = good[0].copy(); face[has] = np.setdiff1d(np.arange(mi.seq(name).nt), segs.rows[segs.rows[:, 0] == has, 1])[0]
    with pytest.raises(AssertionError):                                         # ANY: a face that is no row of the segment
        mi.same_segment_any(face, good[11], segs, n, "any")


@pytest.mark.parametrize("name", mi.LARGE)
def test_new_item_queries_cannot_pass_vacuously(name):
    """In EVERY frame of the large sequences: at least 32 boxes, segments and swept segments have no row and at least 32 of each have
    two or more; the root box's rows are every triangle, all inside; every point box has a row; the segments with r = +inf have every
    triangle; some plane has faces cut, below and above, and some plane cuts nothing; some swept-segment row has 0 < toi < 1; no
    swept-segment row is unresolved; the segment rows have crossings and rows that are none."""
    s = mi.seq(name)
    low = dict(none=1 << 30, several=1 << 30, inside=1 << 30)
    for f in range(len(s)):
        what = (name, f)
        boxes, segs, (swept, counts) = mi.want_boxes(name, f), mi.want_segments(name, f), mi.want_swept_segments(name, f)
        for rows, n in ((boxes, mi.box_items(name, f).shape[0]), (segs, mi.segment_items(name, f).shape[0]), (swept, mi.swept_segment_items(name, f).shape[0])):
            c = wn.rows_per_item(rows, n)
            assert (c == 0).sum() >= 32 and (c >= 2).sum() >= 32, (what, type(rows).__name__, int((c == 0).sum()), int((c >= 2).sum()))
            low["none"], low["several"] = min(low["none"], int((c == 0).sum())), min(low["several"], int((c >= 2).sum()))
        c, ci = bx.counts_of(boxes, mi.box_items(name, f).shape[0])
        assert c[mi.NBOX] == s.nt == ci[mi.NBOX] and (c[mi.NBOX + 1:mi.NBOX + 1 + mi.POINT_BOXES] >= 1).all(), what
        near = c[mi.NBOX + 1 + mi.POINT_BOXES:] > 0                             # the near boxes: some meet a face and some do not, in every frame
        assert near.shape[0] == mi.NEAR_BOXES and near.sum() >= 4 and (~near).sum() >= 4, (what, int(near.sum()))
        assert np.array_equal(mi.box_items(name, f)[mi.NBOX], mi.want_root_box(name, f)), what
        assert boxes.inside.any() and not boxes.inside.all(), what
        it = mi.segment_items(name, f)
        c = wn.rows_per_item(segs, it.shape[0])
        assert np.isinf(it[list(mi.SEG_INF), 6]).all() and (c[list(mi.SEG_INF)] == s.nt).all() and np.isfinite(np.delete(it[:, 6], mi.SEG_INF)).all(), what
        assert (it[:mi.NI:mi.SEG_POINT_EVERY, 0:3] == it[:mi.NI:mi.SEG_POINT_EVERY, 3:6]).all() and (segs.cross == 1).any() and (segs.cross == 0).any(), what
        r = it[:mi.NI, 6][np.isfinite(it[:mi.NI, 6])]
        assert np.unique(r).size == 3, what                                  # three radii, by i % 3
        n_cut, n_below, n_above = plr.counts_of_classes(mi.want_plane_classes(name, f))
        assert ((n_cut > 0) & (n_below > 0) & (n_above > 0)).any() and (n_cut == 0).any() and mi.want_planes(name, f).rows.shape[0] == n_cut.sum(), what
        inside = int(((swept.toi > 0) & (swept.toi < 1)).sum())
        assert inside >= 1 and counts[2] == 0 and mi.want_swept_segments_still(name, f)[1][2] == 0, (what, inside, counts)
        low["inside"] = min(low["inside"], inside)
        if name in mi.SELF_SWEEP:
            own, own_counts = mi.want_self_swept_segments(name, f)
            e = mi.mesh_edges(name)
            assert own.rows.shape[0] > 100 and own_counts[2] == 0 and ((own.toi > 0) & (own.toi < 1)).any() and e.shape[0] % 64 != 0, what
            assert not (s.vidx[own.rows[:, 1]][:, :, None] == e[own.rows[:, 0]][:, None, :]).any()       # no face at either end of the edge
    print(f"{name}: the smallest over its frames and the three item sets: items with no row {low['none']}, with several {low['several']}; swept-segment rows with 0 < toi < 1: {low['inside']}")


def test_tiny_sequences_have_box_plane_segment_and_swept_segment_rows_in_some_frame():
    for n in mi.TINY:
        name = f"tiny{n}"
        rows = [(mi.want_boxes(name, f).rows.shape[0], mi.want_planes(name, f).rows.shape[0], mi.want_segments(name, f).rows.shape[0],
                 mi.want_swept_segments(name, f)[0].rows.shape[0], mi.want_swept_segments_still(name, f)[0].rows.shape[0]) for f in range(len(mi.seq(name)))]
        print(f"{name}: (boxes, planes, segments, swept segments, swept segments at rest) rows a frame: {rows}")
        assert all(max(r[k] for r in rows) > 0 for k in range(5)), (name, rows)


def test_the_segment_growth_block_overflows_a_shard_and_the_dense_frame_more_than_doubles_the_rows():
    """Items SEG_GROWTH_AT .. SEG_GROWTH_AT + 63 of jitter's dense frame are ONE block of the descent (one shard), and their rows alone are
    more than the shard's first WITHIN_SHARD_FIRST slots, for cd_segments_within and for cd_sweep_segments_all moving and at rest: the pass
    must grow its candidate buffer and run again.  The frame's rows are more than twice the frame's before it, so a row buffer of twice
    the previous frame's rows does not hold them: the row buffers grow there too, and are oversized on the sparse frames after it."""
    f = mi.JITTER_DENSE_FRAME
    assert mi.SEG_GROWTH_AT % 64 == 0 and mi.GROWTH_ITEMS == 64 and mi.SEG_GROWTH_AT >= mi.NI
    figures = []
    for items, want in ((mi.segment_items, mi.want_segments), (mi.swept_segment_items, lambda n, k: mi.want_swept_segments(n, k)[0]),
                        (mi.swept_segment_items, lambda n, k: mi.want_swept_segments_still(n, k)[0])):
        assert items("jitter", f).shape[0] == mi.SEG_GROWTH_AT + mi.GROWTH_ITEMS
        rows = want("jitter", f)
        blk = int((rows.rows[:, 0] >= mi.SEG_GROWTH_AT).sum())
        fill = int(((rows.rows[:, 0] >= mi.NI) & (rows.rows[:, 0] < mi.SEG_GROWTH_AT)).sum())
        figures.append((blk, rows.rows.shape[0], want("jitter", f - 1).rows.shape[0]))
        assert blk > mi.mi355cd.WITHIN_SHARD_FIRST and fill == 0, (blk, fill)
        assert rows.rows.shape[0] > 2 * want("jitter", f - 1).rows.shape[0] and all(want("jitter", g).rows.shape[0] < rows.rows.shape[0] // 2 for g in range(f + 1, len(mi.seq("jitter"))))
        for g in range(len(mi.seq("jitter"))):
            assert (items("jitter", g).shape[0] == mi.NI) == (g != f)
    print("jitter's growth block: (rows of the block, of the dense frame, of the frame before) for segments, swept segments, swept segments at rest:", figures,
          "of", mi.mi355cd.WITHIN_SHARD_FIRST, "slots")
