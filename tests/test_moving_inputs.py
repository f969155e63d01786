"""The motion sequences of tests/moving_inputs.py can catch stale state, shown on the CPU: consecutive frames have different right
answers, each sequence does what it is named for, and every comparison helper of tests/test_moving_mesh_gpu.py raises when it is fed
frame f - 1's expected result against frame f's (the planted error: a device that kept the previous frame's state)."""
from __future__ import annotations

import numpy as np
import pytest

import moving_inputs as mi
import oracle
import scale_inputs as si
import swept_ref as sr


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
        # ... and raises on the one before it
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
            assert c.shape[0] > 0 and p[0].shape[0] > 0 and q[0].shape[0] > 0
            with pytest.raises(AssertionError):
                mi.same_between_contact((c0, c0.shape[0], 0), c, what)
            with pytest.raises(AssertionError):
                mi.same_between_prox((p0[0], p0[1], p0[0].shape[0], 0), p, what)
            with pytest.raises(AssertionError):
                mi.same_between_ccd((q0[0], q0[1], q0[2], q0[0].shape[0], 0), q, what)
