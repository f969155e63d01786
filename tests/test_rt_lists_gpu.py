"""The ray tracer's binning on the GPU, pinned where tests/test_rt_gpu.py leaves it free: a tile list at, below and above its capacity (TILE_CAP = 48) in
single frames and inside the animation loop's fused launch, every grid-stride loop of the prepare roles going round more than once, single frames /
slabs / brute frames / repeats interleaved with loops on one context, rt_set_spheres, and edge values (tests/rt_ref.py: edge_scenes).

Every image is compared with the CPU oracle byte for byte.  rt_stats.sphere_tests is compared EXACTLY: in binned mode with the numpy restatement of the
binning decision (tests/rt_ref.py, itself checked against the oracle in tests/test_rt_ref.py) -- 4096 * sum over the rendered tiles of the number of
spheres whose may_touch holds, whichever read path a tile takes: a missed tile, a double entry or a stale counter changes it; in brute mode with
n * dim * rows.

For the record (tests/test_rt_ref.py asserts it): the loop scene of tests/test_rt_gpu.py reaches at most 44 spheres in a tile (shake 2; 41 with shake 1,
35 with shake 0) over the frames its fused loops render, so the super-tile path of k_frame was first run by the tests below."""
import concurrent.futures as cf

import numpy as np
import pytest

import mi355rt
import oracle
import rt_ref

pytestmark = pytest.mark.gpu
BINNED, BRUTE = mi355rt.RT_MODE_BINNED, mi355rt.RT_MODE_BRUTE
MODES = [BINNED, BRUTE]


def _want_tests(mode, spheres, shifts, dim, csx=0, csy=0, rows=None):
    if mode == BRUTE:
        y0, y1 = (0, dim) if rows is None else rows
        return spheres.shape[0] * dim * (y1 - y0)
    return rt_ref.expected_sphere_tests(spheres, shifts, dim, csx, csy, rows)


def _check(tag, rt, img, mode, spheres, shifts, dim, csx=0, csy=0, rows=None):
    """The frame (or slab) just rendered on `rt` against the oracle, and its sphere_tests against the restatement; figures printed before they are asserted."""
    want = oracle.rt_render(spheres, shifts, dim, csx, csy, rows=rows)
    if rows is not None:
        want = want[rows[0]:rows[1]]
    got_t, want_t = rt.stats().sphere_tests, _want_tests(mode, spheres, shifts, dim, csx, csy, rows)
    bad = int((img != want).any(axis=2).sum())
    print(f"{tag}: mode {mode} rows {rows}: {bad} pixels differ, sphere_tests {got_t} (want {want_t})")
    assert bad == 0, (tag, bad, np.argwhere((img != want).any(axis=2))[:4])
    assert got_t == want_t, (tag, got_t, want_t)


# ---------------------------------------------------------------- a. the capacity boundary, single frames
TILES = {"first": (0, 0, (1, 2)), "interior": (1, 2, (2, -2)), "last": (3, 3, (-2, -3))}      # tile row, column, (rows, columns) the third render moves the cluster by


def _three_renders(tag, spheres, shifts, shifts_moved, dim):
    """Twice in a row, then with the clusters moved to other tiles: counter sets 0, 1, 2 and list sets 0, 1, 0 of a fresh context -- the third frame reuses
    the lists that overflowed two frames ago."""
    for mode in MODES:
        with mi355rt.RayTracer(spheres, dim) as rt:
            rt.set_mode(mode)
            for step, sh in enumerate((shifts, shifts, shifts_moved)):
                _check(f"{tag} render {step}", rt, rt.render(sh), mode, spheres, sh, dim)


@pytest.mark.parametrize("where", list(TILES))
@pytest.mark.parametrize("k", [47, 48, 49, 50])
def test_capacity_boundary_single_frame(k, where):
    """k = 47, 48, 49, 50 spheres of radius 3 inside ONE tile (the first, an interior one, the last), two of them exact duplicates, 20 others elsewhere:
    cnt < / == TILE_CAP reads the tile's own list, cnt > TILE_CAP the super-tile's; bin_sphere stores entry `pos` only while pos < TILE_CAP."""
    dim = 256
    ty, tx, (dty, dtx) = TILES[where]
    spheres, shifts, (mem,) = rt_ref.capacity_scene(dim, [(ty, tx, k)], seed=100 + k, keep_clear=[(ty + dty, tx + dtx)])
    sh2 = rt_ref.moved(shifts, mem, dty, dtx)
    c1, c2 = rt_ref.tile_counts(spheres, shifts, dim), rt_ref.tile_counts(spheres, sh2, dim)
    assert c1[ty, tx] == k and c2[ty + dty, tx + dtx] == k and c2[ty, tx] == 0
    assert np.delete(c1.ravel(), ty * 4 + tx).max() < k
    _three_renders(f"capacity {k} {where}", spheres, shifts, sh2, dim)


@pytest.mark.parametrize("dim,left,right,move", [(256, (1, 1), (1, 2), (2, -1)), (512, (2, 3), (2, 4), (3, -2))])
def test_capacity_48_beside_49(dim, left, right, move):
    """48 spheres in a tile (its own list, full) and 49 in its right-hand neighbour (the super-tile's list); at dim 512 the two tiles lie in different
    super-tiles."""
    dest = [(left[0] + move[0], left[1] + move[1]), (right[0] + move[0], right[1] + move[1])]
    spheres, shifts, (ma, mb) = rt_ref.capacity_scene(dim, [left + (48,), right + (49,)], seed=7 + dim, keep_clear=dest)
    sh2 = rt_ref.moved(shifts, np.concatenate([ma, mb]), *move)
    c1, c2 = rt_ref.tile_counts(spheres, shifts, dim), rt_ref.tile_counts(spheres, sh2, dim)
    assert c1[left] == 48 and c1[right] == 49 and c2[dest[0]] == 48 and c2[dest[1]] == 49 and c2[left] == 0 and c2[right] == 0
    assert (dim == 512) == (left[1] // 4 != right[1] // 4)
    _three_renders(f"48|49 dim {dim}", spheres, shifts, sh2, dim)


# ---------------------------------------------------------------- the animation loop against the oracle's state, frame and restatement
def _loop_and_check(tag, rt, ref, spheres, dim, frames, shake, csx, csy, seq=None, need_overflow=False):
    """rt_anim_loop(frames) on `rt`; the oracle's state `ref` is moved on alongside (and the context `seq`, if given, through the kernel sequence)."""
    img = rt.anim_loop(frames, shake, 35, 3, 18, csx, csy)
    got_t = rt.stats().sphere_tests
    want_seq = None
    for _ in range(frames):
        rt_ref.anim_step(ref, shake)
        if need_overflow:
            assert rt_ref.tile_counts(spheres, ref.shifts, dim, csx, csy).max() > rt_ref.TILE_CAP        # every frame of the loop has a tile on the super-tile path
        if seq is not None:
            if shake == 1:
                seq.anim_axis_move(35)
            elif shake == 2:
                seq.anim_curve_move(); seq.anim_update_speed_angle(3, 18)
            want_seq = seq.render(None, csx, csy)
    sh, ang, rng = rt.anim_state()
    assert np.array_equal(rng, ref.rng) and np.array_equal(sh, ref.shifts) and np.array_equal(ang.view(np.uint64), ref.angles.view(np.uint64)), tag
    want_t = rt_ref.expected_sphere_tests(spheres, ref.shifts, dim, csx, csy)
    print(f"{tag}: loop of {frames}, shake {shake}: sphere_tests {got_t} (want {want_t})")
    if seq is not None:
        assert np.array_equal(img, want_seq), tag
        assert seq.stats().sphere_tests == want_t, (tag, seq.stats().sphere_tests, want_t)
    return img, got_t, want_t


# ---------------------------------------------------------------- b. capacity inside the loop
@pytest.mark.parametrize("shake", [2, 0])
def test_capacity_inside_the_loop(shake):
    """60 spheres that the animation keeps around one tile for the 10 frames used, 100 others: some tile holds more than 48 in EVERY frame (asserted on the
    CPU), so k_frame's render role walks super_list / geom of set f & 1 while its prepare role fills the other set."""
    n, dim, csx, csy = 160, 256, 2, -3
    spheres, _ = rt_ref.loop_cluster_scene(n, dim, (1, 2), 10, shake, csx, csy, seed=21)
    ref = oracle.RtAnim(n)
    with mi355rt.RayTracer(spheres, dim) as rt, mi355rt.RayTracer(spheres, dim) as seq:
        rt.anim_init(); seq.anim_init()
        for frames in (1, 2, 3, 4):
            tag = f"loop capacity shake {shake} x{frames}"
            img, got_t, want_t = _loop_and_check(tag, rt, ref, spheres, dim, frames, shake, csx, csy, seq=seq, need_overflow=True)
            assert np.array_equal(img, oracle.rt_render(spheres, ref.shifts, dim, csx, csy)), tag
            assert got_t == want_t, (tag, got_t, want_t)
        assert shake == 0 or (np.abs(ref.shifts[:, :2]) > 0).any()


# ---------------------------------------------------------------- c. strides that wrap
@pytest.mark.parametrize("n", [700, 4100])
def test_loop_prepare_strides_wrap(n):
    """dim 64: the prepare row of k_frame has 256 threads for 700 spheres (three rounds); n = 4100 is more than k_anim_prepare's 4096 threads."""
    dim, csx, csy = 64, 1, -2
    rng = np.random.default_rng(n)
    spheres = rt_ref._ordinary(rng, n, dim, spread=6.0)
    spheres["idx"] = np.arange(n, dtype=np.int32)
    ref = oracle.RtAnim(n)
    with mi355rt.RayTracer(spheres, dim) as rt:
        rt.anim_init()
        for frames, shake in ((1, 2), (3, 2), (2, 1), (2, 2)):
            tag = f"loop strides n {n} x{frames}"
            img, got_t, want_t = _loop_and_check(tag, rt, ref, spheres, dim, frames, shake, csx, csy)
            assert np.array_equal(img, oracle.rt_render(spheres, ref.shifts, dim, csx, csy)), tag
            assert got_t == want_t, (tag, got_t, want_t)
            assert 0 < want_t < n * dim * dim
        _check(f"single frame after the loops, n {n}", rt, rt.render(None, csx, csy), BINNED, spheres, ref.shifts, dim, csx, csy)


@pytest.mark.parametrize("mode", MODES)
def test_prepare_zeroing_stride_wraps(mode):
    """dim 1024, ONE sphere: k_prepare has 64 threads for 272 counters.  The sphere (radius 40) is moved across tiles by its shift row; the first and the
    fourth frame use the same counter set and put it on the same tiles (numbers above 64), so a counter that was not zeroed is read one entry too far."""
    dim = 1024
    s = np.zeros(1, dtype=mi355rt.SPHERE_DTYPE)
    s["x"], s["y"], s["z"], s["radius"] = 130.0, 200.0, 5.0, 40.0
    s["r"], s["g"], s["b"] = 0.9, 0.5, 0.25
    places = [(0, 0), (-400, -650), (300, 250), (3, -2), (-130, -200)]
    sh = rt_ref.init_shifts(1)
    with mi355rt.RayTracer(s, dim) as rt:
        rt.set_mode(mode)
        for f, p in enumerate(places[:4]):
            sh[0, :2] = p
            _check(f"one sphere, frame {f}", rt, rt.render(sh), mode, s, sh, dim)
        a = rt_ref.tile_counts(s, sh, dim)
        sh[0, :2] = places[0]
        b = rt_ref.tile_counts(s, sh, dim)
        assert np.array_equal(a, b) and np.nonzero(b.ravel())[0].min() >= 64 and b.sum() == 4     # frames 0 and 3: the same four tiles
        sh[0, :2] = places[3]
        _check("one sphere, repeat x4", rt, rt.render_repeat(sh, 4), mode, s, sh, dim)
        sh[0, :2] = places[4]
        _check("one sphere, after the repeat", rt, rt.render(sh), mode, s, sh, dim)
        sh[0, :2] = places[3]
        _check("one sphere, back", rt, rt.render(sh), mode, s, sh, dim)


def test_loop_at_the_benchmark_shape_with_an_overflowing_tile():
    """dim 4096, n = 4200 (more spheres than k_anim_prepare has threads, n_counts = 4352 counters), 60 of them kept in one tile of the last super-tile row:
    rt_anim_loop(4, shake 2).  sphere_tests for the WHOLE frame; pixels on two 64-row slabs (the oracle needs seconds per slab at this width)."""
    n, dim, csx, csy, tile = 4200, 4096, 2, -3, (61, 37)
    spheres, _ = rt_ref.loop_cluster_scene(n, dim, tile, 4, 2, csx, csy, seed=22)
    ref = oracle.RtAnim(n)
    with mi355rt.RayTracer(spheres, dim) as rt:
        rt.anim_init()
        img, got_t, want_t = _loop_and_check("benchmark shape", rt, ref, spheres, dim, 4, 2, csx, csy, need_overflow=True)
    counts = rt_ref.tile_counts(spheres, ref.shifts, dim, csx, csy)
    assert counts[tile] > rt_ref.TILE_CAP and counts[tile] == counts.max()
    assert got_t == want_t, (got_t, want_t)
    slabs = [(tile[0] * 64, tile[0] * 64 + 64), (0, 64)]
    oracle.rt_render(spheres, ref.shifts, dim, csx, csy, rows=(0, 1))         # (the library is loaded before the threads start)
    with cf.ThreadPoolExecutor(2) as ex:                                     # ctypes releases the GIL inside the C call
        outs = list(ex.map(lambda r: oracle.rt_render(spheres, ref.shifts, dim, csx, csy, rows=r)[r[0]:r[1]].copy(), slabs))
    for (y0, y1), want in zip(slabs, outs):
        assert np.array_equal(img[y0:y1], want), (y0, y1)
        assert want[..., :3].any()


# ---------------------------------------------------------------- d. interleaving on one context
def test_loops_interleaved_with_slabs_brute_frames_and_repeats():
    n, dim, csx, csy = 300, 256, -5, 4
    spheres = rt_ref._ordinary(np.random.default_rng(55), n, dim)
    spheres["idx"] = np.arange(n, dtype=np.int32)
    ref = oracle.RtAnim(n)

    def loop(rt, frames, tag):
        img, got_t, want_t = _loop_and_check(tag, rt, ref, spheres, dim, frames, 2, csx, csy)
        assert np.array_equal(img, oracle.rt_render(spheres, ref.shifts, dim, csx, csy)), tag
        assert got_t == want_t, (tag, got_t, want_t)

    with mi355rt.RayTracer(spheres, dim) as rt:
        rt.anim_init()
        loop(rt, 2, "interleave: loop 2")
        _check("interleave: slab", rt, rt.render(None, csx, csy, rows=(64, 128)), BINNED, spheres, ref.shifts, dim, csx, csy, rows=(64, 128))
        rt.set_mode(BRUTE)
        _check("interleave: brute", rt, rt.render(None, csx, csy), BRUTE, spheres, ref.shifts, dim, csx, csy)
        rt.set_mode(BINNED)
        loop(rt, 3, "interleave: loop 3")
        sh, _, _ = rt.anim_state()                                           # render_repeat takes host shifts: the state's own, so the state stays what it is
        _check("interleave: repeat", rt, rt.render_repeat(sh, 2, csx, csy), BINNED, spheres, ref.shifts, dim, csx, csy)
        loop(rt, 1, "interleave: loop 1")
        _check("interleave: last", rt, rt.render(None, csx, csy), BINNED, spheres, ref.shifts, dim, csx, csy)


# ---------------------------------------------------------------- e. rt_set_spheres
def test_set_spheres_switches_between_the_fused_loop_and_the_kernel_sequence():
    """Identity idx (the fused launch) -> a permuted idx, other positions and colours (the kernel sequence; a sphere reads the shift row its idx names) ->
    identity again.  The animation state belongs to the rows and runs on.  A bad idx is refused and leaves the old spheres in place."""
    n, dim, csx, csy = 200, 256, 3, -1
    a = rt_ref._ordinary(np.random.default_rng(61), n, dim)
    a["idx"] = np.arange(n, dtype=np.int32)
    b = rt_ref._ordinary(np.random.default_rng(62), n, dim)
    b["idx"] = np.random.default_rng(63).permutation(n).astype(np.int32)
    assert (b["idx"] != a["idx"]).any()
    ref = oracle.RtAnim(n)
    with mi355rt.RayTracer(a, dim) as rt:
        rt.anim_init()
        for step, (s, frames) in enumerate(((a, 2), (b, 3), (a, 2), (b, 1))):
            if step:
                rt.set_spheres(s)
                assert np.array_equal(rt.spheres, s) and rt.n == n
            tag = f"set_spheres step {step}"
            img, got_t, want_t = _loop_and_check(tag, rt, ref, s, dim, frames, 2, csx, csy)
            assert np.array_equal(img, oracle.rt_render(s, ref.shifts, dim, csx, csy)), tag
            assert got_t == want_t, (tag, got_t, want_t)
        for bad_idx in (n, -1):
            bad = a.copy()
            bad["idx"][n // 2] = bad_idx
            with pytest.raises(mi355rt.RtError) as err:
                rt.set_spheres(bad)
            assert err.value.rc == mi355rt.RT_ERR_ARG
            assert np.array_equal(rt.spheres, b)
            _check(f"after a refused idx {bad_idx}", rt, rt.render(None, csx, csy), BINNED, b, ref.shifts, dim, csx, csy)


# ---------------------------------------------------------------- f. edge values
EDGE = rt_ref.edge_scenes()


@pytest.mark.parametrize("case", range(len(EDGE)), ids=[e[0] for e in EDGE])
def test_edge_values(case):
    """One scene per edge value (tests/rt_ref.py: edge_scenes; what each does on the CPU is asserted in tests/test_rt_ref.py), dim 128, both modes, the
    whole frame and a slab.  sphere_tests must equal the restatement on the NaN spheres too: may_touch keeps NaN, bin_sphere keeps the full range."""
    name, spheres, shifts, csx, csy, _ = EDGE[case]
    dim = rt_ref.EDGE_DIM
    with mi355rt.RayTracer(spheres, dim) as rt:
        for mode in MODES:
            rt.set_mode(mode)
            _check(name, rt, rt.render(shifts, csx, csy), mode, spheres, shifts, dim, csx, csy)
            for rows in ((64, 128), (0, 64)):
                _check(name, rt, rt.render(shifts, csx, csy, rows=rows), mode, spheres, shifts, dim, csx, csy, rows=rows)
