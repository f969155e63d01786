"""tests/rt_ref.py (the numpy restatement of the ray tracer's binning decision, prepare_one + may_touch) against the pixel oracle, on the CPU:
what tests/test_rt_lists_gpu.py compares rt_stats.sphere_tests with must itself be right.

  * conservative: every pixel a sphere hits by the oracle (rendered alone) lies in a tile whose count includes that sphere;
  * tight where geometry decides: a sphere at least radius + 1 pixels inside one tile is counted in that tile only;
  * on the scenes the GPU tests use: the capacity clusters (47..50 spheres in one tile) and the edge values (radius 0 / denormal / negative / 1e19,
    centres at 1e8 and 3e9, z of +-inf / NaN / -2e10, NaN in x, y, radius, shifts of 2^24 + 1 and 2^30, camera offsets of 2^24 + 3).

MEASURED HERE, asserted below: the animation-loop scene of tests/test_rt_gpu.py (sphere_scene(700, 512, seed 13), camera offsets 2, -3) never fills a
tile beyond its own list.  Over the 18 frames its fused loops render, the largest tile count is 44 with shake 2, 41 with shake 1 and 35 with shake 0
(TILE_CAP is 48): k_frame's super-tile path and a list at capacity were never reached by that test.  tests/test_rt_lists_gpu.py reaches both."""
import numpy as np
import pytest

import mi355_synth as synth
import oracle
import rt_ref


def _alone(spheres, shifts, dim, csx, csy, i):
    """Pixels [dim, dim] that sphere i hits by the oracle."""
    return rt_ref.hit_mask(spheres, shifts, dim, csx, csy, int(i))


def _check_conservative(spheres, shifts, dim, csx=0, csy=0, which=None):
    touch = rt_ref.tile_touch(spheres, shifts, dim, csx, csy)
    counts = rt_ref.tile_counts(spheres, shifts, dim, csx, csy)
    assert np.array_equal(counts, touch.sum(axis=2))
    nt = dim // 64
    lit_any = False
    for i in (range(spheres.shape[0]) if which is None else which):
        lit = _alone(spheres, shifts, dim, csx, csy, i).reshape(nt, 64, nt, 64).any(axis=(1, 3))
        assert not (lit & ~touch[:, :, i]).any(), (i, np.argwhere(lit & ~touch[:, :, i]))
        lit_any = lit_any or lit.any()
    return touch, counts, lit_any


@pytest.mark.parametrize("dim,n,seed,csx,csy", [(64, 30, 1, 0, 0), (128, 120, 2, 5, -9), (256, 200, 3, -40, 77), (192, 150, 4, 13, 64)])
def test_may_touch_keeps_every_tile_the_oracle_colours(dim, n, seed, csx, csy):
    rng = np.random.default_rng(seed)
    spheres, shifts = synth.sphere_scene(n, dim, seed)
    spheres["radius"] = (rng.random(n) ** 3 * float(rng.choice([4.0, 40.0, 2.0 * dim])) + 0.25).astype(np.float32)
    spheres["x"] = (spheres["x"] * 1.5).astype(np.float32)
    spheres["idx"] = rng.permutation(n).astype(np.int32)                     # the shift row is the one idx names
    shifts[:, :2] = rng.integers(-40, 40, size=(n, 2))
    touch, counts, lit = _check_conservative(spheres, shifts, dim, csx, csy)
    assert lit and counts.max() > 0
    assert rt_ref.expected_sphere_tests(spheres, shifts, dim, csx, csy) == 4096 * int(counts.sum())
    if dim >= 128:
        rows = (64, 128)
        slab = rt_ref.tile_counts(spheres, shifts, dim, csx, csy, rows)
        assert np.array_equal(slab[1], counts[1]) and slab.sum() == counts[1].sum()
        assert rt_ref.expected_sphere_tests(spheres, shifts, dim, csx, csy, rows) == 4096 * int(counts[1].sum())


def test_a_sphere_well_inside_one_tile_is_counted_there_only():
    dim, n = 256, 200
    rng = np.random.default_rng(8)
    spheres, shifts = synth.sphere_scene(n, dim, 8)
    ty, tx = rng.integers(0, 4, n), rng.integers(0, 4, n)
    rad = (0.3 + rng.random(n) * 25.0).astype(np.float32)
    m = rad.astype(np.float64) + 1.0                                        # centre at least radius + 1 pixels from the tile's edges
    px = tx * 64 + m + rng.random(n) * (63 - 2 * m)
    py = ty * 64 + m + rng.random(n) * (63 - 2 * m)
    csx, csy = 7, -11
    shifts[:, 0] = rng.integers(-30, 30, n); shifts[:, 1] = rng.integers(-30, 30, n)
    spheres["radius"] = rad
    spheres["x"] = np.round(px * 4) / 4 - dim // 2 + csx - shifts[:, 0]      # (quarter pixels: exact in float)
    spheres["y"] = np.round(py * 4) / 4 - dim // 2 + csy - shifts[:, 1]
    touch, counts, lit = _check_conservative(spheres, shifts, dim, csx, csy)
    assert lit
    want = np.zeros_like(touch)
    want[ty, tx, np.arange(n)] = True
    assert np.array_equal(touch, want)
    assert np.array_equal(counts, np.bincount(ty * 4 + tx, minlength=16).reshape(4, 4))


@pytest.mark.parametrize("k", [47, 48, 49, 50])
def test_capacity_scenes_count_the_cluster_in_its_tile_only(k):
    dim = 256
    for ty, tx, (dty, dtx) in ((0, 0, (1, 2)), (1, 2, (2, -2)), (3, 3, (-2, -3))):
        spheres, shifts, (mem,) = rt_ref.capacity_scene(dim, [(ty, tx, k)], seed=100 + k, keep_clear=[(ty + dty, tx + dtx)])
        assert spheres.shape[0] == k + 20 and mem.shape[0] == k
        touch, counts, lit = _check_conservative(spheres, shifts, dim)
        assert lit and counts[ty, tx] == k and touch[:, :, mem].sum() == k
        sh2 = rt_ref.moved(shifts, mem, dty, dtx)
        _, counts2, _ = _check_conservative(spheres, sh2, dim, which=mem)
        assert counts2[ty + dty, tx + dtx] == k and counts2[ty, tx] == 0
        a, b = mem[0], mem[1]                                               # the exact duplicates
        assert all(spheres[f][a] == spheres[f][b] for f in ("x", "y", "z", "radius")) and spheres["r"][a] != spheres["r"][b]


EDGE = rt_ref.edge_scenes()


@pytest.mark.parametrize("case", range(len(EDGE)), ids=[e[0] for e in EDGE])
def test_edge_scenes(case):
    name, spheres, shifts, csx, csy, edge = EDGE[case]
    dim = rt_ref.EDGE_DIM
    touch, counts, lit = _check_conservative(spheres, shifts, dim, csx, csy)
    assert lit                                                              # the ordinary spheres at least
    e = touch[:, :, edge]
    cov = [rt_ref.coverage(spheres, shifts, dim, csx, csy, which=int(i)) for i in edge]
    if name in ("radius 0", "radius smallest denormal"):
        assert not e.any() and cov == [0.0]                                 # rr = 0: mx*mx + my*my >= 0 everywhere
    elif name == "radius -17.5":
        pos = spheres.copy(); pos["radius"] = np.abs(pos["radius"])
        assert np.array_equal(touch, rt_ref.tile_touch(pos, shifts, dim)) and 0.05 < cov[0] < 0.07    # pi 17.5^2 / 128^2
        assert np.array_equal(oracle.rt_render(spheres, shifts, dim), oracle.rt_render(pos, shifts, dim))
    elif name == "radius 1e19":
        assert e.all() and cov == [1.0]
    elif name[0] in "xy" and "NaN" not in name:
        assert 0.01 < cov[0] < 0.99, cov                                    # the rim crosses the screen
        assert e.any()
    elif name in ("z -inf", "z NaN", "z -2e10"):
        assert 0.2 < cov[0] < 0.4 and e.all()                               # hit and binned (neither reads z) -- and never visible: t > maxz fails
        assert np.array_equal(oracle.rt_render(spheres, shifts, dim), oracle.rt_render(spheres[:6], shifts[:6], dim))
    elif name == "z +inf twice":
        img = oracle.rt_render(spheres, shifts, dim)
        both = _alone(spheres, shifts, dim, 0, 0, 6) & _alone(spheres, shifts, dim, 0, 0, 7)
        assert both.sum() > 1000 and np.array_equal(img[both], oracle.rt_render(spheres[:7], shifts[:7], dim)[both])     # t = +inf twice: the lowest index wins
        assert not np.array_equal(img, oracle.rt_render(spheres[:7], shifts[:7], dim))
    elif name == "x NaN":
        assert cov == [0.0] and e.all()                                     # m = 0 on the NaN axis; the other axis (cy = 0, radius 40) touches both tile rows
    elif name == "y NaN":
        assert cov == [0.0] and e.all()
    elif "radius NaN" in name:
        assert cov == [0.0] and e.all()                                     # !(anything >= NaN): kept everywhere
    else:                                                                   # shifts and camera offsets beyond 2^24: the sphere is on the screen
        assert all(0.02 < c < 0.9 for c in cov), cov
        assert e.any(axis=(0, 1)).all()


def _old_loop_scene_max(shake):
    """The largest tile count over the 18 frames that test_animation_loop_in_one_launch_per_frame_equals_the_kernel_sequence renders in its fused loops
    (loops of 1, 2, 3, 7, 1, 4 frames: sphere_scene(700, 512, 13), update_prob 3, max_speed 18, shake_width 35, camera offsets 2, -3)."""
    n, dim = 700, 512
    spheres, _ = synth.sphere_scene(n, dim, seed=13)
    ref = oracle.RtAnim(n)
    best = 0
    for _ in range(18):
        if shake == 1:
            ref.axis_move(35)
        elif shake == 2:
            ref.curve_move(); ref.speed_angle(3, 18)
        best = max(best, int(rt_ref.tile_counts(spheres, ref.shifts, dim, 2, -3).max()))
    return best


def test_the_old_loop_scene_never_reached_the_super_tile_path():
    got = {shake: _old_loop_scene_max(shake) for shake in (2, 1, 0)}
    assert got == {2: 44, 1: 41, 0: 35}, got                                # the figures of this file's docstring
    assert max(got.values()) < rt_ref.TILE_CAP
