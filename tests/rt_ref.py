"""numpy restatement of the ray tracer's binning DECISION (csrc/mi355rt.hip: prepare_one + may_touch), float32 operation by
float32 operation, in the kernel's order and with no fused multiply-add -- and nothing else: bin_sphere's conservative pixel
range is deliberately NOT restated.  A sphere is entered in a tile's count exactly when may_touch holds for that tile, so
rt_stats.sphere_tests of a binned render is 4096 * (the sum of these counts over the rendered tile rows), whichever of the two
read paths (the tile's own list, or the super-tile's index list re-culled with may_touch) a tile takes.  Test infrastructure."""
from __future__ import annotations

import numpy as np

TILE = 64
TILE_CAP = 48
F32 = np.float32


def prepared(spheres, shifts):
    """prepare_one: cx = x + (float)x_shift, cy likewise (the shift row is the one the sphere's idx names), rr = radius * radius."""
    sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1, 4)
    idx = spheres["idx"]
    with np.errstate(all="ignore"):
        cx = spheres["x"].astype(F32) + sh[idx, 0].astype(F32)
        cy = spheres["y"].astype(F32) + sh[idx, 1].astype(F32)
        rr = spheres["radius"].astype(F32) * spheres["radius"].astype(F32)
    return cx, cy, rr


def _corners(dim, cs):
    """(float)(X0 - dim/2 + cs) and (float)(X0 + 63 - dim/2 + cs) of every tile column (or row): integer sum first, then one rounding."""
    x0 = np.arange(dim // TILE, dtype=np.int64) * TILE - dim // 2 + int(cs)
    assert -2 ** 31 <= x0[0] and x0[-1] + TILE - 1 < 2 ** 31, "the kernel's int arithmetic would overflow"
    return x0.astype(F32), (x0 + (TILE - 1)).astype(F32)


def _m2(lo, hi, c):
    """may_touch's m * m per (tile column, sphere): d0 = lo - c, d1 = hi - c, m = d0 > 0 ? d0 : (d1 < 0 ? d1 : 0).  NaN fails both comparisons: m = 0."""
    with np.errstate(all="ignore"):
        d0 = lo[:, None] - c[None, :]
        d1 = hi[:, None] - c[None, :]
        m = np.where(d0 > F32(0), d0, np.where(d1 < F32(0), d1, F32(0))).astype(F32)
        return m * m


def tile_touch(spheres, shifts, dim, csx=0, csy=0):
    """bool [dim/64 (tile row), dim/64 (tile column), n]: may_touch(sphere, tile) = !(mx*mx + my*my >= rr)."""
    cx, cy, rr = prepared(spheres, shifts)
    mx2 = _m2(*_corners(dim, csx), cx)
    my2 = _m2(*_corners(dim, csy), cy)
    nt = dim // TILE
    out = np.zeros((nt, nt, cx.shape[0]), dtype=bool)
    with np.errstate(all="ignore"):
        for ty in range(nt):
            out[ty] = ~((mx2 + my2[ty][None, :]) >= rr[None, :])
    return out


def tile_counts(spheres, shifts, dim, csx=0, csy=0, rows=None):
    """int64 [dim/64, dim/64]: per tile the number of spheres whose may_touch holds; tile rows outside the pixel rows `rows` = (y0, y1) are 0."""
    cx, cy, rr = prepared(spheres, shifts)
    mx2 = _m2(*_corners(dim, csx), cx)
    my2 = _m2(*_corners(dim, csy), cy)
    nt = dim // TILE
    t0, t1 = (0, nt) if rows is None else (rows[0] // TILE, rows[1] // TILE)
    out = np.zeros((nt, nt), dtype=np.int64)
    with np.errstate(all="ignore"):
        for ty in range(t0, t1):
            out[ty] = (~((mx2 + my2[ty][None, :]) >= rr[None, :])).sum(axis=1)
    return out


def expected_sphere_tests(spheres, shifts, dim, csx=0, csy=0, rows=None):
    """rt_stats.sphere_tests of a binned render of the pixel rows `rows` (None: the whole frame)."""
    return int(TILE * TILE * tile_counts(spheres, shifts, dim, csx, csy, rows).sum())


# ---------------------------------------------------------------- scenes shared by tests/test_rt_ref.py (CPU) and tests/test_rt_lists_gpu.py
from oracle import SPHERE_DTYPE  # noqa: E402


def init_shifts(n):
    """sphere.cuh:54-56: {0, 0, (i % 5 + 1) * 5, (i % 2) * 2 - 1}."""
    sh = np.zeros((n, 4), dtype=np.int32)
    i = np.arange(n)
    sh[:, 2] = (i % 5 + 1) * 5
    sh[:, 3] = (i % 2) * 2 - 1
    return sh


def _ordinary(rng, n, dim, spread=1.0):
    s = np.zeros(n, dtype=SPHERE_DTYPE)
    for c in "rgb":
        s[c] = rng.random(n, dtype=np.float32)
    for c in "xyz":
        s[c] = ((rng.random(n) - 0.5) * dim * spread).astype(F32)
    s["radius"] = (rng.random(n) * 20.0 + 8.0).astype(F32)
    return s


def capacity_scene(dim, clusters, n_background=20, seed=0, keep_clear=()):
    """`clusters`: [(tile row, tile column, k)] -- k spheres of radius 3, centres at least 6 pixels inside the tile (each touches that tile only),
    distinct colours, varied z, the first two of a cluster exact duplicates (a tie in t on every pixel they cover).  `n_background` small spheres
    that touch neither a cluster's tile nor a tile of `keep_clear`.  The array order is shuffled; idx = position.  Camera offsets 0.
    Returns spheres, shifts, member[len(clusters)][k] (positions of each cluster's spheres; member[c][0] and [1] are the duplicates)."""
    rng = np.random.default_rng(seed)
    parts, tag = [], []
    for c, (ty, tx, k) in enumerate(clusters):
        s = np.zeros(k, dtype=SPHERE_DTYPE)
        s["x"] = (tx * TILE + 6 + rng.random(k) * 51 - dim // 2).astype(F32)
        s["y"] = (ty * TILE + 6 + rng.random(k) * 51 - dim // 2).astype(F32)
        s["z"] = (rng.random(k) * 200 - 100).astype(F32)
        s["radius"] = 3.0
        for ch in "rgb":
            s[ch] = (0.2 + 0.8 * rng.random(k)).astype(F32)
        col = (s["r"][1], s["g"][1], s["b"][1])
        s[1] = s[0]
        s["r"][1], s["g"][1], s["b"][1] = col
        parts.append(s); tag += [c] * k
    clear = [(ty, tx) for ty, tx, _ in clusters] + list(keep_clear)
    bg = np.zeros(n_background, dtype=SPHERE_DTYPE)
    m = 0
    while m < n_background:
        px, py, rad = rng.random() * dim, rng.random() * dim, 4.0 + 6.0 * rng.random()
        if any(tx * TILE - rad - 3 < px < tx * TILE + TILE + rad + 3 and ty * TILE - rad - 3 < py < ty * TILE + TILE + rad + 3 for ty, tx in clear):
            continue
        bg[m]["x"], bg[m]["y"], bg[m]["z"], bg[m]["radius"] = px - dim // 2, py - dim // 2, rng.random() * 200 - 100, rad
        bg[m]["r"], bg[m]["g"], bg[m]["b"] = rng.random(3)
        m += 1
    parts.append(bg); tag += [-1] * n_background
    s = np.concatenate(parts)
    tag = np.array(tag)
    order = rng.permutation(s.shape[0])
    where = np.argsort(order)                                              # where[j]: the position record j went to
    s = s[order]
    s["idx"] = np.arange(s.shape[0], dtype=np.int32)
    return s, init_shifts(s.shape[0]), [where[tag == c] for c in range(len(clusters))]


def moved(shifts, member, dty, dtx):
    """The spheres `member` moved by whole tiles through their shift rows."""
    sh = shifts.copy()
    sh[member, 0] += TILE * dtx
    sh[member, 1] += TILE * dty
    return sh


def hit_mask(spheres, shifts, dim, csx=0, csy=0, which=0):
    """bool [dim, dim]: the pixels where the oracle's Sphere::hit holds for sphere `which`, whatever its colour, its z and the shading factor (the
    rim of a very large sphere shades to 0).  The sphere is rendered alone, black and with z = +inf, in front of a white backdrop that covers every
    pixel with shading factor 1 (radius 1e19): the black pixels are the hits."""
    import oracle
    s = np.zeros(2, dtype=SPHERE_DTYPE)
    s[0] = spheres[which]
    s[0]["r"] = s[0]["g"] = s[0]["b"] = 0.0
    s[0]["z"] = np.inf
    s[1]["r"] = s[1]["g"] = s[1]["b"] = 1.0
    s[1]["x"], s[1]["y"], s[1]["z"], s[1]["radius"] = csx, csy, -1e19, 1e19
    s["idx"] = (0, 1)
    sh = np.zeros((2, 4), dtype=np.int32)
    sh[0] = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1, 4)[spheres["idx"][which]]
    img = oracle.rt_render(s, sh, dim, csx, csy)
    assert ((img[..., :3] == 0).all(axis=2) | (img[..., :3] == 255).all(axis=2)).all()
    return (img[..., :3] == 0).all(axis=2)


def coverage(spheres, shifts, dim, csx=0, csy=0, which=0):
    """Fraction of the frame's pixels that sphere `which` hits (oracle)."""
    return float(hit_mask(spheres, shifts, dim, csx, csy, which).mean())


def rim_radius(x, y, dim, csx=0, csy=0):
    """For a centre far off the screen: the float radius, within a few ulp of the centre's distance, whose rim crosses the dim x dim screen most evenly
    (float spacing at these magnitudes exceeds a pixel, so the oracle decides, not geometry)."""
    s = np.zeros(1, dtype=SPHERE_DTYPE)
    s["x"], s["y"] = x, y
    r = F32(np.hypot(np.float64(x), np.float64(y)))
    cands = [r]
    lo = hi = r
    for _ in range(24):
        lo = np.nextafter(lo, F32(0)); hi = np.nextafter(hi, F32(np.inf)); cands += [lo, hi]
    best, best_cov = None, None
    for c in cands:
        s["radius"] = c
        cov = coverage(s, np.zeros((1, 4), np.int32), dim, csx, csy)
        if best is None or abs(cov - 0.5) < abs(best_cov - 0.5):
            best, best_cov = c, cov
    return F32(best)


EDGE_DIM = 128
P24, P30 = 2 ** 24, 2 ** 30


def edge_scenes():
    """[(name, spheres, shifts, csx, csy, edge)]: dim 128, six ordinary spheres and, AFTER them in index order, the spheres that carry the edge values
    (`edge`: their positions).  Every input keeps C's results defined: colours in [0, 1], radius * radius finite, so n = dz / sr is in [0, 1] and every
    (int)(c * 255) is in range."""
    dim = EDGE_DIM
    base = _ordinary(np.random.default_rng(41), 6, dim)
    out = []

    def add(name, recs, shift_rows=None, csx=0, csy=0):
        k = len(recs)
        s = np.concatenate([base, np.zeros(k, dtype=SPHERE_DTYPE)])
        for j, (x, y, z, rad) in enumerate(recs):
            e = s[6 + j]
            e["x"], e["y"], e["z"], e["radius"] = x, y, z, rad
            e["r"], e["g"], e["b"] = ((1.0, 0.25, 0.5), (0.0, 1.0, 0.75), (0.5, 0.5, 1.0))[j % 3]
        s["idx"] = np.arange(6 + k, dtype=np.int32)
        sh = init_shifts(6 + k)
        if csx or csy:                                                   # the ordinary spheres follow the camera, so the frame is not empty around the edge sphere
            s["x"][:6] += F32(csx); s["y"][:6] += F32(csy)
        for j, row in enumerate(shift_rows or []):
            sh[6 + j, :2] = row
        out.append((name, s, sh, csx, csy, np.arange(6, 6 + k)))

    nan, inf = float("nan"), float("inf")
    add("radius 0", [(3.0, -4.0, 50.0, 0.0)])
    add("radius smallest denormal", [(3.0, -4.0, 50.0, float(np.float32(1e-45)))])
    add("radius -17.5", [(10.0, -20.0, 50.0, -17.5)])
    add("radius 1e19", [(5.0, 7.0, -1e19, 1e19)])                        # t = dz + z is about 0: behind some ordinary spheres, in front of others
    # Centres far off the screen, the radius picked (rim_radius) so that the rim crosses the screen.  At 1e8 floats are 8 apart: dx = fl(ox - cx) takes a
    # new value every 8 columns.  At 3e9 they are 256 apart, more than the 128-pixel screen: dx changes only where ox - cx passes an odd multiple of 128,
    # i.e. at ox = -128 / +128 -- so those scenes move the camera by 100 pixels to put that column on the screen (no radius splits the screen otherwise).
    for name, x, y, cx_, cy_ in (("x +1e8", 1e8, 0.0, 0, 0), ("x -1e8", -1e8, 0.0, 0, 0), ("y +1e8", 0.0, 1e8, 0, 0), ("y -1e8", 0.0, -1e8, 0, 0),
                                 ("x +3e9", 3e9, 0.0, -100, 0), ("x -3e9", -3e9, 0.0, 100, 0), ("y +3e9", 0.0, 3e9, 0, -100), ("y -3e9", 0.0, -3e9, 0, 100),
                                 ("x +1e8 y -1e8", 1e8, -1e8, 0, 0), ("x -3e9 y +3e9", -3e9, 3e9, 100, -100)):
        # z in front: the sphere shades to black (n = dz / sr is tiny at the rim) and hides what it covers
        add(name, [(x, y, 1e6, float(rim_radius(x, y, dim, cx_, cy_)))], None, cx_, cy_)
    add("z +inf twice", [(-20.0, 10.0, inf, 30.0), (-5.0, 15.0, inf, 30.0)])
    add("z -inf", [(0.0, 0.0, -inf, 40.0)])
    add("z NaN", [(0.0, 0.0, nan, 40.0)])
    add("z -2e10", [(0.0, 0.0, -2e10, 40.0)])
    add("x NaN", [(nan, 0.0, 10.0, 40.0)])
    add("y NaN", [(0.0, nan, 10.0, 40.0)])
    add("radius NaN", [(0.0, 0.0, 10.0, nan)])
    add("x and radius NaN", [(nan, 20.0, 10.0, nan)])
    add("shift +(2^24+1)", [(-float(P24) + 10.0, 5.0, 20.0, 30.0), (-20.0, -float(P24) - 10.0, 20.0, 25.0)], [(P24 + 1, 0), (0, P24 + 1)])
    add("shift -(2^24+1)", [(float(P24) - 10.0, 5.0, 20.0, 30.0), (-20.0, float(P24) + 10.0, 20.0, 25.0)], [(-P24 - 1, 0), (0, -P24 - 1)])
    add("shift +2^30", [(-float(P30) + 64.0, 0.0, 20.0, 40.0), (0.0, -float(P30), 20.0, 20.0)], [(P30, 0), (0, P30)])
    add("shift -2^30", [(float(P30) - 64.0, 0.0, 20.0, 40.0), (0.0, float(P30), 20.0, 20.0)], [(-P30, 0), (0, -P30)])
    add("camera +(2^24+3), +(2^24+3)", [(float(P24), float(P24) + 20.0, 20.0, 30.0)], None, P24 + 3, P24 + 3)
    add("camera -(2^24+3), -(2^24+3)", [(-float(P24), -float(P24) - 20.0, 20.0, 30.0)], None, -P24 - 3, -P24 - 3)
    add("camera +(2^24+3), -(2^24+3)", [(float(P24) + 31.0, -float(P24), 20.0, 30.0)], None, P24 + 3, -P24 - 3)
    add("shift +2^30 under camera +(2^24+3)", [(float(P24 - P30), 0.0, 20.0, 35.0)], [(P30, 0)], P24 + 3, 0)
    add("shift -2^30 under camera -(2^24+3)", [(0.0, float(P30 - P24), 20.0, 35.0)], [(0, -P30)], 0, -P24 - 3)
    return out


def anim_step(ref, shake, shake_width=35, update_prob=3, max_speed=18):
    """One frame's move of the spheres on the oracle's animation state (anime_ray.cu:115-125), as rt_anim_loop's `shake` selects it."""
    if shake == 1:
        ref.axis_move(shake_width)
    elif shake == 2:
        ref.curve_move(); ref.speed_angle(update_prob, max_speed)


def loop_cluster_scene(n, dim, tile, frames, shake, csx, csy, seed, radius=14.0):
    """n ordinary spheres, 60 of which (the first 60 whose initial speed is 5 or 10: i % 5 in (0, 1)) are placed so that the path the oracle's animation
    state takes them along over `frames` frames stays around the centre of `tile` = (row, column): each is centred on its own path's bounding box.
    Whether they do stay is for the caller to assert with tile_counts.  Returns spheres, ids of the 60."""
    import oracle
    rng = np.random.default_rng(seed)
    s = _ordinary(rng, n, dim)
    s["idx"] = np.arange(n, dtype=np.int32)
    ids = np.array([i for i in range(n) if i % 5 in (0, 1)][:60])
    assert ids.shape[0] == 60
    ref = oracle.RtAnim(n)
    path = []
    for _ in range(frames):
        anim_step(ref, shake)
        path.append(ref.shifts[ids, :2].copy())
    path = np.array(path)
    mid = (path.min(axis=0) + path.max(axis=0)) // 2
    jit = rng.integers(-8, 9, size=(60, 2))
    ty, tx = tile
    s["x"][ids] = tx * TILE + 32 - dim // 2 + csx + jit[:, 0] - mid[:, 0]
    s["y"][ids] = ty * TILE + 32 - dim // 2 + csy + jit[:, 1] - mid[:, 1]
    s["radius"][ids] = radius
    return s, ids
