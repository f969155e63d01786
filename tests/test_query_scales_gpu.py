"""Proximity and continuous collision queries at the ends of the fp32 range, far from the origin, and through candidate-buffer growth.

The device's broad phases work in fp32 (stored hi rounded down and bumped in ambiguous cells, [lo, next_up(hi)] on read, pads with
directed rounding); the restatements (tests/proximity_ref.py, tests/ccd_ref.py) evaluate every pair of the meshes here in FP64 and use
no box filter.  The meshes are scaled by 2^k over tests/scale_inputs.SCALES, which runs past FLT_MAX (coordinates in the FLT_MAX and
-FLT_MAX cells, +inf after rounding up) and below the smallest fp32 subnormal; the restatements are equivariant there (pinned on the
CPU), so every scale must give the k = 0 result: the same pairs, distances and toi bits times 2^k (toi unchanged), for both cell-table
settings and both Morton frames, and cd_self_collide the oracle's pairs and pairs tested."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ccd_ref as cr
import mi355_synth as synth
import mi355cd
import oracle
import proximity_ref as pr
import scale_inputs as si

pytestmark = pytest.mark.gpu

MESHES = si.meshes()
FRAMES = ((mi355cd.CD_FRAME_REFERENCE, "reference"), (mi355cd.CD_FRAME_AUTO, "auto"))


def _bits(d):
    return np.asarray(d, dtype=np.float64).view(np.uint64)


def _same_prox(got, want, what):
    gp, gd = pr.sort_pairs(got[0], got[1])
    wp, wd = want
    assert got[3] == mi355cd.CD_OK and got[2] == wp.shape[0], (what, got[2], wp.shape[0])
    assert np.array_equal(gp, wp), what
    bad = np.nonzero(_bits(gd) != _bits(wd))[0]
    assert bad.size == 0, (what, bad.size, gd[bad[:3]], wd[bad[:3]])


def _same_ccd(got, want, what):
    gp, gt, gd = cr.sort_pairs(got[0], got[1], got[2])
    wp, wt, wd = want
    assert got[4] == mi355cd.CD_OK and got[3] == wp.shape[0], (what, got[3], wp.shape[0])
    assert np.array_equal(gp, wp), what
    assert np.array_equal(_bits(gt), _bits(wt)), what
    assert np.array_equal(_bits(gd), _bits(wd)), what


def _prox_dists(edge):
    return (0.0, edge / 4)


def _ccd_dist(edge):
    return edge / 4


@functools.lru_cache(maxsize=None)
def _restated(name, k, shift=0.0):
    """The restatements on mesh `name` scaled by 2^k (translated by `shift` first): {dist: (pairs, dists)} for the proximity
    distances, and (pairs, toi, dists), (tested, evals) for CCD.  Every pair is evaluated (<= pr.BRUTE_MAX triangles)."""
    v, vidx, edge = MESHES[name]
    x1 = si.motion(v, edge)
    if shift:
        v, x1 = v + shift, x1 + shift
    v, x1 = si.scaled(v, k), si.scaled(x1, k)
    assert vidx.shape[0] <= pr.BRUTE_MAX
    dists = [np.ldexp(d, k) for d in _prox_dists(edge)]
    p, d = pr.proximity_pairs(v, vidx, None, max(dists))                  # the smaller distances' pairs are its subsets
    prox = {}
    for dd in dists:
        keep = d <= dd
        prox[dd] = (p[keep], d[keep])
    ccd, counts = cr.ccd_pairs(v, x1, vidx, None, np.ldexp(_ccd_dist(edge), k), counts=True)
    return prox, ccd, counts


def _scaled_want(name, k):
    """What every scale must give: the restatement at k itself on the band's edges, else its k = 0 result scaled by 2^k."""
    if k in si.EDGES:
        return _restated(name, k)
    prox0, (cp, ct, cd), counts = _restated(name, 0)
    prox = {np.ldexp(d, k): (p, np.ldexp(dd, k)) for d, (p, dd) in prox0.items()}
    return prox, (cp, ct, np.ldexp(cd, k)), counts


def _run_all(cd, verts, vidx, x1, edge, k, want, what):
    """Both cell-table settings and both frames: cd_self_collide against the oracle, proximity and CCD against `want`."""
    prox, ccd, (tested, evals) = want
    oracle_ref = {}
    for table in (1, 0):
        cd.set_option(mi355cd.CD_OPT_CELL_TABLE, table)
        for frame, fname in FRAMES:
            w = f"{what} table={table} frame={fname}"
            cd.set_morton_frame(frame)
            if fname not in oracle_ref:
                if frame == mi355cd.CD_FRAME_AUTO:
                    off, span, lay = oracle.auto_frame(verts, vidx)
                    oracle_ref[fname] = oracle.pipeline(verts, vidx, off=off, span=span, layout=lay)
                else:
                    oracle_ref[fname] = oracle.pipeline(verts, vidx)
            r = oracle_ref[fname]
            pairs, n, rc = cd.self_collide(cap=1 << 20)
            assert rc == mi355cd.CD_OK and np.array_equal(oracle.pair_set(pairs), oracle.pair_set(r["pairs"])), w
            assert cd.stats().pairs_tested == r["stats"].pairs_tested, w
            for d, wp in prox.items():                                   # on the tree the collision step built
                _same_prox(cd.find_proximity(d, cap=max(1, 2 * wp[0].shape[0])), wp, f"{w} proximity dist={d!r}")
            d = np.ldexp(_ccd_dist(edge), k)
            _same_ccd(cd.find_ccd(x1, d, cap=max(1, 2 * ccd[0].shape[0])), ccd, f"{w} ccd dist={d!r}")
            assert cd.ccd_info.n_tested == tested and cd.ccd_info.n_evals == evals, (w, cd.ccd_info.n_tested, tested, cd.ccd_info.n_evals, evals)
        d = max(prox)                                                     # the build-and-query entry point too
        _same_prox(cd.self_proximity(d, cap=max(1, 2 * prox[d][0].shape[0])), prox[d], f"{what} table={table} self_proximity")


@pytest.mark.parametrize("k", si.SCALES)
@pytest.mark.parametrize("name", list(MESHES))
def test_scaled_mesh_gives_the_scaled_result(name, k):
    v, vidx, edge = MESHES[name]
    verts, x1 = si.scaled(v, k), si.scaled(si.motion(v, edge), k)
    if k >= 128:                                                          # the range end is really reached: the FLT_MAX cell is ambiguous
        for a in range(3):
            assert np.unique(verts[np.abs(verts[:, a]) > si.FLT_MAX, a]).size >= 2, (name, k, a)
    want = _scaled_want(name, k)
    assert want[0][max(want[0])][0].shape[0] > 0 and want[1][0].shape[0] > 0
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        _run_all(cd, verts, vidx, x1, edge, k, want, f"{name} k={k}")


SHIFT = 2.0 ** 20 + 0.37


@pytest.mark.parametrize("name", list(MESHES))
def test_far_from_origin(name):
    """World coordinates: the meshes translated by 2^20 + 0.37 (the pads' M 2^-20 is then several edges wide), against the
    restatements on every pair."""
    v, vidx, edge = MESHES[name]
    verts, x1 = v + SHIFT, si.motion(v, edge) + SHIFT
    want = _restated(name, 0, SHIFT)
    assert want[0][max(want[0])][0].shape[0] > 0 and want[1][0].shape[0] > 0
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        _run_all(cd, verts, vidx, x1, edge, 0, want, f"{name} shifted")


# ---------------------------------------------------------------- candidate-buffer growth
# Both queries start with shards of max(4096, ceil(16 n / 64)) candidates (mi355cd.hip PairBuf::ensure); a shard that
# overflows is detected, the buffer grows and the pass is redone.  More candidates in all than 64 shards hold forces that path.
NSHARD = 64


def _shard_cap0(n):
    return max(4096, (16 * n + NSHARD - 1) // NSHARD)


@pytest.fixture(scope="module")
def all_pairs_soup():
    """1 500 triangles of private vertices and distances at least the mesh's diameter: every one of the n (n - 1) / 2 pairs is a
    candidate and is reported."""
    v, vidx = si.box_soup(1500, 0.3, 1.0, 3.0, 21)
    x1 = si.motion(v, 0.3, seed=8)
    lo, hi = np.minimum(v.min(0), x1.min(0)), np.maximum(v.max(0), x1.max(0))
    big = float(np.ceil(np.linalg.norm(hi - lo)))                         # >= the diameter at x0, at x1 and in between
    small = 0.05
    p, d = pr.proximity_pairs(v, vidx, None, big)
    prox = {big: (p, d), small: (p[d <= small], d[d <= small])}
    ccd = {dd: cr.ccd_pairs(v, x1, vidx, None, dd) for dd in (big, small)}
    return v, vidx, x1, big, small, prox, ccd


def test_candidate_growth_on_all_pairs(all_pairs_soup):
    v, vidx, x1, big, small, prox, ccd = all_pairs_soup
    n = vidx.shape[0]
    every = n * (n - 1) // 2
    assert every > NSHARD * _shard_cap0(n)
    assert prox[big][0].shape[0] == every and ccd[big][0].shape[0] == every
    cap = every + 16
    with mi355cd.CollisionDetector(v, vidx) as cd:
        cd.build_tree()
        _same_prox(cd.find_proximity(big, cap=cap), prox[big], "proximity, all pairs")
        assert cd.proximity_tested == every
        _same_ccd(cd.find_ccd(x1, big, cap=cap), ccd[big], "ccd, all pairs")
        assert cd.ccd_info.n_candidates == every and cd.ccd_info.n_candidates > NSHARD * _shard_cap0(n)
        assert cd.ccd_info.n_tested == every and cd.ccd_info.n_evals == every          # all apart by <= dist at t = 0: one evaluation
        # the grown buffers serve small queries, and the two queries interleaved keep to their own buffers
        for kind, d in (("prox", small), ("ccd", small), ("prox", big), ("ccd", small), ("prox", small), ("ccd", big), ("prox", small)):
            if kind == "prox":
                _same_prox(cd.find_proximity(d, cap=cap), prox[d], f"proximity dist={d} after growth")
            else:
                _same_ccd(cd.find_ccd(x1, d, cap=cap), ccd[d], f"ccd dist={d} after growth")
        _same_prox(cd.self_proximity(small, cap=cap), prox[small], "self_proximity after growth")
        _same_ccd(cd.self_ccd(x1, small, cap=cap), ccd[small], "self_ccd after growth")


def test_first_query_overflows_behind_the_build(all_pairs_soup):
    """A fresh context whose very first call is a build-and-query entry point: every buffer of the query is allocated by that call,
    the pass behind the build overflows its initial shards, and the redo runs on the grown buffer and the tree just built."""
    v, vidx, x1, big, small, prox, ccd = all_pairs_soup
    n = vidx.shape[0]
    every = n * (n - 1) // 2
    assert every > NSHARD * _shard_cap0(n)
    cap = every + 16
    with mi355cd.CollisionDetector(v, vidx) as cd:
        _same_ccd(cd.self_ccd(x1, big, cap=cap), ccd[big], "self_ccd first, all pairs")
        assert cd.ccd_info.n_candidates == every
        assert cd.debug_swept()[0].shape[0] == n                          # (debug_swept itself refuses a swept tree of another size)
    with mi355cd.CollisionDetector(v, vidx) as cd:
        _same_prox(cd.self_proximity(big, cap=cap), prox[big], "self_proximity first, all pairs")
        assert cd.proximity_tested == every


def test_candidate_growth_above_the_per_triangle_capacity():
    """20 000 triangles (shards of 16 n / 64 candidates) with more than 16 candidates per triangle in all: some shard overflows.
    The restatements on every pair touching 1 500 query triangles."""
    v, vidx = synth.soup(20_000, e=0.1, seed=23)
    n = vidx.shape[0]
    assert _shard_cap0(n) * NSHARD <= 16 * n + NSHARD
    x1 = si.motion(v, 0.1, seed=9)
    dp, dc = 0.08, 0.03
    q = np.random.default_rng(4).choice(n, 1500, replace=False)
    wp = pr.proximity_pairs(v, vidx, None, dp, queries=q)
    wc = cr.ccd_pairs(v, x1, vidx, None, dc, queries=q)
    with mi355cd.CollisionDetector(v, vidx) as cd:
        for step in range(2):                                              # the first call grows the buffers, the second runs on them
            p, dd, npairs, rc = cd.self_proximity(dp, cap=1 << 22)
            # (more candidates than the 64 initial shards hold: one of them overflowed)
            assert rc == mi355cd.CD_OK and npairs == p.shape[0] and cd.proximity_tested > 16 * n, (step, cd.proximity_tested)
            touch = np.isin(p[:, 0], q) | np.isin(p[:, 1], q)
            _same_prox((p[touch], dd[touch], int(touch.sum()), rc), wp, f"proximity step {step}")
            cp, ct, cdd, ncp, rc = cd.find_ccd(x1, dc, cap=1 << 22)
            assert rc == mi355cd.CD_OK and ncp == cp.shape[0] and cd.ccd_info.n_candidates > 16 * n, (step, cd.ccd_info.n_candidates)
            touch = np.isin(cp[:, 0], q) | np.isin(cp[:, 1], q)
            _same_ccd((cp[touch], ct[touch], cdd[touch], int(touch.sum()), rc), wc, f"ccd step {step}")
