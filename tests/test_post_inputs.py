"""CPU checks of tests/post_inputs.py (no GPU): the by-construction pair lists are what the oracle finds on the meshes, the ID maps
are injections with the bytes they promise, and every comparison tests/test_post_gpu.py makes FAILS on a wrong result."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import post_inputs as pi


def _live(m, seed, keep):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.random(m) < keep


SHAPES = {
    "one": lambda: pi.crosses(1),
    "two": lambda: pi.crosses(2),
    "crosses_513": lambda: pi.crosses(513),
    "crosses_4097": lambda: pi.crosses(4097),
    "fans": lambda: pi.crosses(1000, (1, 7, 300, 5000)),
    "fan_only_1025": lambda: pi.crosses(0, (1025,)),
    "live_mask": lambda: pi.crosses(200, (65, 300), live=_live(565, 5, 0.4)),
    "nothing_live": lambda: pi.crosses(30, (9,), live=np.zeros(39, dtype=bool)),
}
COUNTS = {"one": (1, 2), "two": (2, 4), "crosses_513": (513, 1026), "crosses_4097": (4097, 8194), "fans": (6308, 7312), "fan_only_1025": (1025, 1026)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_oracle_finds_exactly_the_constructed_pairs(name):
    m = SHAPES[name]()
    if name in COUNTS:
        assert (m.pairs.shape[0], m.nt) == COUNTS[name]
    assert m.pairs.shape[0] == int(m.live.sum()) and np.all(m.pairs[:, 0] < m.pairs[:, 1])
    assert np.array_equal(m.verts, m.verts.astype(np.float32).astype(np.float64)) and m.verts.min() >= 0 and m.verts.max() < 1
    for map_name in ("identity", "random"):
        ids = pi.ids_for(map_name, m.nt)
        r = oracle.pipeline(m.verts, m.vidx, ids, off=pi.FRAME_OFF, span=pi.FRAME_SPAN)
        assert r["stats"].n_pairs == m.pairs.shape[0]
        pi.same_step((r["pairs"], r["stats"].n_pairs, 0), pi.ordered(m.pairs, ids), name)


def test_large_case_counts():
    """The large case of the GPU tests: 370 000 pairs on 670 001 triangles, against the oracle (about half a second)."""
    m = pi.crosses(300000, (70000,))
    assert m.pairs.shape[0] == 370000 and m.nt == 670001 and m.fans == [(600000, 600001, 70000)]
    r = oracle.pipeline(m.verts, m.vidx, None, off=pi.FRAME_OFF, span=pi.FRAME_SPAN)
    pi.same_step((r["pairs"], r["stats"].n_pairs, 0), pi.ordered(m.pairs, pi.ids_for("identity", m.nt)), "large")


@pytest.mark.parametrize("nt", [2, 3, 257, 8194, 16386, 670001])
def test_id_maps_are_injections(nt):
    i = np.arange(nt, dtype=np.uint64)
    for name in pi.ID_MAPS:
        if (name == "shl12_fff" and nt > 1 << 20):
            continue
        ids = pi.ids_for(name, nt)
        assert ids.dtype == np.uint32 and np.unique(ids).shape[0] == nt, name
    assert np.array_equal(pi.ids_for("reversed", nt), (nt - 1 - i).astype(np.uint32))
    assert np.array_equal(pi.ids_for("shl8", nt), (i << np.uint64(8)).astype(np.uint32))
    if nt <= 1 << 20:
        assert np.array_equal(pi.ids_for("shl12_fff", nt), ((i << np.uint64(12)) | np.uint64(0xFFF)).astype(np.uint32))
    want = np.array([int(format(int(k), "032b")[::-1], 2) for k in i[:300]], dtype=np.uint32)
    assert np.array_equal(pi.ids_for("bitrev", nt)[:300], want)
    rnd = pi.ids_for("random", nt)
    assert 0 in rnd and 0xFFFFFFFF in rnd and np.array_equal(rnd, pi.ids_for("random", nt))
    if nt > 1000:                                                    # every byte of the random IDs takes (nearly) every value
        assert all(np.unique((rnd >> np.uint32(8 * b)) & np.uint32(255)).shape[0] > 250 for b in range(4))


@pytest.mark.parametrize("where", ["smallest", "largest", "middle"])
def test_hub_placement(where):
    m = pi.crosses(5, (1, 64, 7))
    for name in ("identity", "bitrev", "random"):
        ids = pi.place_hubs(pi.ids_for(name, m.nt), m, where)
        assert np.array_equal(np.sort(ids), np.sort(pi.ids_for(name, m.nt)))
        assert np.array_equal(ids[:10], pi.ids_for(name, m.nt)[:10])          # the crosses in front keep theirs
        for hub, first, j in m.fans:
            fan = ids[hub:hub + j + 1]
            assert np.array_equal(np.sort(fan), np.sort(pi.ids_for(name, m.nt)[hub:hub + j + 1]))
            assert int((fan < ids[hub]).sum()) == {"smallest": 0, "largest": j, "middle": j // 2}[where]
            rows = pi.ordered(m.pairs, ids)[5 + sum(jj for _, _, jj in m.fans[:m.fans.index((hub, first, j))]):][:j]
            col = {"smallest": 0, "largest": 1}.get(where)
            if col is not None:
                assert np.all(rows[:, col] == ids[hub])


# ---- every comparison fails on its mutation
def _case():
    m = pi.crosses(40, (9, 3))
    ids = pi.place_hubs(pi.ids_for("bitrev", m.nt), m, "smallest")
    rows = pi.ordered(m.pairs, ids)
    return rows, pi.sort_rows(rows), pi.id_set(rows)


def _fails(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def test_comparisons_accept_the_right_result():
    rows, srt, ids = _case()
    pi.same_sorted_pairs((srt, srt.shape[0], 0), rows)
    pi.same_id_set((ids, ids.shape[0], 0), rows)
    pi.same_step((rows[::-1], rows.shape[0], 0), rows)
    e = np.zeros((0, 2), dtype=np.uint32)
    pi.same_sorted_pairs((e, 0, 0), e)
    pi.same_id_set((np.zeros(0, dtype=np.uint32), 0, 0), e)


def test_sorted_pairs_comparison_fails_on_wrong_lists():
    rows, srt, _ = _case()
    n = srt.shape[0]
    k = n // 2
    swapped = srt.copy(); swapped[[k, k + 1]] = swapped[[k + 1, k]]                     # two adjacent rows swapped
    _fails(pi.same_sorted_pairs, (swapped, n, 0), rows)
    dup = srt.copy(); dup[k + 1] = dup[k]                                              # one row duplicated over its neighbour
    _fails(pi.same_sorted_pairs, (dup, n, 0), rows)
    cols = srt.copy(); cols[k] = cols[k, ::-1]                                         # a pair's two columns swapped
    _fails(pi.same_sorted_pairs, (cols, n, 0), rows)
    _fails(pi.same_sorted_pairs, (np.ascontiguousarray(srt[:, ::-1]), n, 0), rows)     # ... every pair's
    # the right multiset, in order by the first column, unsorted in the second column only: the hub's run (equal first column) reversed
    first, cnt = np.unique(srt[:, 0], return_counts=True)
    a = first[np.argmax(cnt)]
    run = np.flatnonzero(srt[:, 0] == a)
    assert run.shape[0] >= 3
    unsorted = srt.copy(); unsorted[run] = unsorted[run[::-1]]
    assert np.all(np.diff(unsorted[:, 0].astype(np.int64)) >= 0) and np.array_equal(pi.sort_rows(unsorted), srt)
    _fails(pi.same_sorted_pairs, (unsorted, n, 0), rows)
    # a stale tail: the right prefix, then rows of a previous, larger result -- whether n says so or not
    prev = pi.sort_rows(pi.ordered(pi.crosses(80).pairs, pi.ids_for("bitrev", 160)))
    stale = np.concatenate([srt, prev[n:]])
    _fails(pi.same_sorted_pairs, (stale, stale.shape[0], 0), rows)
    _fails(pi.same_sorted_pairs, (stale, n, 0), rows)
    _fails(pi.same_sorted_pairs, (srt, n + 1, 0), rows)
    _fails(pi.same_sorted_pairs, (srt[:-1], n - 1, 0), rows)                           # a row missing
    _fails(pi.same_sorted_pairs, (srt, n, pi.CD_OVERFLOW), rows)
    _fails(pi.same_sorted_pairs, (srt, n, -1005), rows)                                # CD_ERR_SORT
    _fails(pi.same_sorted_pairs, (srt.astype(np.int64), n, 0), rows)


def test_id_set_comparison_fails_on_wrong_sets():
    rows, _, ids = _case()
    n = ids.shape[0]
    k = n // 3
    _fails(pi.same_id_set, (np.delete(ids, k), n - 1, 0), rows)                        # one ID missing
    _fails(pi.same_id_set, (np.delete(ids, k), n, 0), rows)
    _fails(pi.same_id_set, (np.insert(ids, k, ids[k]), n + 1, 0), rows)                # one ID repeated
    rep = ids.copy(); rep[k + 1] = rep[k]
    _fails(pi.same_id_set, (rep, n, 0), rows)
    sw = ids.copy(); sw[[k, k + 1]] = sw[[k + 1, k]]
    _fails(pi.same_id_set, (sw, n, 0), rows)
    low16 = ids[np.concatenate([[True], (ids[1:] & 0xFFFF) != (ids[:-1] & 0xFFFF)])]   # a unique that compares 16 bits only
    if low16.shape[0] != n:
        _fails(pi.same_id_set, (low16, low16.shape[0], 0), rows)
    stale = np.concatenate([ids, ids[-3:] + np.uint32(1)])
    _fails(pi.same_id_set, (stale, n, 0), rows)
    _fails(pi.same_id_set, (ids, n, pi.CD_OVERFLOW), rows)


def test_step_comparison_fails_on_a_wrong_set():
    rows, _, _ = _case()
    n = rows.shape[0]
    _fails(pi.same_step, (rows[:-1], n - 1, 0), rows)
    twice = rows.copy(); twice[0] = twice[1]
    _fails(pi.same_step, (twice, n, 0), rows)
    _fails(pi.same_step, (np.ascontiguousarray(rows[:, ::-1]), n, 0), rows)
