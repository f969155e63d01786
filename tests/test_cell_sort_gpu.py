"""The two forms of the hybrid sort's global stage (cd_sort.h): the two onesweep passes ("classic") and the one launch that places every key by
its cell of the 16 global key bits (k_cell_scatter, "cells").  The order inside a cell differs between the forms and, by cells, from run to
run; what the sort hands back -- keys AND permutation -- must not: k_local_sort orders every run completely, full-key ties by triangle number.
CD_DBG_SORT_CELLS forces either form; left alone, the host takes the cells from the step after one whose triangles came in coherent order."""
import numpy as np
import pytest

import mi355_synth as synth
import mi355cd
import oracle
import records_inputs as ri

pytestmark = pytest.mark.gpu

CLASSIC, CELLS = 1, 2


def _every_key_equal(n=2800):
    """All centroids exactly one point (test_cd_gpu.py test_every_morton_key_equal's construction): one Morton key."""
    i = np.arange(n, dtype=np.float64)
    c = np.array([1.0, 0.0, 0.5])
    a = np.stack([(i % 97 + 1) * 2.0 ** -12, (i // 97 + 1) * 2.0 ** -13, np.zeros(n)], axis=1)
    b = np.stack([np.zeros(n), (i % 89 + 1) * 2.0 ** -12, (i // 89 + 1) * 2.0 ** -13], axis=1)
    verts = np.stack([c + a, c + b, c - a - b], axis=1).reshape(-1, 3)
    return verts, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def _sorted(verts, vidx, form):
    """cd_morton_sort in the reference frame with the global stage forced: keys, permutation, digits ordered globally, the stage's form, the sort's form."""
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        cd.debug_set(mi355cd.CD_DBG_SORT_CELLS, form)
        cd.morton_sort()
        keys, perm = cd.export_keys()
        return keys, perm, cd.stats().sort_passes, cd.debug_get(mi355cd.CD_DBG_GET_SORT_CELLS), cd.debug_get(mi355cd.CD_DBG_GET_SORT_FORM)


def _agree(verts, vidx, passes=2):
    ka, pa, npa, cells_a, form_a = _sorted(verts, vidx, CLASSIC)
    kb, pb, npb, cells_b, form_b = _sorted(verts, vidx, CELLS)
    assert np.array_equal(ka, kb), "keys: cells != classic"
    assert np.array_equal(pa, pb), "permutation: cells != classic"
    assert npa == npb == passes and form_a == form_b, ("escalation", npa, npb, form_a, form_b)
    assert cells_a == 0 and cells_b == (1 if passes == 2 else 0)           # (the forms beyond the hybrid ones have no cells)
    r_keys, r_perm = oracle.sort_by_key(oracle.centroid_morton(verts, vidx))
    assert np.array_equal(ka, r_keys) and np.array_equal(pa, r_perm), "differs from the oracle's stable sort"
    return ka, pa


def test_cloth_of_ten_tiles():
    verts, vidx = synth.cloth_pair(100)
    assert vidx.shape[0] == 40000
    _agree(verts, vidx)


def test_soup_every_wave_past_the_loops_cap():
    verts, vidx = synth.soup(10000, 0.02, 71)
    top = (oracle.centroid_morton(verts, vidx) >> np.uint64(44)).astype(np.int64)
    per_wave = [len(np.unique(top[i:i + 64])) for i in range(0, 10000 - 63, 64)]
    assert min(per_wave) > 8, min(per_wave)                                 # CELL_LOOP_CAP: the lanes left over add for themselves
    _agree(verts, vidx)


def test_full_key_ties_come_out_by_triangle_number():
    verts, vidx = ri.mesh("duplicates")
    keys, perm = _agree(verts, vidx)
    ties = np.flatnonzero(keys[1:] == keys[:-1])
    assert len(ties) >= 250 and np.all(perm[ties] < perm[ties + 1])


def test_every_key_equal_escalates_from_both_forms_alike():
    verts, vidx = _every_key_equal()
    assert len(np.unique(oracle.centroid_morton(verts, vidx))) == 1
    keys, perm = _agree(verts, vidx, passes=8)
    assert np.array_equal(perm, np.arange(len(perm), dtype=perm.dtype))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097])
def test_sizes_around_a_wave_and_a_tile(n):
    verts, vidx = synth.soup(n, 0.05, 900 + n)
    _agree(verts, vidx)


def _step(cd, r, passes=2):
    pairs, n, rc = cd.self_collide(cap=1 << 20)
    assert rc == 0 and n == r["stats"].n_pairs and cd.stats().pairs_tested == r["stats"].pairs_tested
    assert np.array_equal(oracle.pair_set(pairs), oracle.pair_set(r["pairs"]))
    keys, perm = cd.export_keys()
    assert np.array_equal(keys, r["keys"]) and np.array_equal(perm, r["perm"])
    assert passes is None or cd.stats().sort_passes == passes
    return cd.debug_get(mi355cd.CD_DBG_GET_SORT_FORM), cd.debug_get(mi355cd.CD_DBG_GET_SORT_CELLS), cd.stats().sort_passes


def test_mesh_moved_out_of_a_kept_auto_frame_and_back():
    """CD_FRAME_AUTO's frame kept (a frame with a key layout: k_morton's other instance), then sheet B moved beyond it -- its centroids pile up on the frame's
    edge: long runs of equal key bits, whatever escalation they ask for -- and back: from either form of the global stage the same escalations, step by step,
    and the oracle's keys, permutation and pairs all the way."""
    verts, vidx = synth.cloth_pair(60)
    out = verts.copy(); out[verts.shape[0] // 2:, 0] += 4.0
    off, span, lay = oracle.auto_frame(verts, vidx)
    assert lay != 0
    r_in = oracle.pipeline(verts, vidx, None, off=off, span=span, layout=lay)
    r_out = oracle.pipeline(out, vidx, None, off=off, span=span, layout=lay)
    assert not np.array_equal(r_in["keys"], r_out["keys"])
    seen = {}
    for form in (CLASSIC, CELLS):
        with mi355cd.CollisionDetector(verts, vidx) as cd:
            cd.debug_set(mi355cd.CD_DBG_SORT_CELLS, form)
            cd.set_morton_frame(mi355cd.CD_FRAME_AUTO, None, None)
            log = [_step(cd, r_in)]
            cd.keep_auto_frame()
            log.append(_step(cd, r_in))
            cd.update_vertices(out)
            log += [_step(cd, r_out, None) for _ in range(2)]
            cd.update_vertices(verts)
            log += [_step(cd, r_in, None) for _ in range(3)]
            seen[form] = log
    assert [(f, p) for f, _, p in seen[CLASSIC]] == [(f, p) for f, _, p in seen[CELLS]]
    assert all(c == 0 for _, c, _ in seen[CLASSIC]) and all(c == (1 if p == 2 else 0) for _, c, p in seen[CELLS])


def test_unforced_the_cloth_takes_the_cells_from_its_second_step_and_the_soup_never():
    """The 1 M cloth pair (along 64 consecutive triangles the cell changes 5.7 times on average; a cloth of 100 x 100 quads is too coarse against the 2^16 cells: 22.9)
    and a 10 k soup (64).  The threshold is 8 (CELL_FORM_MAX_MEAN_16, mi355cd.hip)."""
    for (verts, vidx), want in ((synth.cloth_pair(500), [0, 1, 1, 1]), (synth.soup(10000, 0.02, 71), [0, 0, 0, 0])):
        r_keys, r_perm = oracle.sort_by_key(oracle.centroid_morton(verts, vidx))
        waves = (vidx.shape[0] + 63) // 64
        with mi355cd.CollisionDetector(verts, vidx) as cd:
            used = []
            for _ in range(4):
                cd.morton_sort()
                used.append(cd.debug_get(mi355cd.CD_DBG_GET_SORT_CELLS))
                keys, perm = cd.export_keys()
                assert np.array_equal(keys, r_keys) and np.array_equal(perm, r_perm) and cd.stats().sort_passes == 2
            stat = cd.debug_get(mi355cd.CD_DBG_GET_CELL_STAT)
        assert used == want, used
        assert (waves <= stat <= 8 * waves) if want[1] else (8 * waves < stat <= 64 * waves), (stat, waves)


def test_graph_replay_and_stream_agree_across_a_change_of_form():
    verts, vidx = synth.cloth_pair(100)
    r = oracle.pipeline(verts, vidx)
    with mi355cd.CollisionDetector(verts, vidx) as g, mi355cd.CollisionDetector(verts, vidx) as s:
        for cd, graph in ((g, 1), (s, 0)):
            cd.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)
            cd.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
            cd.set_option(mi355cd.CD_OPT_GRAPH, graph)
        used = []
        plan = (0,) * 3 + (CELLS,) * 5 + (CLASSIC,) * 4 + (CELLS,) * 4
        for force in plan:
            for cd in (g, s):
                cd.debug_set(mi355cd.CD_DBG_SORT_CELLS, force)
            a, b = _step(g, r), _step(s, r)
            assert a == b, (force, a, b)
            used.append(a[1])
        assert used == [0] * 3 + [1] * 5 + [0] * 4 + [1] * 4, used          # (this cloth is too coarse for the cells unforced: see above)
        assert g.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) >= 8 and s.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == 0
        assert g.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES) >= 3           # (the form is part of a captured step's key)
