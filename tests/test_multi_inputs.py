"""The cases of tests/multi_inputs.py reach what they are there for, shown with the oracle alone (no GPU): every condition the GPU tests
of tests/test_multi_step_gpu.py rely on is asserted here on the inputs, and the comparison the child-process driver applies to a
step's results (multi_inputs.compare) passes on the right results and fails on planted errors -- planted in the DATA handed to it."""
from __future__ import annotations

import numpy as np
import pytest

import mi355_multi as multi
import mi355_synth as synth
import mi355cd
import multi_inputs as mu
import oracle


def _ids(run):
    return [r.ids for r in run.ranks]


@pytest.mark.parametrize("name", mu.NAMES)
def test_every_case_is_small_and_its_right_results_pass_the_comparison(name):
    c = mu.case(name)
    assert 2 <= c.world <= 4
    for k, run in enumerate(c.runs):
        assert len(run.ranks) == c.world and all(r.vidx.shape[0] <= 25_000 for r in run.ranks)
        for r in run.ranks:
            assert np.isfinite(r.verts).all() and np.unique(r.vidx).size == r.verts.shape[0]          # every vertex belongs to a triangle
        for it, st in enumerate(run.steps):
            w = mu.want(name, k, it)
            assert w.peers == w.box_peers, (run.name, it)            # n_peers counts exchanges: here the same as what the root boxes say
            assert w.peers == [sum(1 for p in range(c.world) if p != a and multi.boxes_overlap(w.roots[a], w.roots[p])) for a in range(c.world)]
            assert max(x.size for x in w.local) + max(x.size for x in w.cross) < run.cap
            ck = mu.compare(w, mu.perfect(w, st.caps, st.null, run.cap), _ids(run))
            assert all(ck.values()), (run.name, it, ck)
            print(f"{name}/{run.name} step {it}: triangles {[r.vidx.shape[0] for r in run.ranks]}, pairs {w.pairs.size}, local {[x.size for x in w.local]}, "
                  f"cross {[x.size for x in w.cross]}, sent {w.sent}, peers {w.peers}, pairs_tested {w.tested}")


def test_soup_ids_and_cross_pairs():
    run = mu.case("soup").runs[0]
    w = mu.want("soup", 0, 0)
    assert sum(x.size for x in w.cross) >= 100 and all(x.size > 0 for x in w.cross)
    ids = np.concatenate(_ids(run))
    assert ids.min() == 0 and ids.max() == 0xFFFFFFFF and np.unique(ids).size == ids.size
    owner = np.concatenate([np.full(r.ids.size, k) for k, r in enumerate(run.ranks)])[np.argsort(ids)]
    assert (owner[:-1] != owner[1:]).all()                              # in ID order no two neighbours belong to one rank: nobody holds a block
    assert all(not np.array_equal(r.ids, np.sort(r.ids)) for r in run.ranks)
    assert [r.options["frame"][0] for r in run.ranks] == [mi355cd.CD_FRAME_REFERENCE, mi355cd.CD_FRAME_AUTO, mi355cd.CD_FRAME_CUSTOM]
    off, span = run.ranks[2].options["frame"][1:]
    assert int((oracle.centroid_morton(run.ranks[2].verts, run.ranks[2].vidx, off, span) >> np.uint64(60)).max()) == 0     # inside its custom frame


def test_double_runs_tie_as_the_cross_pass_test_does():
    c = mu.case("double")
    assert [r.name for r in c.runs] == ["float", "double", "double-coarse-cells", "float-vs-double-no-table"]
    for k, run in enumerate(c.runs):
        w = mu.want("double", k, 0)
        nt = run.ranks[0].vidx.shape[0]
        assert w.pairs.size > 1000 and sum(w.sent) > nt, (run.name, w.pairs.size, w.sent)
        is32 = [np.array_equal(r.verts.astype(np.float32).astype(np.float64), r.verts) for r in run.ranks]
        assert is32 == {"float": [True, True], "float-vs-double-no-table": [True, False]}.get(run.name, [False, False])
    assert c.runs[3].ranks[1].options[mi355cd.CD_OPT_CELL_TABLE] == 0 and mi355cd.CD_OPT_CELL_TABLE not in c.runs[3].ranks[0].options


def test_shared_vertices_need_the_gate_on_global_indices():
    run = mu.case("shared-vertices").runs[0]
    r0, r1 = run.ranks
    shared = r0.vbase + r0.verts.shape[0] - r1.vbase
    assert shared == 2 * (mu.SHARED_QUADS + 1) and np.array_equal(r0.verts[-shared:], r1.verts[:shared])
    w, ungated = mu.want("shared-vertices", 0, 0), mu.expected(run.ranks, share=False)
    v, t = mu.shared_cloth()
    assert np.array_equal(w.pairs, oracle.pair_set(oracle.pipeline(v, t)["pairs"]))           # the merged reference IS the uncut mesh
    only = np.setdiff1d(ungated.pairs, w.pairs)
    assert only.size >= 1 and np.setdiff1d(w.pairs, ungated.pairs).size == 0
    # every pair the gate removes is between the two ranks, its boxes overlap strictly and the triangles share a global vertex
    verts, vidx, ids, owner = mu.merged(run.ranks)
    at = {int(i): k for k, i in enumerate(ids)}
    boxes = mu.tri_boxes(verts, vidx)
    for key in only:
        a, b = at[int(key >> np.uint64(32))], at[int(key & np.uint64(0xFFFFFFFF))]
        assert owner[a] != owner[b] and mu._overlap(boxes[a], boxes[b]) and np.intersect1d(vidx[a], vidx[b]).size >= 1
    print(f"shared-vertices: {only.size} pairs across the cut reported only when the column's vertices get two indices each")


def test_variants_every_rank_owns_cross_pairs():
    c = mu.case("variants")
    assert [[r.options[mi355cd.CD_OPT_TRAVERSAL] for r in run.ranks] for run in c.runs] == [[0, 1, 3], [0, 0, 0]]
    for k in range(2):
        assert all(x.size > 0 for x in mu.want("variants", k, 0).cross)


def test_tiny_rank_of_one_triangle_sends_to_all_and_owns_nothing():
    c = mu.case("tiny")
    run = c.runs[0]
    assert [[r.options.get(mi355cd.CD_OPT_TRAVERSAL) for r in x.ranks] for x in c.runs] == [[None] * 4, [0] * 4]
    assert all(np.array_equal(a.verts, b.verts) and np.array_equal(a.ids, b.ids) for a, b in zip(c.runs[0].ranks, c.runs[1].ranks))
    w = mu.want("tiny", 0, 0)
    assert [r.vidx.shape[0] for r in run.ranks] == [1, 2, 65, 2 * 2 * 20 * 20] and int(run.ranks[0].ids[0]) == 0
    assert w.sent[0] == 3 and w.peers[0] == 3 and w.cross[0].size == 0 and w.local[0].size == 0
    for r in (1, 2, 3):
        assert int(((w.cross[r] >> np.uint64(32)) == 0).sum()) >= 1, r                             # a pair (0, its triangle)


def test_deep_combs_overflow_the_descents_stack():
    c = mu.case("deep")
    for run in c.runs:
        r0 = run.ranks[0]
        mode, off, span = r0.options["frame"]
        assert mode == mi355cd.CD_FRAME_CUSTOM and np.array_equal(off, np.zeros(3)) and np.array_equal(span, np.full(3, 2.0 ** 20))
        tree = oracle.pipeline(r0.verts, r0.vidx, r0.ids, off=off, span=span)
        sp = np.asarray(mu.spanning_triangle(run.name == "local-only"), dtype=np.float64)
        depth = mu.pending_subtrees(tree, mu.tri_boxes(sp, np.arange(3)[None])[0])
        # (the oracle's own max_stack follows the reference's order -- push both, pop right -- which this comb does not trouble:
        #  test_deep_tree_uses_the_deferred_stack_path takes its bound of 32 from the MIRRORED comb for that reason)
        assert depth > mu.DEEP_STACK_BOUND, (run.name, depth)
        if run.name == "local-only":
            assert int(tree["perm"][0]) == r0.vidx.shape[0] - 1                                # the spanning triangle sorts first
        print(f"deep/{run.name}: {depth} subtrees pending at once for the spanning query")
    a, b = (mu.want("deep", k, 0) for k in range(2))
    assert a.cross[0].size >= 40 and a.recv[0] == mu.DEEP_SPANNING + 3 and a.sent[1] == a.recv[0] and b.cross[1].size >= 1 and b.recv[0] == 4 and b.cross[0].size == 0


def test_dense_overflows_a_shard_of_the_cross_pass():
    """Rank 1's pass over the received queries overflows its candidate shards, and NOTHING else sends a pass of either rank to
    run_traversal: no stack fills, no other shard overflows (multi_inputs: the descents restated on the oracle's tree)."""
    run = mu.case("dense").runs[0]
    r0, r1 = run.ranks
    w = mu.want("dense", 0, 0)
    assert r0.vidx.shape[0] <= 1024                                     # one pack workgroup: rank 0's queries arrive in triangle order
    assert max(w.sent) <= run.qcap and w.sent[1] == mu.DENSE_SMALL and w.sent[0] > 64
    assert r0.ids.max() < r1.ids.min() and w.cross[0].size == 0 and w.cross[1].size > 0
    assert all(np.array_equal(r.verts.astype(np.float32).astype(np.float64), r.verts) and np.unique(r.vidx).size == r.vidx.size for r in run.ranks)
    assert all(r.options == mu.AUTO for r in run.ranks)
    trees = [mu.auto_tree(r) for r in run.ranks]
    # the cross pass of rank 1: every leaf hit of a query of rank 0 is kept (its ID is the smaller, no shared vertex): one slot each
    depth, hits = mu.received_descent(trees[1], mu.sent_boxes(run.ranks, 0, 1))
    groups = mu.groups_of_64(hits)
    assert hits.size == w.sent[0] and depth <= mu.WQ_STACK and groups.max() > mu.DENSE_SHARD, (depth, groups)
    # ... and of rank 0: nothing is kept (the queries' IDs are the larger), whatever the order the 8192 arrive in
    depth0, _ = mu.received_descent(trees[0], mu.sent_boxes(run.ranks, 1, 0))
    assert depth0 <= mu.WQ_STACK
    # the local passes: a kept candidate takes four slots; at most 64 workgroups a shard's worth each when nt <= 4096, else several groups
    # share a shard -- bounded by ALL of them together
    for r, tree in zip(run.ranks, trees):
        d, h = mu.half_traversal(tree)
        per_shard = mu.groups_of_64(h).max() if r.vidx.shape[0] <= 4096 else h.sum()
        assert d <= mu.HALF_STACK and 4 * per_shard <= mu.DENSE_SHARD, (d, per_shard)
        print(f"dense: rank of {r.vidx.shape[0]}: half traversal's fullest stack {d} of {mu.HALF_STACK}, {4 * per_shard} slots of {mu.DENSE_SHARD}")
    # the smallest power of two on rank 1 for which a shard overflows
    v, t = synth.soup(mu.DENSE_SMALL // 2, mu.DENSE_SMALL_E, seed=42)
    half = [r0, r1._replace(verts=v, vidx=t, ids=r1.ids[:t.shape[0]])]
    below = mu.groups_of_64(mu.received_descent(mu.auto_tree(half[1]), mu.sent_boxes(half, 0, 1))[1])
    assert below.max() <= mu.DENSE_SHARD
    print(f"dense: received queries' fullest stack {depth} and {depth0} of {mu.WQ_STACK}; slots a wave of 64 queries {groups.tolist()} against {mu.DENSE_SHARD}; "
          f"with {mu.DENSE_SMALL // 2} triangles on rank 1 {below.tolist()}")


def test_sort_redo_keys():
    c = mu.case("sort-redo")
    r0 = c.runs[0].ranks[0]
    assert np.unique(oracle.centroid_morton(r0.verts, r0.vidx)).size == 1 and r0.options["frame"][0] == mi355cd.CD_FRAME_REFERENCE
    w = mu.want("sort-redo", 0, 0)
    assert w.local[0].size == mu.EQUAL_N * (mu.EQUAL_N - 1) // 2 > mu.spec_pairs() and w.cross[1].size > 0
    run = c.runs[1]
    mode, off, span = run.ranks[1].options["frame"]
    assert mode == mi355cd.CD_FRAME_CUSTOM
    above = []
    for it in range(len(run.steps)):
        v = mu.verts_at(run, it)[1]
        keys = oracle.centroid_morton(run.ranks[1].verts if v is None else v, run.ranks[1].vidx, off, span)
        above.append(int((keys >> np.uint64(60)).max()) > 0)
        assert mu.want("sort-redo", 1, it).cross[1].size > 0
    assert above == [False, True, True, False]


def test_caps_cross_every_branch_below_spec_pairs():
    c = mu.case("caps")
    w = mu.want("caps", 0, 0)
    L, X = int(w.local[mu.CAPS_RANK].size), int(w.cross[mu.CAPS_RANK].size)
    assert L >= 70 and X >= 70
    assert mu.spec_pairs() == 1 << 15
    # SPEC_PAIRS itself is out of a cloth shard's reach at the size a rank may have here (the case's docstring): the largest allowed one
    big = mu.expected(mu._cloth_ranks(79, (0, 0.9)))
    assert 2 * 2 * 79 * 79 <= 25_000 < 2 * 2 * 80 * 80 and max(x.size for x in big.local) + max(x.size for x in big.cross) < mu.spec_pairs()
    caps = [st.caps[mu.CAPS_RANK] for st in c.runs[0].steps]
    assert caps == [0, 0, 1, L - 1, L, L + 1, L + X - 1, L + X, None] and [bool(st.null[mu.CAPS_RANK]) for st in c.runs[0].steps] == [True] + [False] * 8
    assert all(st.caps[1 - mu.CAPS_RANK] is None for st in c.runs[0].steps)
    print(f"caps: local {L}, cross {X} on rank {mu.CAPS_RANK}; SPEC_PAIRS {mu.spec_pairs()}; the largest cloth shard allowed has {[x.size for x in big.local]} + {[x.size for x in big.cross]} pairs")


def test_caps_past_spec_pairs_on_the_fast_path():
    """The second run of caps: both of the capped rank's lists are longer than SPEC_PAIRS, its caps lie on either side of every
    comparison of the two separate device copies, and neither rank has a reason to leave the fast path (no stack fills, no shard
    overflows: multi_inputs' restated descents) -- so those copies are cd_multi_step's own, not run_traversal's."""
    run = mu.case("caps").runs[1]
    k, S = mu.CAPS_RANK, mu.spec_pairs()
    w = mu.want("caps", 1, 0)
    L, X = int(w.local[k].size), int(w.cross[k].size)
    assert run.name == "past-spec" and L > S + 1 and X > S + 1 and L + X < run.cap and w.cross[1 - k].size == 0
    caps = [st.caps[k] for st in run.steps]
    assert caps == mu.past_spec_caps(S, L, X) and all(st.caps[1 - k] is None and not st.null for st in run.steps)
    assert S < S + 1 < L - 1 and L + 1 < L + S < L + S + 1 < L + X - 1                      # the caps are distinct and ordered as their comments say
    assert all(r.options == mu.AUTO and r.vidx.shape[0] > 4096 for r in run.ranks)
    for a, r in enumerate(run.ranks):
        tree = mu.auto_tree(r)
        d, h = mu.half_traversal(tree)
        peer = run.ranks[1 - a]
        dx, hx = mu.received_descent(tree, mu.tri_boxes(peer.verts, peer.vidx))
        # slots: a workgroup has 64 queries and shard b & 63, so ceil(n / 4096) workgroups share a shard: four slots a candidate in the local
        # pass, one in the other -- bounded by the fullest workgroup there can be
        share = -(-r.vidx.shape[0] // 4096)
        assert d <= mu.HALF_STACK and dx <= mu.WQ_STACK, (d, dx)
        assert 4 * mu.groups_of_64(h).max() * share <= mu.DENSE_SHARD and 64 * hx.max() * -(-hx.size // 4096) <= mu.DENSE_SHARD
        print(f"caps/past-spec rank {a}: {r.vidx.shape[0]} triangles, fullest stacks {d} of {mu.HALF_STACK} and {dx} of {mu.WQ_STACK}")
    print(f"caps/past-spec: local {L}, cross {X}, SPEC_PAIRS {S}, caps {caps}")


def test_moving_touches_exactly():
    run = mu.case("moving").runs[0]
    wants = [mu.want("moving", 0, it) for it in range(4)]
    assert [sum(x.size for x in w.cross) > 0 for w in wants] == [True, False, False, True]
    assert [w.peers for w in wants] == [[1, 1], [0, 0], [0, 0], [1, 1]]
    touch = run.steps[1].updates[1]
    assert touch[:, 0].min() == run.ranks[0].verts[:, 0].max() and np.array_equal(touch.astype(np.float32).astype(np.float64), touch)
    assert wants[1].roots[1][0] == wants[1].roots[0][1] and not multi.boxes_overlap(wants[1].roots[0], wants[1].roots[1])
    assert wants[2].roots[1][0] > wants[2].roots[0][1]


def test_queries_after_frames_differ():
    """The frames test_queries_after steps through have different right answers: for the step, the root box, proximity, points and rays
    test_moving_inputs.py shows it on the whole jitter sequence; here for cd_points_within's rows, and that the dense frame is among them."""
    import moving_inputs as mi
    import within_ref as wr
    assert mu.QA_NAME == "jitter" and mi.JITTER_DENSE_FRAME < mu.QA_FRAMES <= len(mi.seq(mu.QA_NAME))
    for f in range(mu.QA_FRAMES):
        w = mu.want_within(f)
        wr.same_rows(w, w, f)
        assert w.rows.shape[0] > 0 and mi.want_step(mu.QA_NAME, f)["stats"].n_pairs > 0
        if f:
            with pytest.raises(AssertionError):
                wr.same_rows(mu.want_within(f - 1), w, f)


# ---------------------------------------------------------------- the comparison can fail
def _plant(name="variants"):
    run = mu.case(name).runs[0]
    w = mu.want(name, 0, 0)
    return w, mu.perfect(w), _ids(run)


def _failed(ck):
    return sorted(k for k, v in ck.items() if not v)


def test_comparison_rejects_a_cross_pair_reported_by_the_wrong_side():
    """Rank 1's first cross pair -- with rank 0 or 2 -- leaves rank 1's list and is appended to the list of the OTHER rank of the pair:
    the union, the counts' sum and pairs_tested are all still right."""
    w, res, ids = _plant()
    L = res[1]["info"]["local_pairs"]
    row = res[1]["pairs"][L].copy()
    other = next(k for k in (0, 2) if np.isin(row, ids[k]).any())
    n1 = res[1]["n"]
    res[1]["pairs"][L:n1 - 1] = res[1]["pairs"][L + 1:n1]; res[1]["pairs"][n1 - 1] = mu.CANARY
    res[1]["n"] -= 1; res[1]["info"]["cross_pairs"] -= 1
    res[other]["pairs"][res[other]["n"]] = row
    res[other]["n"] += 1; res[other]["info"]["cross_pairs"] += 1
    ck = mu.compare(w, res, ids)
    assert ck["pair_set_equals_oracle"] and ck["no_duplicates"] and ck["n_counts"] and ck["pairs_tested_equals_single_tree"]
    assert not ck["ownership"] and not ck["segments_are_the_oracles"], _failed(ck)


def test_comparison_rejects_a_duplicated_pair():
    w, res, ids = _plant()
    n = res[2]["n"]
    res[2]["pairs"][n] = res[2]["pairs"][n - 1]
    res[2]["n"] += 1; res[2]["info"]["cross_pairs"] += 1
    ck = mu.compare(w, res, ids)
    assert not ck["no_duplicates"] and not ck["n_is_the_true_count"], _failed(ck)
    # ... also when another rank reports it: the pair of two ranks from BOTH sides
    w, res, ids = _plant()
    L = res[1]["info"]["local_pairs"]
    row = res[1]["pairs"][L].copy()
    other = next(k for k in (0, 2) if np.isin(row, ids[k]).any())
    res[other]["pairs"][res[other]["n"]] = row
    res[other]["n"] += 1; res[other]["info"]["cross_pairs"] += 1
    ck = mu.compare(w, res, ids)
    assert not ck["no_duplicates"] and not ck["ownership"], _failed(ck)


def test_comparison_rejects_a_missing_pair():
    for segment in ("local", "cross"):
        w, res, ids = _plant()
        n, L = res[1]["n"], res[1]["info"]["local_pairs"]
        at = 0 if segment == "local" else L
        res[1]["pairs"][at:n - 1] = res[1]["pairs"][at + 1:n]; res[1]["pairs"][n - 1] = mu.CANARY
        res[1]["n"] -= 1; res[1]["info"][segment + "_pairs"] -= 1
        ck = mu.compare(w, res, ids)
        assert not ck["pair_set_equals_oracle"] and not ck["segments_are_the_oracles"] and not ck["n_is_the_true_count"] and ck["n_counts"], (segment, _failed(ck))


def test_comparison_rejects_pairs_tested_off_by_two():
    for d in (2, -2):
        w, res, ids = _plant()
        res[0]["info"]["pairs_tested"] += d
        assert _failed(mu.compare(w, res, ids)) == ["pairs_tested_equals_single_tree"]


def test_comparison_rejects_errors_of_a_capped_step():
    """The capped rank of the caps case: a row written behind cap, a wrong return code, a count that is not the true one, rows that are not
    the local pairs first."""
    c = mu.case("caps")
    w, ids = mu.want("caps", 0, 0), _ids(c.runs[0])
    k = mu.CAPS_RANK
    for it, st in enumerate(c.runs[0].steps[:-1]):
        def fresh():
            return mu.perfect(w, st.caps, st.null)
        assert all(mu.compare(w, fresh(), ids).values())
        cap = st.caps[k]
        res = fresh(); res[k]["rc"] = 0 if res[k]["rc"] else mi355cd.CD_OVERFLOW
        assert _failed(mu.compare(w, res, ids)) == ["rc_overflow_exactly_when_n_exceeds_cap"], it
        res = fresh(); res[k]["n"] = min(res[k]["n"], cap) if cap < res[k]["n"] else res[k]["n"] + 1
        assert "n_is_the_true_count" in _failed(mu.compare(w, res, ids)), it
        if not st.null[k]:
            res = fresh(); res[k]["pairs"][cap] = res[k]["pairs"][0] if cap else (1, 2)
            assert _failed(mu.compare(w, res, ids)) == ["canary_behind_cap"], it
        if cap >= 1:                                                        # the last row it may write replaced by a pair of the oracle's that is the OTHER rank's
            wrong = w.local[1 - k][0]
            res = fresh(); res[k]["pairs"][cap - 1] = (int(wrong >> np.uint64(32)), int(wrong & np.uint64(0xFFFFFFFF)))
            assert {"segments_are_the_oracles", "ownership"} <= set(_failed(mu.compare(w, res, ids))), it
