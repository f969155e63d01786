"""cd_multi_step on the paths the cloth shards of tests/multi_loopback_driver.py never take: one test per case of
tests/multi_inputs.py.  A case runs in a child process (tests/multi_cases_driver.py: ranks are host threads, the library talks to
tests/loopback_rccl), which judges every step against the oracle on the merged mesh -- per rank the LOCAL segment and the CROSS segment
of its list (so: the union, no duplicate, and each cross pair from the owner of the larger ID), the counts, pairs_tested, the queries
sent and received, the peers, the root box, the rows behind cap -- and prints what each step reported of itself; the tests here assert
that JSON and, per case, the path the step was expected to take.  tests/test_multi_inputs.py shows on the CPU that the inputs reach
what each case is there for.  The last test is in-process: the multi step as a rebuild entry for the queries."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mi355cd
import moving_inputs as mi
import multi_inputs as mu
import oracle
import proximity_ref as pr
import within_ref as wr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OVERFLOW = mi355cd.CD_OVERFLOW


def _case(name):
    p = subprocess.run([sys.executable, os.path.join(HERE, "multi_cases_driver.py"), name], capture_output=True, text=True, timeout=240)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(lines[-1])
    assert "hung" not in res, res
    for run in res.get("runs", []):
        for it, st in enumerate(run["steps"]):
            bad = [k for k, v in st["checks"].items() if not v]
            assert not bad, (name, run["run"], it, bad, {k: v for k, v in st.items() if k not in ("checks", "ms")})
    assert res["ok"] and p.returncode == 0, res
    assert [r["run"] for r in res["runs"]] == [r.name for r in mu.case(name).runs] and res["world"] == mu.case(name).world
    for k, run in enumerate(res["runs"]):
        assert len(run["steps"]) == len(mu.case(name).runs[k].steps)
    return res["runs"]


def _fast(st, r):
    """The step went through the two passes enqueued side by side and nothing else: one host synchronisation per round of the
    collectives, one for both passes; with CD_MULTI_TIMING both passes are timed."""
    return st["host_syncs"][r] == st["attempts"][r] + 1 and st["ms"][r]["ms_local"] > 0 and st["ms"][r]["ms_cross"] >= 0


def _general(st, r, passes):
    """`passes` of the two passes were run again by run_traversal (one more host synchronisation each, plus the copies of a long list and
    the redos of a sort, hence >=), and the step says that its pass timings do not apply."""
    return st["host_syncs"][r] >= st["attempts"][r] + 1 + passes and st["ms"][r]["ms_local"] == -1.0 and st["ms"][r]["ms_cross"] == -1.0


def test_soup():
    """Unstructured triangles, IDs all over uint32 in no order, a REFERENCE, an AUTO and a CUSTOM frame.  Expected: the fast path on every
    rank (3200 triangles a rank are far from any candidate shard's capacity), k_pack_triangles and the cross pass on records of triangles
    that share no vertex; who reports a cross pair follows the IDs alone."""
    for st in _case("soup")[0]["steps"]:
        assert all(_fast(st, r) for r in range(3)) and min(st["cross"]) > 0 and st["n_peers"] == [2, 2, 2], st


def test_double():
    """Box faces that tie on every level of both trees, in fp32 values, full doubles, full doubles in coarse fp32 cells, and fp32 queries
    against a full-double tree without its cell table.  Expected: fast path; step 0 grows the slabs once (every triangle is a query:
    5184 > nt / 8 + 1024) and step 1 keeps them; the received queries meet a tree WITH a cell table in runs 2 and 3."""
    for run in _case("double"):
        s0, s1 = run["steps"]
        assert s0["attempts"] == [2, 2] and s1["attempts"] == [1, 1], run["run"]
        for st in (s0, s1):
            assert _fast(st, 0) and _fast(st, 1) and st["cross"][1] > 1000 and sum(st["sent"]) > 5184, (run["run"], st)


def test_shared_vertices():
    """One mesh cut in two along a vertex column whose vertices both ranks hold under the same global index, with one fold across the cut
    that intersects its neighbour through a shared vertex.  Expected: fast path; neighbor_count sees q.vidx (the sender's local index +
    its base) equal to leaf.v + the receiver's base and drops the pair -- a gate on local indices, or on one base only, reports the
    pairs test_multi_inputs.py counts as well."""
    w = mu.want("shared-vertices", 0, 0)
    for st in _case("shared-vertices")[0]["steps"]:
        assert _fast(st, 0) and _fast(st, 1) and st["cross"] == [x.size for x in w.cross] and min(st["cross"]) > 0, st


def test_variants():
    """CD_OPT_TRAVERSAL 0, 1 and 3 on the three ranks, then 0 on all.  Expected from the code: variant 0 has no candidate stage, so
    `fast_path` is false -- no pass is enqueued beside the exchange, both run through run_traversal afterwards (k_traverse, the cross
    pass writing at pairs + 2 * local), two more host synchronisations, pass timings -1; variants 1 and 3 take the fast path (the
    received queries go through k_descend<EXTERNAL> for both).  A rank's variant is its own business: the mixed world agrees."""
    mixed, all0 = _case("variants")
    for st in mixed["steps"]:
        assert _general(st, 0, 2) and _fast(st, 1) and _fast(st, 2) and min(st["cross"]) > 0, st
    for st in all0["steps"]:
        assert all(_general(st, r, 2) for r in range(3)) and min(st["cross"]) > 0, st


def test_tiny():
    """Ranks of 1, 2, 65 and 1600 triangles; the single triangle has the smallest ID and cuts through every other rank.  Expected:
    k_vertex_box on 3 vertices, a pack launch of one partly filled wave, and on rank 0 a tree WITHOUT records receiving every query
    whose box meets its triangle's.  k_descend and k_traverse start at `root`, which a one-leaf tree does not have: both test leaf 0
    against such queries instead (cd_traverse.h) -- rank 0 owns no pair, so only pairs_tested tells, which the common checks hold to
    the single tree's.  That sum also needs the lone triangle meeting itself, which a leaf of the single tree does and a one-leaf
    tree's local pass cannot: cd_multi_step counts it.  The second run has CD_OPT_TRAVERSAL 0 on every rank: the same through k_traverse,
    both passes by run_traversal."""
    w = mu.want("tiny", 0, 0)
    default, plain = _case("tiny")
    for run in (default, plain):
        for st in run["steps"]:
            assert st["sent"][0] == 3 and st["recv"][0] == w.recv[0] > 100 and st["cross"][0] == 0 and min(st["cross"][1:]) >= 1 and st["n_peers"] == [3, 1, 1, 1], st
            assert all(_fast(st, r) if run is default else _general(st, r, 2) for r in range(4)), st


def test_deep():
    """The 60-level comb.  cross-only: 64 spanning queries arrive at the rank that holds the comb -- expected: its local pass is
    fast, the pass over the received queries defers (59 subtrees pending against WQ_STACK = 12, no idle lane to share with), so
    need_general_x alone: ONE run_traversal (cross), pairs written behind the local ones.  local-only: the comb's own half traversal
    defers (HALF_STACK = 8) -- need_general_l, which forces the cross pass onto run_traversal too: TWO.  The stacks do not grow, so every
    step defers again; cd_stats.stack_overflows is the step's: cd_multi.h sums both passes'."""
    cross_only, local_only = _case("deep")
    for st in cross_only["steps"]:
        assert _general(st, 0, 1) and st["stack_overflows"][0] > 0 and st["cross"][0] >= 40, st
        # (rank 1's 64 spanning centroids lie outside its frame: its sort is redone in step 0, one more synchronisation there)
        assert st["ms"][1]["ms_local"] > 0 and st["host_syncs"][1] <= st["attempts"][1] + 2 and st["stack_overflows"][1] == 0, st
    for st in local_only["steps"]:
        assert _general(st, 0, 2) and st["stack_overflows"][0] > 0 and st["recv"][0] == 4, st
        assert _fast(st, 1) and st["stack_overflows"][1] == 0 and st["cross"][1] >= 1, st


def test_dense():
    """128 triangles as large as the cube on rank 0 (the smaller IDs), 8192 small ones on rank 1.  test_multi_inputs.py shows that on
    rank 1 the two waves of received queries each keep more candidates than a shard of tb[1] holds, and that no stack fills and no
    other shard overflows on either rank.  Expected in step 0 on rank 1: the local pass counts as it is; shards_overflowed(t1, h1)
    alone sets need_general_x: ONE run_traversal, which grows tb[1]'s candidate buffer (grow_candidates: max shard + a quarter),
    repeats the pass and writes the cross pairs behind the local ones -- one more host synchronisation, pass timings -1, and
    cd_stats.stack_overflows == 0 says that no deferred item had a part in it.  tb[1] KEEPS the grown buffer (multi_alloc allocates
    only where there is none, nothing frees or shrinks it between steps), so steps 1 and 2 take the fast path on rank 1 too.  Rank 0 is
    fast throughout: its 8192 received queries keep no candidate, their IDs being the larger."""
    steps = _case("dense")[0]["steps"]
    for it, st in enumerate(steps):
        assert st["stack_overflows"] == [0, 0] and st["attempts"] == [1, 1] and st["cross"][0] == 0 and st["cross"][1] > 0, (it, st)
        assert _fast(st, 0), (it, st)
    assert _general(steps[0], 1, 1) and steps[0]["host_syncs"][1] == 3, steps[0]
    assert _fast(steps[1], 1) and _fast(steps[2], 1), steps[1:]


def test_sort_redo():
    """The redo loop of the step.  equal-keys: one run of 2800 equal keys -- expected: the sort's flag word comes back with the local
    pass's report, judge_sort_flags escalates (more than FIX_MAX keys share their high half: the full form, 3), the rank enqueues sort,
    tree and local pass again and zeroes and repeats the cross pass, all after the collectives: `attempts` stays 1 on both ranks, the
    form afterwards is 3 and stays.
    frame-exit: rank 1's upper centroids leave its CUSTOM frame before step 1 -- SORTF_ABOVE alone: form 0 -> 1 with one redo (one more
    host synchronisation in that step only), kept while outside, and kept in step 3 too: the first form gets its next try only after
    SORT_RETRY_STEPS steps."""
    equal, leave = _case("sort-redo")
    for st in equal["steps"]:
        assert st["attempts"] == [1, 1] and st["sort_form"] == [3, 0] and st["local"][0] == mu.EQUAL_N * (mu.EQUAL_N - 1) // 2 and st["cross"][1] > 0, st
    assert equal["steps"][0]["host_syncs"][0] > equal["steps"][1]["host_syncs"][0]            # the redos are step 0's alone
    assert [st["sort_form"] for st in leave["steps"]] == [[0, 0], [0, 1], [0, 1], [0, 1]]
    assert [st["attempts"] for st in leave["steps"]] == [[1, 1]] * 4
    assert [st["host_syncs"] for st in leave["steps"]] == [[2, 2], [2, 3], [2, 2], [2, 2]]


def test_caps():
    """Rank 1 steps with cap 0 and NULL, 0, 1, local - 1, local, local + 1, local + cross - 1, local + cross, LARGE.  Expected from the
    `room` / `from_spec` arithmetic: CD_OVERFLOW exactly while cap < local + cross, n always the true count, the local pairs first and
    whole once they fit, cross pairs only in the room behind them, nothing behind cap, nothing at all through NULL; rank 0 returns
    CD_OK with its whole list in every one of these rounds (an overflow is not a failure to publish).
    past-spec: both lists of rank 1 are longer than SPEC_PAIRS and the caps (multi_inputs.past_spec_caps) lie on either side of it in
    each list.  Expected: a list's first SPEC_PAIRS rows come with its report, the rest in one hipMemcpy of `ncopy - spec0` rows
    (local) or `ncopy - from_spec` rows from t1.d_pairs + 2 from_spec to pairs + 2 (n_local + from_spec) (cross), one host
    synchronisation each -- and no such copy with a cap at or below SPEC_PAIRS (local) or local + SPEC_PAIRS (cross).  Every step of
    both runs stays on the fast path (the pass timings are there), so these copies are the step's own."""
    small, past = _case("caps")
    k = mu.CAPS_RANK
    for r, (run, res) in enumerate(zip(mu.case("caps").runs, (small, past))):
        w = mu.want("caps", r, 0)
        n = [int(w.local[a].size + w.cross[a].size) for a in range(2)]
        for st, got in zip(run.steps, res["steps"]):
            cap = run.cap if st.caps[k] is None else st.caps[k]
            assert got["cap"][k] == cap and got["n"] == n and got["rc"][1 - k] == 0 and got["rc"][k] == (OVERFLOW if cap < n[k] else 0), (run.name, cap, got)
            assert got["ms"][0]["ms_local"] > 0 and got["ms"][1]["ms_local"] > 0 and got["ms"][k]["ms_cross"] >= 0, (run.name, cap, got)
    assert all(_fast(st, 0) and _fast(st, 1) for st in small["steps"])
    S, L = mu.spec_pairs(), int(mu.want("caps", 1, 0).local[k].size)
    for st in past["steps"]:                        # host synchronisations of the capped rank: the two of every step, and one a separate copy
        cap = st["cap"][k]
        assert st["host_syncs"][k] == st["attempts"][k] + 1 + (cap > S) + (cap > L + S), st
        assert st["host_syncs"][1 - k] == st["attempts"][1 - k] + 2, st                 # (rank 0: its local list is longer than SPEC_PAIRS, it has no cross pair)


def test_flags():
    """CD_MULTI_CROSS_SERIAL on one rank, on all, off; CD_MULTI_TIMING off and on; a second stream of the highest priority.  Expected:
    serial moves the cross pass to the first stream behind the local one (its counters zeroed there, after ev_payload instead of
    ev_tree) -- the same lists, counts and two host synchronisations under every setting; the ms_* fields are measured with
    CD_MULTI_TIMING and left unset (0) without it, rank by rank."""
    case = mu.case("flags")
    for k, run in enumerate(_case("flags")):
        flags = [case.runs[k].create_flags & ~mu.PRIO] * 3
        for it, st in enumerate(run["steps"]):
            f = case.runs[k].steps[it].flags
            flags = [flags[r] if f is None or f[r] is None else f[r] for r in range(3)]
            assert st["host_syncs"] == [2, 2, 2] and st["attempts"] == [1, 1, 1], (run["run"], it)
            for r in range(3):
                ms = st["ms"][r]
                if flags[r] & mu.T:
                    assert ms["ms_tree"] > 0 and ms["ms_local"] > 0 and ms["ms_pack"] >= 0 and min(ms.values()) >= 0, (run["run"], it, r, ms)
                else:
                    assert all(v in (0.0, -1.0) for v in ms.values()), (run["run"], it, r, ms)


def test_moving():
    """Rank 1 slides: overlapping, touching rank 0 exactly (x-min == x-max, fp32 values), apart, overlapping again.  Expected: the root
    boxes' test is strict, so touching is no peer -- no record packed, no send or receive posted, the cross pass skipped (recvd == 0)
    with its counters zeroed by k_vertex_box all the same -- and the step after two such steps exchanges and reports as the first did."""
    steps = _case("moving")[0]["steps"]
    assert [st["n_peers"] for st in steps] == [[1, 1], [0, 0], [0, 0], [1, 1]]
    assert [st["cross"][1] > 0 for st in steps] == [True, False, False, True] and [st["sent"] for st in steps[1:3]] == [[0, 0]] * 2
    assert all(_fast(st, 0) and _fast(st, 1) for st in steps)


def test_queries_after():
    """The multi step as a rebuild entry: one rank, real RCCL, CD_MULTI_SELF_PEER; per frame of the jitter sequence
    cd_update_vertices, the step, then cd_root_box, cd_find_proximity, cd_closest_points, cd_cast_rays, cd_points_within and
    cd_sorted_pairs, each against the CPU restatement of that frame and a fresh context; so are cd_boxes_overlap_all, cd_planes_cut_all,
    cd_segments_within, cd_sweep_segments_all, cd_boxes_count and cd_planes_count on moving_inputs' items of the frame.  Expected: the step leaves the tree of the
    CURRENT vertices (records, leaves, root box cached from the all-gathered boxes) exactly as cd_build_tree would; its pair list is
    two lists, so cd_sorted_pairs answers CD_OVERFLOW without writing while the step found pairs, and n = 0 with CD_OK when it found none."""
    name = mu.QA_NAME
    s = mi.seq(name)
    cap = 1 << 20
    with mi355cd.CollisionDetector(s.frames[0], s.vidx) as cd:
        if s.frame_mode != "reference":
            cd.set_morton_frame(mi355cd.CD_FRAME_AUTO)
        with mi355cd.MultiStep(cd, mi355cd.multi_unique_id(), 0, 1, flags=mi355cd.CD_MULTI_SELF_PEER) as ms:
            for f in range(mu.QA_FRAMES):
                v, what = s.frames[f], f"{name} frame {f} after cd_multi_step"
                cd.update_vertices(v)
                pairs, n, rc, info = ms.step(cap=cap)
                st = mi.want_step(name, f)
                nl = int(st["stats"].n_pairs)
                assert rc == 0 and n == 2 * nl and info.local_pairs == nl and info.cross_pairs == nl and nl > 0, (what, rc, n, nl)
                mi.same_pair_set(pairs[:nl], st["pairs"], what + " local"); mi.same_pair_set(pairs[nl:], st["pairs"], what + " cross")
                assert info.pairs_tested == 2 * st["stats"].pairs_tested, what
                with mi355cd.CollisionDetector(v, s.vidx) as fresh:
                    if s.frame_mode != "reference":
                        fresh.set_morton_frame(mi355cd.CD_FRAME_AUTO)
                    fresh.build_tree()
                    rays, pts, rm, d = mi.rays(name, f), mi.points(name, f), mi.radii(name, f), mi.prox_dist(name, f)
                    got = cd.root_box()
                    mi.same_root_box(got, mi.want_root_box(name, f), what); mi.same_root_box(got, fresh.root_box(), what + " (fresh)")
                    got = cd.find_proximity(d, cap=cap)
                    mi.same_prox(got, mi.want_prox(name, f), what + " proximity")
                    gf = fresh.find_proximity(d, cap=cap)
                    mi.same_prox(got, pr.sort_pairs(gf[0], gf[1]), what + " proximity (fresh)")
                    assert cd.proximity_tested == fresh.proximity_tested, what
                    got = cd.closest_points(pts, rm)
                    mi.same_points(got, mi.want_points_r(name, f), what + " points")
                    mi.same_points(got[:7], fresh.closest_points(pts, rm)[:7], what + " points (fresh)")
                    got = cd.cast_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6])
                    mi.same_rays(got, mi.want_rays(name, f), what + " rays")
                    mi.same_rays(got[:5], fresh.cast_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6])[:5], what + " rays (fresh)")
                    got = cd.points_within(pts, rm, cap=cap)
                    assert got[8] == 0 and got[7] == got[0].shape[0], what
                    rows = wr.PointRows(*wr.sort_rows(*got[:7]))
                    wr.same_rows(rows, mu.want_within(f), what + " points within")
                    gf = fresh.points_within(pts, rm, cap=cap)
                    wr.same_rows(rows, wr.PointRows(*wr.sort_rows(*gf[:7])), what + " points within (fresh)")
                    # the box, plane, segment and swept-segment rows and the two count calls, on moving_inputs' items of the frame
                    room = lambda w: max(1, 2 * w.rows.shape[0])
                    b, p, sg, sw = mi.box_items(name, f), mi.plane_items(name, f), mi.segment_items(name, f), mi.swept_segment_items(name, f)
                    want = mi.want_boxes(name, f)
                    got = cd.boxes_overlap_all(b[:, 0::2], b[:, 1::2], cap=room(want))
                    mi.same_item_rows(got, want, what + " boxes")
                    mi.same_item_rows(got, mi.item_rows(fresh.boxes_overlap_all(b[:, 0::2], b[:, 1::2], cap=room(want))), what + " boxes (fresh)")
                    assert cd.boxes_tested == fresh.boxes_tested, what
                    got = cd.boxes_count(b[:, 0::2], b[:, 1::2])
                    mi.same_box_counts(got, want, b.shape[0], what + " boxes count")
                    assert all(np.array_equal(x, y) for x, y in zip(got[:2], fresh.boxes_count(b[:, 0::2], b[:, 1::2])[:2])), what + " boxes count (fresh)"
                    want = mi.want_planes(name, f)
                    got = cd.planes_cut_all(p[:, :3], p[:, 3], cap=room(want))
                    mi.same_item_rows(got, want, what + " planes")
                    mi.same_item_rows(got, mi.item_rows(fresh.planes_cut_all(p[:, :3], p[:, 3], cap=room(want))), what + " planes (fresh)")
                    assert cd.planes_tested == fresh.planes_tested, what
                    got = cd.planes_count(p[:, :3], p[:, 3])
                    mi.same_plane_counts(got, mi.want_plane_classes(name, f), what + " planes count")
                    assert all(np.array_equal(x, y) for x, y in zip(got[:3], fresh.planes_count(p[:, :3], p[:, 3])[:3])), what + " planes count (fresh)"
                    want = mi.want_segments(name, f)
                    got = cd.segments_within(sg[:, 0:3], sg[:, 3:6], sg[:, 6], cap=room(want))
                    mi.same_item_rows(got, want, what + " segments")
                    mi.same_item_rows(got, mi.item_rows(fresh.segments_within(sg[:, 0:3], sg[:, 3:6], sg[:, 6], cap=room(want))), what + " segments (fresh)")
                    assert cd.segments_tested == fresh.segments_tested, what
                    want, counts = mi.want_swept_segments(name, f)
                    ends = (sw[:, 0:3], sw[:, 3:6], sw[:, 6:9], sw[:, 9:12], sw[:, 12])
                    got = cd.sweep_segments_all(*ends, verts_end=mi.x1(name, f), cap=room(want))
                    info = cd.sweep_segments_info
                    mi.same_item_rows(got, want, what + " swept segments")
                    assert (info.n_tested, info.n_evals, info.n_unresolved) == counts, (what, counts)
                    mi.same_item_rows(got, mi.item_rows(fresh.sweep_segments_all(*ends, verts_end=mi.x1(name, f), cap=room(want))), what + " swept segments (fresh)")
                    assert bytes(info) == bytes(fresh.sweep_segments_info), what
                    sentinel = np.full((4, 2), 0xDEADBEEF, dtype=np.uint32)
                    nn = mi355cd.C.c_uint64(12345)
                    assert cd.lib.cd_sorted_pairs(cd._ctx, sentinel.ctypes.data, 4, mi355cd.C.byref(nn)) == OVERFLOW, what
                    assert nn.value == 12345 and (sentinel == 0xDEADBEEF).all(), what          # neither the buffer nor the count is written
    # a step that finds no pair: two triangles far apart
    verts = np.array([[0.1, 0, 0], [0.2, 0, 0], [0.1, 0.1, 0.1], [2.1, 0, 1], [2.2, 0, 1], [2.1, 0.1, 1.1]], dtype=np.float64)
    vidx = np.arange(6, dtype=np.uint32).reshape(2, 3)
    assert oracle.pipeline(verts, vidx)["stats"].n_pairs == 0
    with mi355cd.CollisionDetector(verts, vidx) as cd:
        with mi355cd.MultiStep(cd, mi355cd.multi_unique_id(), 0, 1, flags=mi355cd.CD_MULTI_SELF_PEER) as ms:
            pairs, n, rc, info = ms.step(cap=16)
            assert rc == 0 and n == 0 and info.recv_queries == 2
            p2, n2, rc2 = cd.sorted_pairs(cap=16)
            assert rc2 == 0 and n2 == 0 and p2.shape[0] == 0
