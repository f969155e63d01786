"""cd_sorted_pairs / cd_collision_triangles beyond one sort tile: the device pair-list sort (pp_sort: k_os_hist + eight k_os_pass, every
one with the ticket and the decoupled look-back), the 32 -> 64-bit key packers, k_unique_flags / k_scan_exclusive / k_unique_scatter and
the buffers pp_reserve grows, on the meshes of tests/post_inputs.py whose pair list is known by construction.

Every comparison is exact byte equality, with (a) np.lexsort / np.unique of the by-construction list mapped through the ID map and (b)
the same of the unordered pairs the step itself returned; every call must return CD_OK (CD_ERR_SORT raises in the bindings) and the
expected count.  tests/test_post_inputs.py shows without a GPU that the comparisons fail on wrong results."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import mi355cd
import oracle
import post_inputs as pi

pytestmark = pytest.mark.gpu

CAP = 1 << 15                  # pairs, for everything but the large cases
CANARY = 0xA5A5A5A5
TILE = 4096                    # keys per sort tile (csrc/cd_sort.h SORT_TILE)


@functools.lru_cache(maxsize=4)
def _crosses(m, fans=()):
    return pi.crosses(m, fans)


def _ctx(mesh, ids, frame=mi355cd.CD_FRAME_CUSTOM):
    cd = mi355cd.CollisionDetector(mesh.verts, mesh.vidx, ids)
    if frame == mi355cd.CD_FRAME_CUSTOM:
        cd.set_morton_frame(frame, pi.FRAME_OFF, pi.FRAME_SPAN)
    else:
        cd.set_morton_frame(frame)
    return cd


def _post(cd, want, step_pairs, what, cap=CAP, order=("pairs", "ids")):
    """Both post-processing calls against both references.  -> (sorted pairs, ID set) as returned."""
    out = {}
    for call in order:
        if call == "pairs":
            res = out["pairs"] = cd.sorted_pairs(cap)
            pi.same_sorted_pairs(res, want, f"{what}: cd_sorted_pairs against the constructed list")
            pi.same_sorted_pairs(res, step_pairs, f"{what}: cd_sorted_pairs against the step's own list")
        else:
            res = out["ids"] = cd.collision_triangles(2 * cap)
            pi.same_id_set(res, want, f"{what}: cd_collision_triangles against the constructed list")
            pi.same_id_set(res, step_pairs, f"{what}: cd_collision_triangles against the step's own list")
    return out["pairs"][0], out["ids"][0]


def _step_and_post(cd, want, what, cap=CAP, order=("pairs", "ids")):
    step = cd.self_collide(cap)
    pi.same_step(step, want, f"{what}: the step")
    return _post(cd, want, step[0], what, cap, order)


# ---- sizes x ID maps
SIZES = [1, 2, 127, 128, 129, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8193]


@pytest.mark.parametrize("id_map", list(pi.ID_MAPS))
@pytest.mark.parametrize("m", SIZES)
def test_every_size_with_every_id_map(m, id_map):
    """m pairs on 2 m triangles: 2 m goes through 1024 (the scan's chunk 1 -> 2) and through one tile, m through one and two tiles."""
    mesh = _crosses(m)
    ids = pi.ids_for(id_map, mesh.nt)
    with _ctx(mesh, ids) as cd:
        sp, tri = _step_and_post(cd, pi.ordered(mesh.pairs, ids), f"crosses({m}) {id_map}")
    assert sp.shape == (m, 2) and tri.shape == (2 * m,)


@pytest.fixture(scope="module")
def large():
    return pi.crosses(300000, (70000,))


@pytest.mark.parametrize("id_map", pi.LARGE_MAPS)
def test_seventeen_pair_tiles(id_map):
    mesh = _crosses(65537)
    ids = pi.ids_for(id_map, mesh.nt)
    with _ctx(mesh, ids) as cd:
        _step_and_post(cd, pi.ordered(mesh.pairs, ids), f"crosses(65537) {id_map}", cap=1 << 17)


@pytest.mark.parametrize("id_map", pi.LARGE_MAPS)
def test_large_case_91_pair_tiles_181_id_tiles(large, id_map):
    """370 000 pairs on 670 001 triangles, 70 000 of them in one fan."""
    assert large.nt == 670001 and large.pairs.shape[0] == 370000
    assert -(-370000 // TILE) == 91 and -(-740000 // TILE) == 181
    ids = pi.ids_for(id_map, large.nt)
    with _ctx(large, ids) as cd:
        _step_and_post(cd, pi.ordered(large.pairs, ids), f"large {id_map}", cap=1 << 19)


@pytest.mark.parametrize("where", ["smallest", "largest", "middle"])
def test_large_case_run_of_70000_equal_ids(large, where):
    """The hub of the 70 000 fan as the smallest / largest / a middle ID of its fan: a run of 70 000 equal IDs (17 tiles) in the
    flattened list, 70 000 keys that share their high (low) word in the pair sort."""
    ids = pi.place_hubs(pi.ids_for("bitrev", large.nt), large, where)
    hub = ids[large.fans[0][0]]
    with _ctx(large, ids) as cd:
        sp, tri = _step_and_post(cd, pi.ordered(large.pairs, ids), f"large, hub {where}", cap=1 << 19)
    _hub_rows(sp, tri, hub, 70000, where)


def _hub_rows(sp, tri, hub, j, where):
    """The hub once in the set; all j of its rows in the sorted list, in order of the other column."""
    assert int((tri == hub).sum()) == 1
    rows = sp[(sp[:, 0] == hub) | (sp[:, 1] == hub)]
    assert rows.shape[0] == j
    other = np.where(rows[:, 0] == hub, rows[:, 1], rows[:, 0]).astype(np.int64)
    if where in ("smallest", "largest"):
        assert np.all(rows[:, 0 if where == "smallest" else 1] == hub) and np.all(np.diff(other) > 0)
    else:                                                            # hub second for the smaller blades, first for the larger: two ascending stretches
        k = int((rows[:, 1] == hub).sum())
        assert k == j // 2 and np.all(np.diff(other[rows[:, 1] == hub]) > 0) and np.all(np.diff(other[rows[:, 0] == hub]) > 0)


# ---- runs of equal IDs across tile and scan-chunk boundaries
FANS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097]
PREFIXES = [0, 1, 2047, 2048, 4095]


@pytest.mark.parametrize("j", FANS)
def test_runs_of_equal_ids_across_boundaries(j):
    """A fan of j blades behind P plain crosses with identity IDs: in the sorted flattened list the hub's run of j equal IDs starts at
    2 P (hub smallest: at, just before, just after a tile boundary for P = 2048, 2047 / 4095, 1), ends there (hub largest), or lies
    in between; the scan's chunk is ceil(2 (P + j) / 1024) entries, so the run's ends move over chunk boundaries with P and j too."""
    for P in PREFIXES:
        mesh = _crosses(P, (j,))
        assert mesh.pairs.shape[0] == P + j and mesh.nt == 2 * P + j + 1
        for where in ("smallest", "largest", "middle"):
            ids = pi.place_hubs(pi.ids_for("identity", mesh.nt), mesh, where)
            hub = ids[mesh.fans[0][0]]
            want = pi.ordered(mesh.pairs, ids)
            flat = np.sort(want.reshape(-1))
            run = np.flatnonzero(flat == hub)
            assert run.shape[0] == j and run[0] == 2 * P + {"smallest": 0, "largest": j, "middle": j // 2}[where]
            with _ctx(mesh, ids) as cd:
                sp, tri = _step_and_post(cd, want, f"crosses({P}, ({j},)) hub {where}")
            assert tri.shape[0] == 2 * P + j + 1
            _hub_rows(sp, tri, hub, j, where)


# ---- where the list comes from
def _comb(codes):
    """The comb of test_readers_of_the_query_boxes_get_them_on_request (tests/test_cd_gpu.py): two tiny triangles per Morton code in a
    frame whose cells are unit cubes, and one triangle over everything that sorts first -- its query overflows a lane's stack."""
    tris = []
    for code in codes:
        c = np.zeros(3)
        for p in range(60):
            if (code >> p) & 1:
                c[{2: 0, 1: 1, 0: 2}[p % 3]] += float(1 << (p // 3))
        c += 0.5
        for s in (0.0, 0.02):
            tris.append([c + [s, 0, 0], c + [s + 0.2, 0.1, 0], c + [s, 0.1, 0.2]])
    tris.append([[-9.0e6] * 3, [4.0e6, -1.0, -1.0], [-1.0, 4.0e6, 4.0e6]])
    verts = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    return verts, np.arange(verts.shape[0], dtype=np.uint32).reshape(-1, 3)


def _stats_bytes(cd):
    return bytes(cd.stats())


def _both_orders_twice(cd, want, step_pairs, what):
    """Both calls in both orders, twice each: the same bytes every time, and cd_get_stats as the step left it."""
    st0 = _stats_bytes(cd)
    first = None
    for order in (("pairs", "ids"), ("ids", "pairs")):
        for rep in range(2):
            got = _post(cd, want, step_pairs, f"{what} {order} #{rep}", order=order)
            if first is None:
                first = got
            assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()
            assert _stats_bytes(cd) == st0, f"{what}: the post-processing changed cd_get_stats"


def _source(cd, name, hp):
    """One way of making the pair list.  -> (pairs, n, rc)"""
    if name == "stream":
        return cd.self_collide(CAP)
    if name == "graph":
        cd.self_collide(CAP)                                           # (the first step of a context is the stream's)
        # The hub of the 5 000 fan hands more work on than a replay can answer: such a step replays the graph (tree and descent), then
        # finishes its traversal on the stream and leaves scratch a capture cannot start from -- the step after it is the stream's,
        # the one after that a replay again.  Whichever of the next two steps replays is the one taken.
        rep0 = cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
        got = cd.self_collide(CAP)
        if cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0:
            got = cd.self_collide(CAP)
        assert cd.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + 1, "no step is a replay: nothing of the graph path would be tested"
        return got
    if name.startswith("variant"):
        cd.set_option(mi355cd.CD_OPT_TRAVERSAL, int(name[-1]))
        cd.build_tree()
        return cd.find_collisions(CAP)
    if name.startswith("brute"):
        if not getattr(cd, "_tree_built", False):
            # cd_brute_force needs no tree, the two calls do (include/mi355cd.h): without one they refuse and write nothing
            pairs, n, rc = cd.brute_force(box_filter=name.endswith("box"), cap=CAP)
            assert rc == mi355cd.CD_OK and n == 6308
            for which in ("pairs", "ids"):
                buf, n, rc = _raw(cd, which, 16, 16)
                assert rc == mi355cd.CD_ERR_ORDER and np.all(buf == CANARY)
            cd.build_tree()
            cd._tree_built = True
        return cd.brute_force(box_filter=name.endswith("box"), cap=CAP)
    assert name == "host_pairs"
    for _ in range(3):                                                 # (the first two steps into a pinned buffer synchronise the stream; the third is the steady state)
        hp.array[:] = 0xFFFFFFFF
        n, rc = cd.self_collide_into(hp.array)
    assert (hp.array[n:n + 8] == 0xFFFFFFFF).all()
    return hp.array[:min(n, CAP)].copy(), n, rc


SOURCES = ["stream", "graph", "variant0", "variant1", "variant3", "brute_box", "brute_nobox", "host_pairs"]


@pytest.mark.parametrize("source", SOURCES)
def test_every_source_of_the_list(source):
    """One medium mesh (6 308 pairs, fans of 1, 7, 300 and 5 000) through every call that leaves a pair list.  (In the frame the mesh
    computes for itself: in the unit-cube frame more than 16 blades of the large fan share a key's high half, the sort goes to its
    eight-pass form for good, and such a context captures no graph.)"""
    mesh = _crosses(1000, (1, 7, 300, 5000))
    ids = pi.place_hubs(pi.ids_for("bitrev", mesh.nt), mesh, "middle")
    want = pi.ordered(mesh.pairs, ids)
    assert want.shape[0] == 6308
    with _ctx(mesh, ids, mi355cd.CD_FRAME_AUTO) as cd, mi355cd.HostPairs(CAP) as hp:
        if source in ("graph", "host_pairs"):
            cd.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0); cd.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
        cd.set_option(mi355cd.CD_OPT_GRAPH, 1 if source == "graph" else 0)
        step = _source(cd, source, hp)
        pi.same_step(step, want, source)
        tested = cd.stats().pairs_tested
        _both_orders_twice(cd, want, step[0], source)
        again = _source(cd, source, hp)                                # the next step is what it was
        pi.same_step(again, want, f"{source}, the step after the post-processing")
        assert cd.stats().pairs_tested == tested
        _post(cd, want, again[0], f"{source}, after the next step")


def test_list_partly_from_the_deep_pass():
    off = np.zeros(3); span = np.full(3, 1048576.0)
    verts, vidx = _comb([1 << (59 - k) for k in range(60)])
    ids = pi.ids_for("bitrev", vidx.shape[0])
    r = oracle.pipeline(verts, vidx, ids, off=off, span=span)
    want = np.ascontiguousarray(r["pairs"], dtype=np.uint32)
    assert want.shape[0] == r["stats"].n_pairs >= 40
    with mi355cd.CollisionDetector(verts, vidx, ids) as cd:
        cd.set_morton_frame(mi355cd.CD_FRAME_CUSTOM, off, span)
        step = cd.self_collide(CAP)
        assert cd.stats().stack_overflows > 0
        pi.same_step(step, want, "comb")
        tested = cd.stats().pairs_tested
        assert tested == r["stats"].pairs_tested
        _both_orders_twice(cd, want, step[0], "comb")
        again = cd.self_collide(CAP)
        pi.same_step(again, want, "comb, the step after")
        assert cd.stats().pairs_tested == tested and cd.stats().stack_overflows > 0


# ---- one long-lived context, changing counts
def _raw(cd, which, cap, rows, null=False):
    """The C call itself into a canary-filled buffer of `rows` entries.  -> (buffer, n, rc)"""
    buf = np.full((rows, 2) if which == "pairs" else (rows,), CANARY, dtype=np.uint32)
    n = C.c_uint64(0xDEADBEEF)
    fn = cd.lib.cd_sorted_pairs if which == "pairs" else cd.lib.cd_collision_triangles
    rc = fn(cd._ctx, None if null else buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    return buf, n.value, rc


COUNTS = [5, 70000, 3, 0, 4097, 70000, 1]


@functools.lru_cache(maxsize=1)
def _frames():
    K, J = 4097, 70000
    meshes = []
    for f, cnt in enumerate(COUNTS):
        live = np.zeros(K + J, dtype=bool)
        if cnt == 70000 and f == 1:
            live[K:] = True                                             # the fan alone: 70 000 rows with the hub
        elif cnt == 70000:
            live[:K] = True; live[K + 11:K + 11 + (J - K)] = True       # all crosses and most of the fan
        elif cnt == 4097:
            live[:K] = True
        else:
            live[np.random.Generator(np.random.PCG64(f)).permutation(K + J)[:cnt]] = True
        assert int(live.sum()) == cnt
        meshes.append(pi.crosses(K, (J,), live=live))
    return meshes


@pytest.mark.parametrize("order", [("pairs", "ids"), ("ids", "pairs")])
def test_one_context_changing_counts(order):
    """4 097 crosses and a fan of 70 000 in ONE context; `live` masks take the pair count through 5 -> 70 000 -> 3 -> 0 -> 4 097 ->
    70 000 -> 1: a stale tail of the larger sort before, the buffers' regrowth (by the ID call, which needs 2 m, after the pair call
    sized them for m, and the other way round), the look-back area zeroed for this sort's tile count."""
    meshes = _frames()
    ids = pi.place_hubs(pi.ids_for("bitrev", meshes[0].nt), meshes[0], "middle")
    with _ctx(meshes[0], ids) as cd:
        for f, mesh in enumerate(meshes):
            if f:
                cd.update_vertices(mesh.verts)
            want = pi.ordered(mesh.pairs, ids)
            step = cd.self_collide(1 << 17)
            pi.same_step(step, want, f"frame {f}")
            if COUNTS[f] == 0:
                for which in order + order:
                    buf, n, rc = _raw(cd, which, 16, 16)
                    assert (rc, n) == (mi355cd.CD_OK, 0) and np.all(buf == CANARY), (f, which)
            _post(cd, want, step[0], f"frame {f} ({COUNTS[f]} pairs)", cap=1 << 17, order=order)


# ---- capacity edges
def test_capacity_edges():
    """cap in {0 with NULL, 1, n - 1, n, n + 1} at n = 4 097 pairs / 8 194 IDs: CD_OVERFLOW below n, *n the full count, the first cap
    entries the prefix of the sorted result, the entries behind cap untouched; after a truncated step both calls refuse."""
    mesh = _crosses(4097)
    ids = pi.ids_for("bitrev", mesh.nt)
    rows = pi.ordered(mesh.pairs, ids)
    want = {"pairs": pi.sort_rows(rows), "ids": pi.id_set(rows)}
    with _ctx(mesh, ids) as cd:
        pi.same_step(cd.self_collide(CAP), rows, "step")
        for which, n_want in (("pairs", 4097), ("ids", 8194)):
            assert want[which].shape[0] == n_want
            for cap in (0, 1, n_want - 1, n_want, n_want + 1):
                buf, n, rc = _raw(cd, which, cap, n_want + 3, null=cap == 0)
                assert n == n_want, (which, cap, n)
                assert rc == (mi355cd.CD_OVERFLOW if cap < n_want else mi355cd.CD_OK), (which, cap, rc)
                k = min(cap, n_want)
                assert buf[:k].tobytes() == want[which][:k].tobytes(), (which, cap)
                assert np.all(buf[k:] == CANARY), (which, cap)
        # a truncated step: cap_pairs < its n_pairs
        pairs, n, rc = cd.find_collisions(cap=10)
        assert rc == mi355cd.CD_OVERFLOW and n == 4097
        assert cd.sorted_pairs()[2] == mi355cd.CD_OVERFLOW
        for which in ("pairs", "ids", "ids", "pairs"):
            buf, n, rc = _raw(cd, which, 8200, 8200)
            assert rc == mi355cd.CD_OVERFLOW and np.all(buf == CANARY), which
        # ... and a full one after it serves again
        pi.same_step(cd.find_collisions(CAP), rows, "full step after the truncated one")
        _post(cd, rows, rows, "after the truncated step")


# ---- after calls that own no single list (the contract: include/mi355cd.h at cd_sorted_pairs)
def test_previous_list_survives_an_update_and_a_rebuild():
    """cd_update_vertices + cd_build_tree run no traversal: the list of the LAST traversal comes back intact (between the two calls
    there is no tree: CD_ERR_ORDER, nothing written)."""
    K = 5000
    moved = pi.crosses(K, (600,), live=np.arange(K + 600) % 3 == 0)
    mesh = pi.crosses(K, (600,))
    ids = pi.place_hubs(pi.ids_for("random", mesh.nt), mesh, "smallest")
    want = pi.ordered(mesh.pairs, ids)
    with _ctx(mesh, ids) as cd:
        first = _step_and_post(cd, want, "before the update")
        st0 = (cd.stats().n_pairs, cd.stats().pairs_tested)
        cd.update_vertices(moved.verts)
        for which in ("pairs", "ids"):
            buf, n, rc = _raw(cd, which, 16, 16)
            assert rc == mi355cd.CD_ERR_ORDER and np.all(buf == CANARY)
        cd.build_tree()
        for order in (("ids", "pairs"), ("pairs", "ids")):
            got = _post(cd, want, want, "after cd_update_vertices + cd_build_tree", order=order)
            assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()
        assert (cd.stats().n_pairs, cd.stats().pairs_tested) == st0
        want2 = pi.ordered(moved.pairs, ids)                            # the next traversal replaces it
        step = cd.find_collisions(CAP)
        pi.same_step(step, want2, "the moved mesh")
        _post(cd, want2, step[0], "the moved mesh")


def test_after_external_queries_the_list_is_theirs():
    """cd_find_collisions_queries is a traversal like any other: its pairs are the resident list.  (The mesh's own leaves as the
    queries: the ID rule lets every pair through once, so the list is the self-collision's.)"""
    import torch
    import mi355_multi as multi
    mesh = _crosses(1000, (1, 7, 300, 5000))
    ids = pi.place_hubs(pi.ids_for("bitrev", mesh.nt), mesh, "largest")
    want = pi.ordered(mesh.pairs, ids)
    e = multi.HipEngine(mesh.verts, mesh.vidx, ids, torch.device("cuda", 0))
    try:
        cd = e.cd
        few = cd.self_collide(CAP)
        pi.same_step(few, want, "self")
        q = e.pack_queries(np.array([-1.0, 2.0, -1.0, 2.0, -1.0, 2.0]))
        assert q.numel() // multi.QUERY_BYTES == mesh.nt
        half = q[: (mesh.nt // 2) * multi.QUERY_BYTES]                  # the first half of the leaves only: a list of its own
        for qbuf in (half, q):
            torch.cuda.synchronize()
            step = cd.find_collisions_queries(qbuf.data_ptr(), qbuf.numel() // multi.QUERY_BYTES, CAP)
            assert step[2] == mi355cd.CD_OK
            if qbuf is q:
                pi.same_step(step, want, "all leaves as queries")
            else:
                assert 0 < step[1] < want.shape[0]
            rows = np.ascontiguousarray(step[0])
            _both_orders_twice(cd, rows, rows, "after cd_find_collisions_queries")
    finally:
        e.close()


def test_after_a_multi_step_there_is_no_single_list():
    """cd_multi_step leaves two lists (local, cross), neither of them the step's result: both calls return CD_OVERFLOW and write
    nothing when the step found a pair, n = 0 with CD_OK when it found none; the next single-list traversal serves again."""
    mesh = _crosses(4097)
    ids = pi.ids_for("random", mesh.nt)
    want = pi.ordered(mesh.pairs, ids)
    apart = pi.crosses(4097, live=np.zeros(4097, dtype=bool))
    with _ctx(mesh, ids) as cd:
        _step_and_post(cd, want, "before the multi step")
        with mi355cd.MultiStep(cd, mi355cd.multi_unique_id(), 0, 1) as ms:
            pairs, n, rc, info = ms.step(cap=CAP)
            assert rc == 0 and n == 4097 and info.cross_pairs == 0
            pi.same_step((pairs.copy(), n, rc), want, "one-rank multi step")
            for which in ("pairs", "ids", "ids", "pairs"):
                buf, n, rc = _raw(cd, which, 8200, 8200)
                assert rc == mi355cd.CD_OVERFLOW and np.all(buf == CANARY), which
            cd.update_vertices(apart.verts)
            pairs, n, rc, info = ms.step(cap=CAP)
            assert rc == 0 and n == 0
            for which in ("pairs", "ids", "ids", "pairs"):
                buf, n, rc = _raw(cd, which, 8200, 8200)
                assert (rc, n) == (mi355cd.CD_OK, 0) and np.all(buf == CANARY), which
            cd.update_vertices(mesh.verts)
            pairs, n, rc, info = ms.step(cap=CAP)
            assert rc == 0 and n == 4097
        _step_and_post(cd, want, "after the multi step")
