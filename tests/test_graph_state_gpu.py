"""CD_OPT_GRAPH against the stream path across state changes.

A replayed step runs the kernels and arguments its capture baked in.  It is right only if every setter that changes what the step
would enqueue either changes the graph's key, drops the graph, or makes the step ineligible ("The captured step").
Pair sets alone do not show a stale replay: they stay right even when the keys, the sort form or the tree are wrong.

So every test here runs one call sequence on two contexts over the same mesh, G with the graph on and S with it off, and after
every step compares return values, pairs, statistics, keys and permutation, the Morton frame, the sort form and the build with
each other and with the oracle of the current vertices and frame.  G must also really replay (anti-vacuity): under options that
allow a graph step, at least the second step after any change is one graph launch."""
from __future__ import annotations

import numpy as np
import pytest

import mi355_synth as synth
import mi355cd
import oracle
import point_ref as ptr
import ray_ref as rr
import sweep_ref as sr
import within_ref as wr

pytestmark = pytest.mark.gpu

CAP = 1 << 20
REF = ("ref", tuple(synth.REF_OFF), tuple(synth.REF_SPAN), 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Twin:
    """Two contexts on one mesh: g replays captured steps (CD_OPT_GRAPH 1), s runs every step on the stream."""

    def __init__(self, verts, vidx, ids=None):
        self.vidx = np.ascontiguousarray(vidx, dtype=np.uint32)
        self.ids = ids
        self.g = mi355cd.CollisionDetector(verts, vidx, ids)
        self.s = mi355cd.CollisionDetector(verts, vidx, ids)
        for cd, graph in ((self.g, 1), (self.s, 0)):
            cd.set_option(mi355cd.CD_OPT_STAGE_TIMING, 0)
            cd.set_option(mi355cd.CD_OPT_KERNEL_STAMPS, 0)
            cd.set_option(mi355cd.CD_OPT_GRAPH, graph)
        self.verts = np.ascontiguousarray(verts, dtype=np.float64)
        self.vver = 0                                   # bumped with every new vertex array: the oracle cache's key
        self.frame = REF                                # ("ref" | "custom" | "auto", off, span, layout) as set on both contexts
        self.opts = dict(trav=3, timing=0, stamps=0, sort_full=0, stagewise=0, diag=0, lds_pad=0, graph=1)
        self.since_change = 0
        self.log = []
        self._cache = {}
        self._host = {}
        self.replays = 0
        self.last_continued = False

    def close(self):
        for hp in self._host.values():
            hp.close()
        self.g.close(); self.s.close()

    # ---- what the oracle says for the current vertices and frame (computed once per pair)
    def expected_frame(self):
        kind, off, span, lay = self.frame
        if kind == "auto":
            key = ("auto", self.vver)
            if key not in self._cache:
                self._cache[key] = oracle.auto_frame(self.verts, self.vidx)
            return self._cache[key]
        return np.array(off), np.array(span), lay

    def ref(self):
        off, span, lay = self.expected_frame()
        key = (self.vver, tuple(_bits(off)), tuple(_bits(span)), lay)
        if key not in self._cache:
            self._cache[key] = oracle.pipeline(self.verts, self.vidx, self.ids, off=off, span=span, layout=lay)
        return self._cache[key]

    # ---- applying an operation to both contexts
    def both(self, desc, fn, change=True):
        """fn(cd) on g, then on s; returns both results.  Logged, so that a failure prints the sequence that led to it."""
        self.log.append(desc)
        out = fn(self.g), fn(self.s)
        if change:
            self.since_change = 0
        return out

    def set_option(self, key, value, name=None):
        self.both(f"set_option({name or key}, {value})", lambda cd: cd.set_option(key, value))
        self._note(name, value)

    def debug_set(self, key, value, name=None):
        self.both(f"debug_set({name or key}, {value})", lambda cd: cd.debug_set(key, value))
        self._note(name, value)

    def _note(self, name, value):
        field = {"TRAVERSAL": "trav", "STAGE_TIMING": "timing", "KERNEL_STAMPS": "stamps", "SORT_FULL": "sort_full",
                 "STAGEWISE_BUILD": "stagewise", "DIAG": "diag", "LDS_PAD": "lds_pad"}.get(name)
        if field:
            self.opts[field] = value

    def eligible(self):
        """Do the options allow a graph step (graph_eligible)?"""
        o = self.opts
        return (o["graph"] and o["trav"] == 3 and not o["timing"] and o["stamps"] == 0 and o["sort_full"] == 0 and not o["stagewise"]
                and not o["diag"] and o["lds_pad"] == 0)

    def update_vertices(self, verts, desc="update_vertices"):
        v = np.ascontiguousarray(verts, dtype=np.float64)
        self.both(desc, lambda cd: cd.update_vertices(v))
        self.verts = v
        self.vver += 1

    def set_frame(self, mode, off=None, span=None):
        name = {mi355cd.CD_FRAME_REFERENCE: "REFERENCE", mi355cd.CD_FRAME_CUSTOM: "CUSTOM", mi355cd.CD_FRAME_AUTO: "AUTO"}[mode]
        self.both(f"set_morton_frame({name})", lambda cd: cd.set_morton_frame(mode, off, span))
        if mode == mi355cd.CD_FRAME_REFERENCE:
            self.frame = REF
        elif mode == mi355cd.CD_FRAME_CUSTOM:
            self.frame = ("custom", tuple(off), tuple(span), 0)
        else:
            self.frame = ("auto", None, None, None)

    def set_frame_layout(self, off, span, lay):
        self.both(f"set_morton_frame_layout({lay:#x})", lambda cd: cd.set_morton_frame_layout(off, span, lay))
        self.frame = ("custom", tuple(off), tuple(span), lay)

    def keep_auto_frame(self):
        assert self.frame[0] == "auto"
        fg, fs = self.both("keep_auto_frame()", lambda cd: cd.keep_auto_frame())
        assert np.array_equal(_bits(fg[0]), _bits(fs[0])) and np.array_equal(_bits(fg[1]), _bits(fs[1])) and fg[2] == fs[2]
        self.frame = ("custom", tuple(fg[0]), tuple(fg[1]), fg[2])

    # ---- one step on both contexts, and everything compared
    def step(self, cap=CAP, into=False, expect_replay=None):
        self.log.append(f"step(cap={cap}{', into HostPairs' if into else ''})")
        try:
            self._step(cap, into, expect_replay)
        except AssertionError as e:
            raise AssertionError(f"{e}\noperation log:\n  " + "\n  ".join(self.log)) from None

    def _collide(self, cd, cap, into):
        if not into:
            return cd.self_collide(cap=cap)
        hp = self._host.get((id(cd), cap))
        if hp is None:
            hp = self._host[(id(cd), cap)] = mi355cd.HostPairs(cap)
        n, rc = cd.self_collide_into(hp.array)
        return hp.array[:min(n, cap)].copy(), n, rc

    def _step(self, cap, into, expect_replay):
        g, s = self.g, self.s
        form0 = g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM)
        rep0 = g.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS)
        pg, ng, rcg = self._collide(g, cap, into)
        ps, ns, rcs = self._collide(s, cap, into)
        # a replay: one graph launch and no traversal kernel of its own -- or a replayed tree whose pass deferred subtrees, which the stream
        # path's traversal finishes (graph_step; the step after it runs on the stream, with its memset)
        stg = g.stats()
        ran = g.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) == rep0 + 1
        continued = ran and stg.traverse_launches != 0 and stg.stack_overflows > 0
        replayed = ran and (stg.traverse_launches == 0 or continued)
        why = ("replays", g.debug_get(mi355cd.CD_DBG_GET_GRAPH_REPLAYS) - rep0, "captures", g.debug_get(mi355cd.CD_DBG_GET_GRAPH_CAPTURES),
               "launches", stg.traverse_launches, "deferred", stg.stack_overflows)
        r = self.ref()
        want, nwant = oracle.pair_set(r["pairs"]), r["stats"].n_pairs
        # return values and pairs
        assert (rcg, ng) == (rcs, ns), ("rc / n", (rcg, ng), (rcs, ns))
        assert ng == nwant and rcg == (mi355cd.CD_OVERFLOW if nwant > cap else mi355cd.CD_OK), ("n vs oracle", ng, nwant, rcg)
        for name, p in (("G", pg), ("S", ps)):
            got = oracle.pair_set(p)
            if nwant <= cap:
                assert np.array_equal(got, want), f"{name}: pair set differs from the oracle's"
            else:                                       # (which pairs make it into a list that overflows is a race: any cap distinct true ones)
                assert len(got) == cap and len(np.unique(got)) == cap and np.isin(got, want).all(), f"{name}: overflowing list"
        if nwant <= cap:
            assert np.array_equal(oracle.pair_set(pg), oracle.pair_set(ps))
        # statistics
        sg, ss = g.stats(), s.stats()
        assert (sg.n_pairs, sg.pairs_tested) == (ss.n_pairs, ss.pairs_tested) == (nwant, r["stats"].pairs_tested), \
            ("stats", (sg.n_pairs, sg.pairs_tested), (ss.n_pairs, ss.pairs_tested), (nwant, r["stats"].pairs_tested))
        # keys and permutation
        kg, permg = g.export_keys()
        ks, perms = s.export_keys()
        assert np.array_equal(kg, ks) and np.array_equal(permg, perms), "keys / permutation: G != S"
        assert np.array_equal(kg, r["keys"]), "keys differ from the oracle's for this frame"
        assert np.array_equal(permg, r["perm"]), "permutation differs from the oracle's"
        # the frame the sort used
        fg, fs = g.get_morton_frame(), s.get_morton_frame()
        off, span, lay = self.expected_frame()
        assert np.array_equal(_bits(fg[0]), _bits(fs[0])) and np.array_equal(_bits(fg[1]), _bits(fs[1])) and fg[2] == fs[2], ("frame G != S", fg, fs)
        assert np.array_equal(_bits(fg[0]), _bits(off)) and np.array_equal(_bits(fg[1]), _bits(span)) and fg[2] == lay, ("frame", fg, (off, span, lay))
        # sort state and build
        for k in (mi355cd.CD_DBG_GET_SORT_FORM, mi355cd.CD_DBG_GET_TREE_WAS_FUSED):
            assert g.debug_get(k) == s.debug_get(k), ("debug state", k, g.debug_get(k), s.debug_get(k))
        assert sg.sort_passes == ss.sort_passes, ("sort passes", sg.sort_passes, ss.sort_passes)
        # anti-vacuity: the second step after a change, under options that allow it, is one graph launch
        form1 = g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM)
        if expect_replay is None:
            expect_replay = self.eligible() and self.since_change >= 1 and form0 == form1 == 0 and not self.last_continued
        if expect_replay:
            assert replayed, ("G did not replay this step",) + why
        if not self.eligible():
            assert not replayed, ("G replayed a step its options make ineligible",) + why
        self.replays += replayed
        self.last_continued = continued
        self.since_change += 1

    def steps(self, k=3, **kw):
        for _ in range(k):
            self.step(**kw)


def _twin(verts, vidx, ids=None):
    t = Twin(verts, vidx, ids)
    t.steps(3)
    assert t.replays >= 2
    return t


def _cloth(quads=100, round_f32=True):
    return synth.cloth_pair(quads, round_f32=round_f32)


def _frame_of_centroids(verts, vidx, pad=0.0):
    cen = (verts[vidx[:, 0]] + verts[vidx[:, 1]] + verts[vidx[:, 2]]) / 3
    lo, hi = cen.min(0), cen.max(0)
    return lo - pad, (hi - lo) * (1.0 + 2.0 ** -20) + 2 * pad


def _other_layout(lay):
    """A valid layout word with the same bit counts and the first two axes swapped."""
    (a, b, c), na, nab, nabc = oracle.layout_fields(lay)
    return oracle.layout_word((b, a, c), na, nab, nabc)


# ---- 1. frame transitions ------------------------------------------------------------------------------------------------------

def _frame_cycle(t, steps=3):
    off, span, lay = oracle.auto_frame(t.verts, t.vidx)
    assert lay != 0 and _other_layout(lay) != lay
    coff, cspan = _frame_of_centroids(t.verts, t.vidx, pad=0.01)
    t.set_frame(mi355cd.CD_FRAME_REFERENCE); t.steps(steps)
    t.set_frame(mi355cd.CD_FRAME_CUSTOM, coff, cspan); t.steps(steps)
    t.set_frame_layout(coff, cspan, lay); t.steps(steps)                   # layout 0 -> L: k_morton<false> -> k_morton<true>
    t.set_frame(mi355cd.CD_FRAME_CUSTOM, coff, cspan); t.steps(steps)      # L -> 0: back to the reference's interleave
    t.set_frame_layout(coff, cspan, _other_layout(lay)); t.steps(steps)    # 0 -> L'
    t.set_frame_layout(coff, cspan, lay); t.steps(steps)                   # L' -> L: the same instance, another word
    t.set_frame(mi355cd.CD_FRAME_AUTO); t.steps(steps)
    t.keep_auto_frame(); t.steps(steps)                                    # the AUTO frame kept: CUSTOM with its layout
    t.set_frame(mi355cd.CD_FRAME_CUSTOM, coff * 1.01 - 0.003, cspan * np.array([1.2, 1.05, 1.1])); t.steps(steps)   # per-axis, layout 0
    t.set_frame(mi355cd.CD_FRAME_REFERENCE); t.steps(steps)


def _config4_in_reference_frame(quads):
    """config 4's merged shards squeezed along x into the reference's frame: a mesh whose AUTO layout is far from the plain interleave."""
    verts, vidx, ids, _, _ = synth.config4_merged(8, quads)
    verts = verts.copy()
    verts[:, 0] *= 0.14
    return verts.astype(np.float32).astype(np.float64), vidx, ids


def test_frame_transitions_between_replays():
    """REFERENCE -> CUSTOM -> CUSTOM with layout L -> CUSTOM -> L' -> L -> AUTO -> the AUTO frame kept -> CUSTOM per axis -> REFERENCE, three
    steps after each.  A replay that kept the previous frame's k_morton instance gives keys in the wrong interleave (0 -> L) or all-zero keys
    whose sort escalates for good (L -> 0)."""
    verts, vidx, ids = _config4_in_reference_frame(40)                     # 51 200 triangles
    t = _twin(verts, vidx, ids)
    try:
        _frame_cycle(t)
    finally:
        t.close()


def test_frame_transitions_between_replays_of_a_large_tree():
    """The same on a tree of more than 2048 blocks, whose captured step also holds k_tile_chunks and the published upper levels."""
    verts, vidx = synth.cloth_pair(600)                                    # 1 440 000 triangles
    t = _twin(verts, vidx)
    try:
        _frame_cycle(t, steps=2)
    finally:
        t.close()


# ---- 2. sort forms under replay --------------------------------------------------------------------------------------------------

def test_sort_form_cycle_when_the_mesh_leaves_the_frame_and_comes_back():
    """The graph-on twin of test_sort_returns_to_its_first_form_when_the_mesh_is_back_inside_the_frame: leaving the frame during replays
    redoes the step in form 1 and captures again; every 64th sort tries form 0 while outside; back inside, form 0 and replays resume."""
    verts, vidx = _cloth()
    out = verts.copy(); out[verts.shape[0] // 2:, 0] += 0.2                 # sheet B beyond x = 3.0845: keys beyond 2^60
    t = _twin(verts, vidx)
    try:
        t.update_vertices(out, "update_vertices(out of the frame)")
        t.step(expect_replay=False)
        assert t.g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM) == 1
        t.steps(2, expect_replay=True)                                    # form 1 captured and replayed
        r0 = t.replays
        t.steps(70, expect_replay=False)                                   # one of these tries form 0, fails and is redone
        assert t.g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM) == 1 and t.replays - r0 >= 68
        t.update_vertices(verts, "update_vertices(back inside)")
        forms = []
        r0 = t.replays
        for _ in range(70):
            t.step(expect_replay=False)
            forms.append(t.g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM))
        assert forms[0] == 1 and forms[-1] == 0 and forms == sorted(forms, reverse=True)
        assert t.replays - r0 >= 66
        t.steps(3)
    finally:
        t.close()


def _clustered(verts, vidx, k, cell_frac, jitter, seed):
    """The first k triangles moved into ONE cell of the reference frame's top key bits (cell_frac: the cell's size per axis as a fraction
    of the frame), spread over it, each triangle `jitter` wide."""
    rng = np.random.default_rng(seed)
    cell = synth.REF_SPAN * np.asarray(cell_frac)
    c0 = synth.REF_OFF + 0.5 * synth.REF_SPAN + 0.5 * cell
    v = verts.copy()
    cl = (c0 + (rng.random((k, 1, 3)) - 0.5) * 0.6 * cell + (rng.random((k, 3, 3)) - 0.5) * jitter).reshape(-1, 3)
    v[vidx[:k].reshape(-1)] = cl
    return v.astype(np.float32).astype(np.float64)


def test_sort_form_escalations_under_replay():
    """A run of equal top digits too long for any window (SORTF_RUN: no hybrid form), then more than FIX_MAX keys with one high half
    (SORTF_FIXUP: all eight passes), each raised by a REPLAYED step; then CD_OPT_SORT_FULL 0 and the plain mesh: form 0 and replays again."""
    verts, vidx = synth.soup(40_000, 0.03, 7)
    t = _twin(verts, vidx)
    try:
        run = _clustered(verts, vidx, 8000, [1 / 64, 1 / 32, 1 / 32], 1e-3, 61)
        top = np.sort(oracle.centroid_morton(run, vidx) >> np.uint64(44))
        assert np.unique(top, return_counts=True)[1].max() > 6144
        t.update_vertices(run, "update_vertices(8000 keys in one top-16-bit cell)")
        t.step(expect_replay=False)
        assert t.g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM) >= 2                 # (no window form can sort it)
        t.steps(2)
        fix = _clustered(verts, vidx, 40, [1 / 2048, 1 / 2048, 1 / 2048], 1e-6, 62)
        hi = np.unique(oracle.centroid_morton(fix, vidx) >> np.uint64(32), return_counts=True)[1]
        assert hi.max() > 16
        t.update_vertices(verts, "update_vertices(plain)")
        t.set_option(mi355cd.CD_OPT_SORT_FULL, 0, "SORT_FULL")
        t.steps(3)
        assert t.g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM) == 0
        t.update_vertices(fix, "update_vertices(40 keys with one high half)")
        t.step(expect_replay=False)
        assert t.g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM) == 3
        t.steps(2)
        t.update_vertices(verts, "update_vertices(plain)")
        t.set_option(mi355cd.CD_OPT_SORT_FULL, 0, "SORT_FULL")
        t.steps(3)
        assert t.g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM) == 0
    finally:
        t.close()


def test_sort_full_option_between_replays():
    verts, vidx = _cloth()
    t = _twin(verts, vidx)
    try:
        for v in (1, 2, 0, 2, 1, 0):
            t.set_option(mi355cd.CD_OPT_SORT_FULL, v, "SORT_FULL")
            t.steps(3)
            assert t.g.debug_get(mi355cd.CD_DBG_GET_SORT_FORM) == {0: 0, 1: 3, 2: 2}[v]
            assert t.g.stats().sort_passes == {0: 2, 1: 8, 2: 4}[v]
    finally:
        t.close()


# ---- 3. options and debug switches between replays -------------------------------------------------------------------------------

O, D = "opt", "dbg"
TOGGLES = [
    (O, "ORDER_HINT", [0]), (O, "ORDER_HINT", [2]), (O, "ORDER_HINT", [1]),
    (O, "CELL_TABLE", [0]), (O, "TRAVERSAL", [1, 0]), (O, "STAGE_TIMING", [1]), (O, "KERNEL_STAMPS", [15]), (O, "KERNEL_STAMPS", [2]),
    (O, "POLL", [0]), (O, "QUERIES_PER_WAVE", [128]), (O, "GRAPH", [0]),
    (D, "SORT_WINDOWS", [1]), (D, "SORT_WINDOWS", [2]), (D, "REPORT_COPIES", [1]), (D, "STORE_QBOX", [1]), (D, "BIG_OFFSETS", [1]),
    (D, "EXACT_BLOCKS", [128]), (D, "NO_SHARED_PATH", [1]), (D, "SPLIT_CROSS", [1]), (D, "STAGEWISE_BUILD", [1]), (D, "DIAG", [1]),
    (D, "LDS_PAD", [4096]), (D, "POLL_SCAN", [1]),
]
DEFAULTS = {"ORDER_HINT": 1, "CELL_TABLE": 1, "TRAVERSAL": 3, "STAGE_TIMING": 0, "KERNEL_STAMPS": 0, "POLL": 1, "QUERIES_PER_WAVE": 64,
            "SORT_WINDOWS": 0, "REPORT_COPIES": 0, "STORE_QBOX": 0, "BIG_OFFSETS": 0, "EXACT_BLOCKS": 1024, "NO_SHARED_PATH": 0,
            "SPLIT_CROSS": 0, "STAGEWISE_BUILD": 0, "DIAG": 0, "LDS_PAD": 0, "POLL_SCAN": 0}


def _toggle(t, kind, name, value):
    if kind == O and name == "GRAPH":                                      # G only: S never replays
        t.both(f"set_option(GRAPH, {value}) on G", lambda cd: cd.set_option(mi355cd.CD_OPT_GRAPH, value) if cd is t.g else None)
        t.opts["graph"] = value
    elif kind == O:
        t.set_option(getattr(mi355cd, "CD_OPT_" + name), value, name)
    else:
        t.debug_set(getattr(mi355cd, "CD_DBG_" + name), value, name)


@pytest.mark.parametrize("kind,name,values", TOGGLES, ids=[f"{k}-{n}-{'-'.join(map(str, v))}" for k, n, v in TOGGLES])
def test_option_toggle_between_replays(kind, name, values):
    """Set on both twins, three steps, restore, three steps: an option that keeps the step eligible must not replay the old capture; one that
    makes it ineligible falls back to the stream and replays again once cleared.  Full doubles, so that the cell table is in play."""
    verts, vidx = _cloth(round_f32=False)
    t = _twin(verts, vidx)
    try:
        for v in values + [1 if name == "GRAPH" else DEFAULTS[name]]:
            _toggle(t, kind, name, v)
            t.steps(3)
        assert t.eligible()
    finally:
        t.close()


# ---- 4. calls between replays ----------------------------------------------------------------------------------------------------

def _op_stagewise(t):
    r = t.ref()
    t.both("morton_sort()", lambda cd: cd.morton_sort())
    w = t.both("build_hierarchy()", lambda cd: cd.build_hierarchy())
    assert w[0] == w[1] == r["parent_wrong"]
    t.both("refit_boxes()", lambda cd: cd.refit_boxes())
    (pg, ng, _), (ps, ns, _) = t.both("find_collisions()", lambda cd: cd.find_collisions(CAP))
    assert ng == ns == r["stats"].n_pairs and np.array_equal(oracle.pair_set(pg), oracle.pair_set(r["pairs"]))
    assert np.array_equal(oracle.pair_set(ps), oracle.pair_set(r["pairs"]))


def _op_build_tree(t):
    t.both("build_tree()", lambda cd: cd.build_tree())
    kg, ks = t.both("export_keys()", lambda cd: cd.export_keys()[0], change=False)
    assert np.array_equal(kg, ks) and np.array_equal(kg, t.ref()["keys"])


def _op_brute_force(t):
    want = oracle.pair_set(t.ref()["pairs"])                               # (every pair in contact: what the traversal finds)
    for (p, n, rc) in t.both("brute_force()", lambda cd: cd.brute_force(True, CAP)):
        assert rc == 0 and n == len(want) and np.array_equal(oracle.pair_set(p), want)


def _op_test_pairs(t):
    r = t.ref()
    rng = np.random.default_rng(5)
    p = np.concatenate([r["pairs"][:500], rng.integers(0, t.vidx.shape[0], (500, 2)).astype(np.uint32)])
    want = oracle.tri_contact_batch(t.verts, t.vidx, p, t.ids)
    og, os_ = t.both("test_pairs()", lambda cd: cd.test_pairs(p))
    assert np.array_equal(og, os_) and np.array_equal(og.astype(bool), np.asarray(want).astype(bool))


def _op_sorted_pairs(t):
    want = oracle.pair_set(t.ref()["pairs"])
    for (p, n, rc) in t.both("sorted_pairs()", lambda cd: cd.sorted_pairs(CAP)):
        k = (p[:, 0].astype(np.uint64) << np.uint64(32)) | p[:, 1]
        assert rc == 0 and np.array_equal(k, want)


def _op_collision_triangles(t):
    want = np.unique(t.ref()["pairs"])
    for (ids, n, rc) in t.both("collision_triangles()", lambda cd: cd.collision_triangles()):
        assert rc == 0 and np.array_equal(ids, want)


def _op_checks(t):
    ig, is_ = t.both("check_internal()", lambda cd: cd.check_internal())
    lg, ls = t.both("check_leaves()", lambda cd: cd.check_leaves())
    tg, ts = t.both("check_triangle_idx()", lambda cd: cd.check_triangle_idx(t.verts.shape[0]))
    assert ig.tolist() == is_.tolist() == [1, 0, 0, 0, 0] and lg.tolist() == ls.tolist() == [0, 0, 0, 0] and tg == ts == 0


def _order(p):
    return np.argsort((p[:, 0].astype(np.uint64) << np.uint64(32)) | p[:, 1], kind="stable")


def _op_proximity(t):
    (pg, dg, ng, _), (ps, ds, ns, _) = t.both("self_proximity(1e-3)", lambda cd: cd.self_proximity(1e-3))
    og, os_ = _order(pg), _order(ps)
    assert ng == ns > 0 and np.array_equal(pg[og], ps[os_]) and np.array_equal(_bits(dg[og]), _bits(ds[os_]))


def _op_ccd(t):
    end = t.verts + 1e-3 * np.sin(7.0 * t.verts[:, [2, 0, 1]])
    (pg, tg, dg, ng, _), (ps, ts, ds, ns, _) = t.both("self_ccd()", lambda cd: cd.self_ccd(end, 1e-4))
    og, os_ = _order(pg), _order(ps)
    assert ng == ns > 0 and np.array_equal(pg[og], ps[os_]) and np.array_equal(_bits(tg[og]), _bits(ts[os_]))


def _op_export_tree(t):
    r = t.ref()
    for parent, left, right, boxes, bounded in t.both("export_tree()", lambda cd: cd.export_tree()):
        assert np.array_equal(left, r["left"]) and np.array_equal(right, r["right"]) and np.array_equal(parent, r["parent"])
        assert np.array_equal(_bits(boxes), _bits(r["boxes"]))


def _op_debug_records(t):
    a, b = t.both("debug_records()", lambda cd: cd.debug_records())
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def _op_root_box(t):
    bg, bs = t.both("root_box()", lambda cd: cd.root_box(), change=False)
    assert np.array_equal(_bits(bg), _bits(bs)) and np.array_equal(_bits(bg), _bits(t.ref()["boxes"][0]))


def _op_queries(t):
    """A peer context (the engine wrapper of the cross-rank pass) packs its leaves that overlap the twins' root box; both twins traverse them."""
    import torch
    import mi355_multi as multi
    r = t.ref()
    nv, nt = t.verts.shape[0], t.vidx.shape[0]
    pv = t.verts + np.array([0.37, 0.0, 0.0]) * (t.verts.max(0) - t.verts.min(0))
    peer = multi.HipEngine(pv, t.vidx, (np.arange(nt) + nt).astype(np.uint32), torch.device("cuda", 0), vertex_id_base=nv)
    try:
        peer.cd.self_collide(CAP)
        q = peer.pack_queries(t.g.root_box())
        nq = q.numel() // multi.QUERY_BYTES
        assert nq > 0
        torch.cuda.synchronize()
        want, st = oracle.find_collisions_queries(q.cpu().numpy().view(mi355cd.QUERY_DTYPE), t.verts, t.vidx, r["perm"], r["left"], r["right"],
                                                  r["boxes"], t.ids)
        res = t.both("find_collisions_queries(peer)", lambda cd: cd.find_collisions_queries(q.data_ptr(), nq, CAP) + (cd.stats().pairs_tested,))
        for p, n, rc, tested in res:
            assert rc == 0 and n == st.n_pairs and tested == st.pairs_tested and np.array_equal(oracle.pair_set(p), oracle.pair_set(want))
    finally:
        peer.close()


def _op_move_small(t):
    v = t.verts.copy(); v[:, 1] += 0.002 * np.sin(30.0 * v[:, 0] + t.vver)
    t.update_vertices(v.astype(np.float32).astype(np.float64), "update_vertices(small move)")


def _op_to_double(t):
    v = t.verts + 1e-9 * np.cos(11.0 * t.verts)                            # not fp32 values: a cell table
    t.update_vertices(v, "update_vertices(doubles)")


def _op_to_float(t):
    t.update_vertices(t.verts.astype(np.float32).astype(np.float64), "update_vertices(floats)")


def _op_cell_table_off_on(t):
    _op_to_double(t)
    t.steps(2)
    t.set_option(mi355cd.CD_OPT_CELL_TABLE, 0, "CELL_TABLE")
    t.steps(2)
    _op_to_float(t)
    t.steps(2)
    _op_to_double(t)
    t.set_option(mi355cd.CD_OPT_CELL_TABLE, 1, "CELL_TABLE")


def _op_out_and_back(t):
    v = t.verts.copy(); v[v.shape[0] // 2:, 0] += 0.2
    back = t.verts
    t.update_vertices(v, "update_vertices(out of the frame)")
    t.steps(3)
    t.update_vertices(back, "update_vertices(back)")


def _op_capacity(t):
    t.step(cap=16)                                                         # CD_OVERFLOW: the true count comes back
    t.step(cap=16)
    t.step(cap=1 << 18)                                                    # another capacity: another capture
    t.step(cap=1 << 18, into=True)                                         # a pinned buffer
    t.step(cap=1 << 18, into=True)


INTERLEAVED = {
    "stagewise": _op_stagewise, "build_tree": _op_build_tree, "brute_force": _op_brute_force, "test_pairs": _op_test_pairs,
    "sorted_pairs": _op_sorted_pairs, "collision_triangles": _op_collision_triangles, "checks": _op_checks, "proximity": _op_proximity,
    "ccd": _op_ccd, "export_tree": _op_export_tree, "debug_records": _op_debug_records, "root_box": _op_root_box, "queries": _op_queries,
    "move_small": _op_move_small, "float_double": _op_cell_table_off_on, "out_and_back": _op_out_and_back, "capacity": _op_capacity,
}


@pytest.mark.parametrize("op", list(INTERLEAVED))
def test_call_between_replays(op):
    verts, vidx = _cloth()
    t = _twin(verts, vidx)
    try:
        for _ in range(2):
            INTERLEAVED[op](t)
            t.steps(3)
        assert t.eligible()
    finally:
        t.close()


# ---- 4b. item queries between replays ---------------------------------------------------------------------------------------------
# cd_cast_rays, cd_closest_points, cd_points_within, cd_cast_rays_all, cd_sweep_points_all and cd_sweep_points read what the captured step
# rewrites (d_root, d_leaf, d_perm[0], the ticket words) and enqueue their own work on the context's stream.  None of them changes what a
# step would enqueue (change=False): the replays after them go on, and stay right.

NITEMS = 256
CLOTH_EDGE = 2.88 / 100


def _items(t, kind):
    """256 rays / points / swept items derived from t.verts, with the restatement's answer; computed once per vertex array."""
    key = ("items", kind, t.vver)
    if key not in t._cache:
        if kind == "rays":
            rays = rr.mesh_rays(t.verts, t.vidx, NITEMS, seed=5)
            t._cache[key] = (rays, rr.cast_rays_ref(t.verts, t.vidx, t.ids, rays), wr.cast_rays_all_ref(t.verts, t.vidx, t.ids, rays))
        elif kind == "points":
            pts = ptr.mesh_points(t.verts, t.vidx, NITEMS, seed=5, edge=CLOTH_EDGE)
            rows = wr.points_within_ref(t.verts, t.vidx, t.ids, pts, 3 * CLOTH_EDGE)
            t._cache[key] = (pts, ptr.closest_points_ref(t.verts, t.vidx, t.ids, pts), rows)
        else:
            p0 = ptr.mesh_points(t.verts, t.vidx, NITEMS, seed=5, edge=CLOTH_EDGE)
            it = mi355cd.pack_sweeps(p0, p0 + np.random.default_rng(6).normal(size=p0.shape) * 0.6 * CLOTH_EDGE, CLOTH_EDGE / 4)
            end = t.verts + 1e-3 * np.sin(7.0 * t.verts[:, [2, 0, 1]])          # _op_ccd's end positions
            t._cache[key] = (it, end) + sr.sweep_rows_ref(t.verts, end, t.vidx, t.ids, it, counts=True)
    return t._cache[key]


def _same_columns(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, "column", k)


def _same_row_sets(g, s, want, what):
    """Two all-results calls' tuples (rows, values ..., n, rc): CD_OK, G's and S's rows bit-identical after sorting, and the restatement's."""
    for name, got in (("G", g), ("S", s)):
        assert got[-1] == mi355cd.CD_OK and got[-2] == got[0].shape[0] == want.rows.shape[0], (what, name, got[-2:], want.rows.shape[0])
        wr.same_rows(got[:-2], want, f"{what}: {name} against the restatement")
    _same_columns(wr.sort_rows(*g[:-2]), wr.sort_rows(*s[:-2]), what + ": G against S")


def _op_cast_rays(t):
    rays, want, _ = _items(t, "rays")
    g, s = t.both("cast_rays()", lambda cd: cd.cast_rays(rays[:, 0:3], rays[:, 3:6], rays[:, 6]), change=False)
    _same_columns(g[:5], s[:5], "cast_rays: G against S")
    _same_columns(g[:5], want, "cast_rays against the restatement")
    assert g[5].n_hits == s[5].n_hits == int((want[0] != mi355cd.RAY_MISS).sum()) > NITEMS // 8


def _op_closest_points(t):
    pts, want, _ = _items(t, "points")
    g, s = t.both("closest_points()", lambda cd: cd.closest_points(pts), change=False)
    _same_columns(g[:7], s[:7], "closest_points: G against S")
    _same_columns(g[:7], want, "closest_points against the restatement")
    assert g[7].n_found == s[7].n_found == NITEMS


def _op_points_within(t):
    pts, _, want = _items(t, "points")
    g, s = t.both("points_within()", lambda cd: cd.points_within(pts, 3 * CLOTH_EDGE, cap=CAP) + (cd.within_tested,), change=False)
    assert g[-1] == s[-1] >= want.rows.shape[0] > NITEMS
    _same_row_sets(g[:-1], s[:-1], want, "points_within")


def _op_cast_rays_all(t):
    rays, _, want = _items(t, "rays")
    g, s = t.both("cast_rays_all()", lambda cd: cd.cast_rays_all(rays[:, 0:3], rays[:, 3:6], rays[:, 6], cap=CAP) + (cd.rays_all_tested,), change=False)
    assert g[-1] == s[-1] >= want.rows.shape[0] > NITEMS // 8
    _same_row_sets(g[:-1], s[:-1], want, "cast_rays_all")


def _op_sweep_points_all(t):
    it, end, want, counts = _items(t, "sweeps")
    g, s = t.both("sweep_points_all()", lambda cd: cd.sweep_points_all(it[:, 0:3], it[:, 3:6], it[:, 6], verts_end=end, cap=CAP) + (bytes(cd.sweep_info),), change=False)
    assert want.rows.shape[0] > NITEMS // 8 and counts[2] == 0
    _same_row_sets(g[:-1], s[:-1], want, "sweep_points_all")
    info = mi355cd.CdCcdInfo.from_buffer_copy(g[-1])
    assert g[-1] == s[-1] and (info.n_tested, info.n_evals, info.n_unresolved) == counts, (info.n_tested, info.n_evals, info.n_unresolved, counts)


def _op_sweep_points(t):
    it, end, want, _ = _items(t, "sweeps")
    g, s = t.both("sweep_points()", lambda cd: cd.sweep_points(it[:, 0:3], it[:, 3:6], it[:, 6], verts_end=end), change=False)
    _same_columns(g[:8], s[:8], "sweep_points: G against S")
    _same_columns(g[:8], sr.first_of(want, NITEMS), "sweep_points against first_of of the restatement's rows")
    assert g[8].n_found == s[8].n_found == np.unique(want.rows[:, 0]).size > NITEMS // 8


ITEM_QUERIES = {
    "cast_rays": _op_cast_rays, "closest_points": _op_closest_points, "points_within": _op_points_within, "cast_rays_all": _op_cast_rays_all,
    "sweep_points_all": _op_sweep_points_all, "sweep_points": _op_sweep_points,
}


@pytest.mark.parametrize("op", list(ITEM_QUERIES))
def test_item_query_between_replays(op):
    """Two rounds of one item query on both twins and three steps: G's and S's results are bit-identical and the restatement's on the
    current vertices, and the steps after the query are replays again (Twin.step's anti-vacuity rule, unchanged: the query is no change)
    that still match the stream context and the oracle."""
    verts, vidx = _cloth()
    t = _twin(verts, vidx)
    try:
        for _ in range(2):
            ITEM_QUERIES[op](t)
            t.steps(3)
        assert t.eligible()
    finally:
        t.close()


# ---- 5. seeded random walk --------------------------------------------------------------------------------------------------------

def _walk_ops(t, base):
    coff, cspan = _frame_of_centroids(base, t.vidx, pad=0.01)
    _, _, lay = oracle.auto_frame(base, t.vidx)

    def opt(name, v, kind=O):
        return lambda: _toggle(t, kind, name, v)

    def restore_all():
        for kind, name, _ in TOGGLES:
            if name != "GRAPH":
                _toggle(t, kind, name, DEFAULTS[name])
        t.set_option(mi355cd.CD_OPT_SORT_FULL, 0, "SORT_FULL")

    ops = {name: (lambda f=f: f(t)) for name, f in INTERLEAVED.items()}
    ops.update({
        "frame_ref": lambda: t.set_frame(mi355cd.CD_FRAME_REFERENCE),
        "frame_custom": lambda: t.set_frame(mi355cd.CD_FRAME_CUSTOM, coff, cspan),
        "frame_layout": lambda: t.set_frame_layout(coff, cspan, lay),
        "frame_layout2": lambda: t.set_frame_layout(coff, cspan, _other_layout(lay)),
        "frame_auto": lambda: t.set_frame(mi355cd.CD_FRAME_AUTO),
        "keep_auto": lambda: t.keep_auto_frame() if t.frame[0] == "auto" else None,
        "restore_base": lambda: t.update_vertices(base, "update_vertices(base)"),
        "cap_small": lambda: t.step(cap=64),
        "cap_other": lambda: t.step(cap=1 << 17),
        "into": lambda: t.step(into=True),
        "restore_options": restore_all,
        "sort_full": lambda: t.set_option(mi355cd.CD_OPT_SORT_FULL, int(t.rng.integers(0, 3)), "SORT_FULL"),
    })
    for kind, name, values in TOGGLES:
        if name != "GRAPH":
            ops[f"{name}={values[0]}"] = opt(name, values[0], kind)
            ops[f"{name}=default"] = opt(name, DEFAULTS[name], kind)
    return ops


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_random_walk(seed):
    """About 60 operations drawn from all of the above on one mesh, one to three steps after each, every step compared.  A failure
    prints the operation log."""
    verts, vidx = _cloth()
    t = _twin(verts, vidx)
    t.rng = np.random.default_rng(1000 + seed)
    try:
        ops = _walk_ops(t, verts)
        names = sorted(ops)
        for _ in range(60):
            name = names[int(t.rng.integers(0, len(names)))]
            t.log.append(f"# op {name}")
            try:
                ops[name]()
            except AssertionError as e:
                if "operation log:" in str(e):
                    raise
                raise AssertionError(f"{e}\noperation log (seed {seed}):\n  " + "\n  ".join(t.log)) from None
            t.steps(int(t.rng.integers(1, 4)))
        assert t.replays >= 10, t.replays
    finally:
        t.close()
