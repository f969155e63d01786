"""Meshes that MOVE: the motion sequences of tests/test_moving_mesh_gpu.py, their per-frame queries and CPU references, and the
comparison helpers (no test in here: importing it generates nothing; everything is built on first use and cached).

A sequence is a list of vertex arrays over one fixed index array, with a seed, the mean edge length of frame 0 (the way query_meshes
carries `edge`) and, per frame, the factor its lengths are scaled by (distances and end positions follow it).  What each sequence is
for is in its builder's docstring; tests/test_moving_inputs.py holds them to it.

Every reference of a frame is the existing CPU restatement on that frame's vertices alone: nothing here knows what the frame before
it was, so a device result that matches is not the previous frame's (test_moving_inputs.py: consecutive frames differ enough)."""
from __future__ import annotations

import functools

import numpy as np

import between_ref as br
import box_ref as bx
import ccd_ref as cr
import column_ref as cref
import isect_ref as ir
import mi355_synth as synth
import mi355cd
import nearest_ref as nr
import nearest_self_ref as ns
import oracle
import plane_ref as plr
import point_ref as ptr
import proximity_ref as pr
import ray_ref as rr
import segment_ref as sg
import sweep_ref as sw
import swept_ref as sr
import swept_segment_ref as ssr
import within_ref as wn
import witness_ref as wr
from test_between_gpu import _same_ccd as same_between_ccd, _same_contact as same_between_contact, _same_prox as same_between_prox  # noqa: F401
from test_ccd_gpu import _same as _same_ccd
from test_inside_gpu import _same as same_inside  # noqa: F401
from test_points_gpu import _same as same_points
from test_proximity_gpu import _same as _same_prox
from test_rays_gpu import _same as same_rays  # noqa: F401
from test_witness_gpu import _same_as_plain as same_as_plain  # noqa: F401

NQ = 1000                       # rays, and points, a frame: 15 full waves and a ragged one of 40
MISS = 0xFFFFFFFF
OFFSET = 2.0 ** 20 + 0.37       # the translated tests' offset (test_rays_gpu.py, test_points_gpu.py)
TINY = (1, 2, 3, 63, 64, 65)
# the first candidate buffer of the proximity / CCD passes: 64 shards of max(4096, 16 n / 64) (test_swept_gpu.py's regrowth test)
first_candidate_buffer = lambda n: 64 * max(4096, (16 * n + 63) // 64)


def _f32(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64))


class Sequence:
    def __init__(self, name, seed, edge, vidx, frames, frame_mode="reference", scales=None, notes=None):
        self.name, self.seed, self.edge, self.vidx = name, seed, edge, np.ascontiguousarray(vidx, dtype=np.uint32)
        self.frames = [np.ascontiguousarray(v, dtype=np.float64) for v in frames]
        self.frame_mode = frame_mode                                           # "reference": morton.h's fixed frame; "auto": CD_FRAME_AUTO
        self.scales = [1.0] * len(frames) if scales is None else [float(s) for s in scales]
        self.notes = notes or {}
        assert len(self.scales) == len(self.frames) and all(v.shape == self.frames[0].shape for v in self.frames)

    @property
    def nt(self):
        return self.vidx.shape[0]

    def __len__(self):
        return len(self.frames)


# ---------------------------------------------------------------- the sequences
JITTER_DENSE, JITTER_DENSE_FRAME = 256, 2


def _jitter():
    """soup(3000, e = 0.05), its centroids drawn in to 0.7 of the generation box (the walk below stays inside the reference's Morton
    frame: leaving it is frame_exit's subject); every frame adds fresh normal noise of 0.4 edges to the frame before (rounded to
    fp32, like a loader's output), so the Morton order changes.  Frame 2 is the dense one: the scale of the first JITTER_DENSE
    triangles' centroids collapses to a fiftieth (the triangles keep their size), so every pair of them is a candidate -- 32 k pairs
    from a few neighbouring 64-query blocks, which overflows those blocks' shards of the first candidate buffers (4096 a shard for
    proximity and CCD) and makes those passes grow their buffers and run again.  Collapsing the whole soup
    far enough for the TOTAL to pass the first buffer would cost the CPU restatements more than 300 k exact pairs a query.  Frame 3
    continues from frame 1's walk and is sparse again, on the grown buffers."""
    seed, e = 101, 0.05
    v, i = synth.soup(3000, e=e, seed=seed)
    tri = v.reshape(-1, 3, 3)                                                   # (private vertices: triangle t owns vertices 3 t .. 3 t + 2)
    c = tri.mean(axis=1, keepdims=True)
    mid = 0.5 * (synth.BOX_LO + synth.BOX_HI)
    v = _f32((mid + (c - mid) * 0.7 + (tri - c)).reshape(-1, 3))
    g = np.random.default_rng(seed)
    frames, walk = [v], v
    for f in range(1, 7):
        walk = _f32(walk + g.normal(0.0, 0.4 * e, walk.shape))
        frames.append(walk)
    tri = frames[JITTER_DENSE_FRAME].reshape(-1, 3, 3).copy()
    k = JITTER_DENSE
    c = tri[:k].mean(axis=1, keepdims=True)
    c0 = c.mean(axis=0, keepdims=True)
    tri[:k] = c0 + (c - c0) * 0.02 + (tri[:k] - c)
    frames[JITTER_DENSE_FRAME] = _f32(tri.reshape(-1, 3))
    return Sequence("jitter", seed, e, i, frames)


SLIDE_QUADS = 24
SLIDE_SHRINK = 0.8
SLIDE_PATH = ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (1, 2), (0, 2))           # sheet B's position in quads along x and z: one quad a frame
SLIDE_QUAD = (2.88 / SLIDE_QUADS * SLIDE_SHRINK, 2.18 / SLIDE_QUADS * SLIDE_SHRINK)      # a quad's extent along x and along z


@functools.lru_cache(maxsize=None)
def _slide_base():
    """cloth_pair(24) drawn in to 0.8 of its size about the middle of the generation box (rounded to fp32), so that a sheet can slide
    two quads each way and stay inside the reference's Morton frame."""
    v, i = synth.cloth_pair(SLIDE_QUADS)
    mid = 0.5 * (synth.BOX_LO + synth.BOX_HI)
    return _f32(mid + (v - mid) * SLIDE_SHRINK), i


def _shifted(v, qx, qz):
    """bench.py's moving-mesh construction (mi355_synth has none): vertices shifted by whole quads, float-valued like the loader's output."""
    w = v.copy()
    w[:, 0] = np.float32(w[:, 0] + np.float32(qx * SLIDE_QUAD[0]))
    w[:, 2] = np.float32(w[:, 2] + np.float32(qz * SLIDE_QUAD[1]))
    return w


def _slide():
    """The cloth pair of _slide_base, sheet B sliding one quad a frame over sheet A (two along x, two along z, two back along x):
    neighbouring frames share sheet A's half of the tree."""
    v, i = _slide_base()
    half = v.shape[0] // 2
    frames = [np.concatenate([v[:half], _shifted(v[half:], qx, qz)]) for qx, qz in SLIDE_PATH]
    return Sequence("slide", 102, SLIDE_QUAD[0], i, frames)


SCALE_WALK_K = (0, 20, 60, 20, -40, 0, 0, 0)
SCALE_WALK_OFFSET_FRAME = 6


def _scale_walk():
    """soup(1000, e = 0.15) with a fresh jitter every frame, times 2^k for k = 0, 20, 60, 20, -40, 0 (inside the band of
    tests/scale_inputs.py), then one frame at + (2^20 + 0.37) -- full doubles, M = 2^20 -- and one back at the origin: M and the root
    box grow, shrink, grow and shrink again.  In CD_FRAME_AUTO (in the reference's frame all of these keys but frame 0's are one)."""
    seed, e = 103, 0.15
    v, i = synth.soup(1000, e=e, seed=seed)
    g = np.random.default_rng(seed)
    frames = []
    for f, k in enumerate(SCALE_WALK_K):
        w = _f32(v + g.normal(0.0, 0.3 * e, v.shape))
        frames.append(w + OFFSET if f == SCALE_WALK_OFFSET_FRAME else np.ldexp(w, k))
    return Sequence("scale_walk", seed, e, i, frames, frame_mode="auto", scales=[2.0 ** k for k in SCALE_WALK_K])


FRAME_EXIT_OUT = (2, 3)


def _frame_exit():
    """test_sort_returns_to_its_first_form_when_the_mesh_is_back_inside_the_frame's construction at cloth_pair(24): sheet B 0.2 beyond
    the reference's Morton frame in frames 2 and 3 (keys beyond 2^60: the sort takes its second form), inside before and after, with
    a jitter of a fifth of a quad from frame 1 on."""
    seed = 104
    v, i = synth.cloth_pair(24)
    quad = 2.88 / 24
    g = np.random.default_rng(seed)
    frames = [v]
    for f in range(1, 6):
        w = v + g.normal(0.0, 0.2 * quad, v.shape)
        if f in FRAME_EXIT_OUT:
            w[v.shape[0] // 2:, 0] += 0.2
        frames.append(_f32(w))
    return Sequence("frame_exit", seed, quad, i, frames)


def _float_double():
    """cloth_pair(24) with a fresh jitter every frame: fp32-representable vertices in the even frames, full doubles in the odd ones
    (test_update_vertices_switches_the_cell_table_on_and_off: the cell table comes and goes).  In CD_FRAME_AUTO, like that test."""
    seed = 105
    vd, i = synth.cloth_pair(24, round_f32=False)
    quad = 2.88 / 24
    g = np.random.default_rng(seed)
    frames = []
    for f in range(6):
        w = vd + g.normal(0.0, 0.2 * quad, vd.shape)
        frames.append(w if f % 2 else _f32(w))
    return Sequence("float_double", seed, quad, i, frames, frame_mode="auto")


COLLAPSE_FRAMES = (2,)
COLLAPSE_LOG2 = -22


def _collapse():
    """soup(1000, e = 0.08), jittered; in frame 2 the whole mesh is scaled by 2^-22 about the centre of one Morton cell of the
    reference's frame: every centroid lies in that cell (all keys equal: the sort's full form, a tree of index tie-breaks, compare
    test_every_morton_key_equal), the triangles are far below the fp32 spacing at 1 (full doubles: the cell table), and the frames
    after it are the ordinary soup again."""
    seed, e = 106, 0.08
    v, i = synth.soup(1000, e=e, seed=seed)
    g = np.random.default_rng(seed)
    cell = synth.REF_SPAN / 2.0 ** 20
    centre = synth.REF_OFF + (np.floor((np.array([1.5, -0.1, 0.75]) - synth.REF_OFF) / cell) + 0.5) * cell
    mid = 0.5 * (synth.BOX_LO + synth.BOX_HI)
    frames, scales, walk = [], [], v
    for f in range(6):
        if f:
            walk = _f32(walk + g.normal(0.0, 0.5 * e, walk.shape))
        if f in COLLAPSE_FRAMES:
            frames.append(centre + np.ldexp(walk - mid, COLLAPSE_LOG2)); scales.append(2.0 ** COLLAPSE_LOG2)
        else:
            frames.append(walk); scales.append(1.0)
    return Sequence("collapse", seed, e, i, frames, scales=scales)


def _tiny(n):
    """query_meshes' soup of n triangles (n = 1, 2, 3, 63, 64, 65: no record, one record, a wave and one more), jittered over 4 frames."""
    seed, e = 110 + n, 0.3
    v, i = synth.soup(n, e=e, seed=n)
    g = np.random.default_rng(seed)
    frames, walk = [v], v
    for f in range(1, 4):
        walk = _f32(walk + g.normal(0.0, 0.5 * e, walk.shape))
        frames.append(walk)
    return Sequence(f"tiny{n}", seed, e, i, frames)


_BUILDERS = {"jitter": _jitter, "slide": _slide, "scale_walk": _scale_walk, "frame_exit": _frame_exit, "float_double": _float_double,
             "collapse": _collapse, **{f"tiny{n}": functools.partial(_tiny, n) for n in TINY}}
NAMES = tuple(_BUILDERS)
LARGE = tuple(n for n in NAMES if not n.startswith("tiny"))


@functools.lru_cache(maxsize=None)
def seq(name) -> Sequence:
    return _BUILDERS[name]()


# ---------------------------------------------------------------- per-frame queries and their references (cached: the schedules share them)
def edge_at(name, f):
    s = seq(name)
    return s.edge * s.scales[f]


def prox_dist(name, f):
    return edge_at(name, f) / 4


def ccd_dist(name, f):
    return edge_at(name, f) / 10


def _brute(s):
    """The restatements take every pair on the tiny meshes and the grid's candidates (boxes widened by dist and M / 1024: every pair
    where M is large, as on scale_walk's translated frame and the collapsed one) on the others."""
    return s.nt <= 65


@functools.lru_cache(maxsize=None)
def x1(name, f):
    """The CCD end positions of frame f: test_ccd_gpu.py's _move (noise per vertex and one shift of the whole mesh) at that frame's scale,
    at half its size -- the restatement's cost goes with the pairs whose swept boxes meet."""
    s = seq(name)
    g = np.random.default_rng(s.seed)
    e = edge_at(name, f)
    v = s.frames[f]
    return v + g.normal(size=v.shape) * e * 0.15 + g.normal(size=(1, 3)) * e * 0.5


@functools.lru_cache(maxsize=None)
def rays(name, f):
    s = seq(name)
    return rr.mesh_rays(s.frames[f], s.vidx, NQ, seed=s.seed)


@functools.lru_cache(maxsize=None)
def want_rays(name, f):
    s = seq(name)
    return rr.cast_rays_ref(s.frames[f], s.vidx, None, rays(name, f))


@functools.lru_cache(maxsize=None)
def points(name, f):
    s = seq(name)
    return ptr.mesh_points(s.frames[f], s.vidx, NQ, seed=s.seed, edge=edge_at(name, f))


@functools.lru_cache(maxsize=None)
def want_points(name, f):
    s = seq(name)
    return ptr.closest_points_ref(s.frames[f], s.vidx, None, points(name, f))


@functools.lru_cache(maxsize=None)
def radii(name, f):
    return ptr.radii(want_points(name, f)[2], edge_at(name, f), seed=seq(name).seed)


@functools.lru_cache(maxsize=None)
def want_points_r(name, f):
    s = seq(name)
    return ptr.closest_points_ref(s.frames[f], s.vidx, None, points(name, f), radii(name, f))


@functools.lru_cache(maxsize=None)
def want_prox(name, f):
    s = seq(name)
    return pr.proximity_pairs(s.frames[f], s.vidx, None, prox_dist(name, f), brute=_brute(s))


@functools.lru_cache(maxsize=None)
def want_ccd(name, f):
    """(pairs, toi, dists), (pairs through the gate, evaluations)"""
    s = seq(name)
    return cr.ccd_pairs(s.frames[f], x1(name, f), s.vidx, None, ccd_dist(name, f), counts=True, brute=_brute(s))


@functools.lru_cache(maxsize=None)
def want_prox_witness(name, f):
    """witness_ref's Rows of cd_find_proximity_witness on frame f, sorted by (face a, face b)."""
    s = seq(name)
    return wr.witness_pairs(s.frames[f], s.vidx, dist=prox_dist(name, f), brute=_brute(s))


@functools.lru_cache(maxsize=None)
def want_ccd_witness(name, f):
    """witness_ref's Rows of cd_find_ccd_witness on frame f moving to x1(name, f)."""
    s = seq(name)
    return wr.witness_pairs(s.frames[f], s.vidx, dist=ccd_dist(name, f), verts_end=x1(name, f), brute=_brute(s))


@functools.lru_cache(maxsize=None)
def want_contour(name, f):
    """isect_ref's Rows of cd_find_collisions_contour on frame f (with `tested`, the pairs that reach tri_contact)."""
    s = seq(name)
    return ir.contour_pairs(s.frames[f], s.vidx, brute=_brute(s))


# ---------------------------------------------------------------- the all-results item queries and the swept points, frame by frame
INF_EVERY = 16                  # every 16th point of cd_points_within has no radius: every triangle is a row of it
GROWTH_AT, GROWTH_ITEMS, GROWTH_EDGES = 1024, 64, 3.0
SELF_SWEEP = ("slide", "float_double")          # the sequences with shared vertices: the mesh's own vertices as swept items
SELF_SWEEP_ITEMS = 1000


def _growth_block(name, f):
    """jitter's dense frame only: (p0, p1) of GROWTH_ITEMS items at the collapsed cluster's centroid (+ N(0, 0.1 e)), appended as items
    GROWTH_AT .. GROWTH_AT + 63 -- ONE whole 64-item block of the descent, whose candidates all go to one shard (number 16) of the
    candidate buffer; at a radius / dist of GROWTH_EDGES edges the block has more ROWS than the shard's first WITHIN_SHARD_FIRST slots
    (tests/test_moving_inputs.py), so the pass must grow the buffer and run again.  None on every other frame."""
    if (name, f) != ("jitter", JITTER_DENSE_FRAME):
        return None
    s, e = seq(name), edge_at(name, f)
    c0 = s.frames[f].reshape(-1, 3, 3)[:JITTER_DENSE].mean(axis=(0, 1))
    p0 = c0 + np.random.default_rng(1).normal(size=(GROWTH_ITEMS, 3)) * 0.1 * e
    return p0, p0 + np.random.default_rng(2).normal(size=(GROWTH_ITEMS, 3)) * 0.6 * e


def _filler(name, f):
    """The items NQ .. GROWTH_AT - 1 in front of the growth block: points a hundred edges and more beyond the mesh (no rows)."""
    s, e = seq(name), edge_at(name, f)
    return s.frames[f].max(axis=0) + 100.0 * e * (1.0 + np.arange(GROWTH_AT - NQ))[:, None]


@functools.lru_cache(maxsize=None)
def within_items(name, f):
    """(points [n, 3], radii [n]) of cd_points_within on frame f: points(name, f) at radius edge_at, every INF_EVERY-th at +inf; on
    jitter's dense frame the filler and the growth block behind them (n = 1088 there, NQ elsewhere)."""
    s, e = seq(name), edge_at(name, f)
    assert _brute(s) or s.nt <= 3000                                            # (63 points x every triangle: the restatement's rows)
    pts, r = points(name, f), np.full(NQ, e)
    r[::INF_EVERY] = np.inf
    blk = _growth_block(name, f)
    if blk is not None:
        pts = np.concatenate([pts, _filler(name, f), blk[0]])
        r = np.concatenate([r, np.full(GROWTH_AT - NQ, e), np.full(GROWTH_ITEMS, GROWTH_EDGES * e)])
    return np.ascontiguousarray(pts), np.ascontiguousarray(r)


@functools.lru_cache(maxsize=None)
def want_within(name, f) -> wn.PointRows:
    s = seq(name)
    return wn.points_within_ref(s.frames[f], s.vidx, None, *within_items(name, f))


@functools.lru_cache(maxsize=None)
def want_rays_all(name, f) -> wn.RayRows:
    """cd_cast_rays_all's rows of rays(name, f)."""
    s = seq(name)
    return wn.cast_rays_all_ref(s.frames[f], s.vidx, None, rays(name, f))


@functools.lru_cache(maxsize=None)
def sweep_items(name, f):
    """The items [n, 7] of the swept-point queries on frame f: points(name, f) moving by N(0, 0.6 edge_at) a coordinate, dist an eighth,
    a quarter and a half of edge_at by i % 3 (a lane that reads its neighbour's dist gets another one); on jitter's dense frame the
    filler (at rest) and the growth block behind them.  The mesh moves to x1(name, f), the CCD queries' end positions."""
    s, e = seq(name), edge_at(name, f)
    p0 = points(name, f)
    p1 = p0 + np.random.default_rng(s.seed + f).normal(size=p0.shape) * 0.6 * e
    dist = np.array([e / 8, e / 4, e / 2])[np.arange(NQ) % 3]
    blk = _growth_block(name, f)
    if blk is not None:
        pad = _filler(name, f)
        p0, p1 = np.concatenate([p0, pad, blk[0]]), np.concatenate([p1, pad, blk[1]])
        dist = np.concatenate([dist, np.full(GROWTH_AT - NQ, e / 4), np.full(GROWTH_ITEMS, GROWTH_EDGES * e)])
    return mi355cd.pack_sweeps(p0, p1, dist)


@functools.lru_cache(maxsize=None)
def want_sweep(name, f):
    """(sweep_ref's SweepRows, (pairs through the gate, evaluations, unresolved rows)) of sweep_items(name, f) against frame f moving to x1(name, f)."""
    s = seq(name)
    return sw.sweep_rows_ref(s.frames[f], x1(name, f), s.vidx, None, sweep_items(name, f), counts=True)


@functools.lru_cache(maxsize=None)
def want_sweep_still(name, f):
    """The same items against frame f at rest (verts_end = None)."""
    s = seq(name)
    return sw.sweep_rows_ref(s.frames[f], None, s.vidx, None, sweep_items(name, f), counts=True)


@functools.lru_cache(maxsize=None)
def self_sweep_items(name, f):
    """The vertex-face half of the mesh's own CCD pass: its first SELF_SWEEP_ITEMS vertices moving to x1 -> (items, skip_vertex)."""
    assert name in SELF_SWEEP
    v, e = seq(name).frames[f], x1(name, f)
    k = SELF_SWEEP_ITEMS
    return mi355cd.pack_sweeps(v[:k], e[:k], edge_at(name, f) / 4), np.arange(k, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def want_self_sweep(name, f):
    s = seq(name)
    items, skip = self_sweep_items(name, f)
    return sw.sweep_rows_ref(s.frames[f], x1(name, f), s.vidx, None, items, skip=skip, counts=True)


# ---------------------------------------------------------------- boxes, planes, segments and swept segments, frame by frame
NI = 250                        # segments and swept segments a frame: three full waves and a ragged one of 58
NBOX = 258                      # boxes of box_ref.make_boxes a frame: 32 of them are its `miss` kind (250 have 31; test_moving_inputs.py asks for 32 without a row)
POINT_BOXES = 16                # point boxes on vertices of the frame behind the root box, which is item NBOX of the boxes
NEAR_BOXES = 32                 # small boxes beside the surface behind those: whether they meet a face depends on the frame, not on their kind
NPLANES = 24
SEG_INF = (0, 128)              # the segments with r = +inf: every triangle is a row of them
SEG_POINT_EVERY = 8             # every eighth segment has b == a
SEG_GROWTH_AT = 256             # the growth block of the segments and swept segments: items 256 .. 319, one whole block of the descent
SWEPT_SEGMENT_SEED = 3          # (2 gives collapse's sparse frame 0 only 31 items with several rows, 3 gives 43; test_moving_inputs.py asks for 32)
EDGE_EVERY = 5                  # on SELF_SWEEP sequences every fifth edge of the mesh is swept against it


def _far(name, f, n):
    """n points a hundred edges and more beyond the mesh: the items between NI and the growth block (no rows)."""
    s, e = seq(name), edge_at(name, f)
    return s.frames[f].max(axis=0) + 100.0 * e * (1.0 + np.arange(n))[:, None]


@functools.lru_cache(maxsize=None)
def box_items(name, f):
    """The boxes [n, 6] of cd_boxes_overlap_all / cd_boxes_count on frame f: NBOX of box_ref.make_boxes on the frame's vertices (seed by
    frame), the frame's root box exactly (item NBOX: every triangle is a row, and inside), POINT_BOXES point boxes on vertices of
    the frame, where the closed comparison decides, and NEAR_BOXES boxes of half-width a tenth of an edge centred 0.05 to 0.5 edge beside
    a vertex of the frame.  Every kind of make_boxes meets the mesh or misses it by construction, in every frame alike; whether a
    near box does is a matter of where the faces of THIS frame lie, so CD_BOX_ANY's answer changes from frame to frame and differs
    on the previous frame's tree (tests/test_moving_inputs.py)."""
    s, e = seq(name), edge_at(name, f)
    v = s.frames[f]
    used = v[s.vidx.astype(np.int64)].reshape(-1, 3)
    at = used[np.random.default_rng(s.seed + 31 * f).integers(0, used.shape[0], POINT_BOXES)]
    g = np.random.default_rng(s.seed + 37 * f + 5)
    u = g.normal(size=(NEAR_BOXES, 3))
    c = used[g.integers(0, used.shape[0], NEAR_BOXES)] + u / np.linalg.norm(u, axis=1, keepdims=True) * (e * g.uniform(0.05, 0.5, NEAR_BOXES))[:, None]
    boxes = bx.make_boxes(v, s.vidx, e, NBOX, seed=s.seed + f)
    return np.ascontiguousarray(np.concatenate([boxes, bx.root_box(v, s.vidx)[None], np.stack([at, at], axis=2).reshape(-1, 6),
                                                np.stack([c - 0.1 * e, c + 0.1 * e], axis=2).reshape(-1, 6)]))


@functools.lru_cache(maxsize=None)
def stale_boxes(name, f) -> bx.BoxRows:
    """What a device that kept frame f - 1's tree would answer for frame f's boxes: the restatement on the previous frame's vertices."""
    s = seq(name)
    return bx.boxes_overlap_all_ref(s.frames[f - 1], s.vidx, None, box_items(name, f))


@functools.lru_cache(maxsize=None)
def want_boxes(name, f) -> bx.BoxRows:
    s = seq(name)
    return bx.boxes_overlap_all_ref(s.frames[f], s.vidx, None, box_items(name, f))


@functools.lru_cache(maxsize=None)
def plane_items(name, f):
    """The planes [NPLANES, 4] of cd_planes_cut_all / cd_planes_count on frame f: plane_ref.make_planes on the frame's vertices."""
    s = seq(name)
    return plr.make_planes(s.frames[f], s.vidx, NPLANES, seed=s.seed + f)


@functools.lru_cache(maxsize=None)
def want_plane_classes(name, f):
    """plane_ref.classes_ref: the class of every (plane, face) of frame f, uint8 [NPLANES, nt]."""
    s = seq(name)
    return plr.classes_ref(s.frames[f], s.vidx, plane_items(name, f))


@functools.lru_cache(maxsize=None)
def want_planes(name, f) -> plr.PlaneRows:
    s = seq(name)
    return plr.rows_of(s.frames[f], s.vidx, None, plane_items(name, f), want_plane_classes(name, f))


@functools.lru_cache(maxsize=None)
def segment_items(name, f):
    """The segments [n, 7] (a, b, r) of cd_segments_within / cd_segments_closest on frame f: a the frame's first NI points,
    b = a + N(0, 1 edge) a coordinate, r a quarter edge, one edge or two by i % 3; every SEG_POINT_EVERY-th is a point (b == a) and
    items SEG_INF have r = +inf.  On jitter's dense frame the filler and the growth block (a, b = the block's two positions, r =
    GROWTH_EDGES edges) behind them, as items SEG_GROWTH_AT .. SEG_GROWTH_AT + 63."""
    s, e = seq(name), edge_at(name, f)
    a = points(name, f)[:NI]
    b = a + np.random.default_rng(s.seed + 7 * f + 1).normal(size=a.shape) * e
    b[::SEG_POINT_EVERY] = a[::SEG_POINT_EVERY]
    r = np.array([e / 4, e, 2 * e])[np.arange(NI) % 3]
    r[list(SEG_INF)] = np.inf
    blk = _growth_block(name, f)
    if blk is not None:
        pad = _far(name, f, SEG_GROWTH_AT - NI)
        a, b = np.concatenate([a, pad, blk[0]]), np.concatenate([b, pad, blk[1]])
        r = np.concatenate([r, np.full(SEG_GROWTH_AT - NI, e), np.full(GROWTH_ITEMS, GROWTH_EDGES * e)])
    return mi355cd.pack_segments(a, b, r)


@functools.lru_cache(maxsize=None)
def want_segments(name, f) -> sg.SegRows:
    s = seq(name)
    return sg.segments_within_ref(s.frames[f], s.vidx, None, segment_items(name, f))


@functools.lru_cache(maxsize=None)
def swept_segment_items(name, f):
    """The items [n, 13] (a0, b0, a1, b1, dist) of the swept-segment queries on frame f: NI free segments at the frame's points, about
    one edge long, both ends moving by a common N(0, 0.6 edge) and N(0, 0.2 edge) of their own, dist a quarter edge; on jitter's dense
    frame the filler (at rest) and the growth block behind them.  The mesh moves to x1(name, f)."""
    s, e = seq(name), edge_at(name, f)
    g = np.random.default_rng(s.seed + 11 * f + SWEPT_SEGMENT_SEED)
    a0 = points(name, f)[:NI]
    b0 = a0 + g.normal(size=a0.shape) * 0.6 * e
    common = g.normal(size=a0.shape) * 0.6 * e
    a1, b1 = a0 + common + g.normal(size=a0.shape) * 0.2 * e, b0 + common + g.normal(size=a0.shape) * 0.2 * e
    dist = np.full(NI, e / 4)
    blk = _growth_block(name, f)
    if blk is not None:
        pad = _far(name, f, SEG_GROWTH_AT - NI)
        off = np.random.default_rng(3).normal(size=blk[0].shape) * 0.6 * e
        a0, b0 = np.concatenate([a0, pad, blk[0]]), np.concatenate([b0, pad, blk[0] + off])
        a1, b1 = np.concatenate([a1, pad, blk[1]]), np.concatenate([b1, pad, blk[1] + off])
        dist = np.concatenate([dist, np.full(SEG_GROWTH_AT - NI, e / 4), np.full(GROWTH_ITEMS, GROWTH_EDGES * e)])
    return np.ascontiguousarray(ssr.pack(a0, b0, a1, b1, dist))


@functools.lru_cache(maxsize=None)
def want_swept_segments(name, f):
    """(swept_segment_ref's SweepSegRows, (pairs through the gate, evaluations, unresolved rows)) of swept_segment_items(name, f) against
    frame f moving to x1(name, f)."""
    s = seq(name)
    return ssr.sweep_segment_rows_ref(s.frames[f], x1(name, f), s.vidx, None, swept_segment_items(name, f), counts=True)


@functools.lru_cache(maxsize=None)
def want_swept_segments_still(name, f):
    """The same items against frame f at rest (verts_end = None)."""
    s = seq(name)
    return ssr.sweep_segment_rows_ref(s.frames[f], None, s.vidx, None, swept_segment_items(name, f), counts=True)


@functools.lru_cache(maxsize=None)
def mesh_edges(name):
    """Every EDGE_EVERY-th edge [ne, 2] of a SELF_SWEEP sequence's mesh (test_sweep_segments_gpu.py's on `slide`)."""
    assert name in SELF_SWEEP
    t = np.asarray(seq(name).vidx)
    e = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]).astype(np.int64), axis=1), axis=0)
    return np.ascontiguousarray(e[::EDGE_EVERY].astype(np.uint32))


@functools.lru_cache(maxsize=None)
def self_swept_segment_items(name, f):
    """The edge-edge half of the mesh's own CCD pass: mesh_edges moving to x1, dist a quarter edge -> (items, skip_vertices)."""
    v, w, e = seq(name).frames[f], x1(name, f), mesh_edges(name)
    return np.ascontiguousarray(ssr.pack(v[e[:, 0]], v[e[:, 1]], w[e[:, 0]], w[e[:, 1]], edge_at(name, f) / 4)), e


@functools.lru_cache(maxsize=None)
def want_self_swept_segments(name, f):
    s = seq(name)
    items, skip = self_swept_segment_items(name, f)
    return ssr.sweep_segment_rows_ref(s.frames[f], x1(name, f), s.vidx, None, items, skip=skip, counts=True)


# ---------------------------------------------------------------- the mesh against itself and points inside it, frame by frame
NEAREST_SELF_EDGES = 1.0        # cd_nearest_self's radius in edges of the frame: at least half of a frame's rows have a partner within it
NEAREST_SELF_INF = {"scale_walk": (2, SCALE_WALK_OFFSET_FRAME), "collapse": (COLLAPSE_FRAMES[0], COLLAPSE_FRAMES[0] + 1)}
UNDER_VERTICES = 300            # about that many of a frame's vertices get a point under them


def nearest_self_r(name, f):
    return NEAREST_SELF_EDGES * edge_at(name, f)


@functools.lru_cache(maxsize=None)
def want_nearest_self(name, f):
    """(nearest_ref's NearestRows, played faces) of cd_nearest_self at rmax = nearest_self_r on frame f: the restatement of the proximity
    witness rows at that distance (every pair on the tiny meshes, the grid's candidates elsewhere), reduced per face."""
    s = seq(name)
    w = wr.witness_pairs(s.frames[f], s.vidx, dist=nearest_self_r(name, f), brute=_brute(s))
    return ns.reduce_pairs(s.nt, w.faces, w.pairs, w.dists, w.points, w.bary, w.feature)


def has_nearest_self_inf(name, f):
    """The frames whose rows at rmax = +inf are restated over all pairs: every frame of the tiny meshes; of the 1000-triangle soups
    scale_walk's k = 60 and translated frames and collapse's collapsed frame and the one after it."""
    return _brute(seq(name)) or f in NEAREST_SELF_INF.get(name, ())


@functools.lru_cache(maxsize=None)
def want_nearest_self_inf(name, f):
    """The rows of cd_nearest_self at rmax = +inf on frame f: nearest_self_ref.nearest_rows, every admissible pair, no box, no bound."""
    assert has_nearest_self_inf(name, f)
    s = seq(name)
    return ns.nearest_rows(s.frames[f], s.vidx, np.inf)


def _under(name, f):
    v = seq(name).frames[f]
    return v[::max(1, len(v) // UNDER_VERTICES)]


@functools.lru_cache(maxsize=None)
def inside_points(name, f, axis):
    """The points of cd_points_inside / cd_signed_distance on frame f: points(name, f), and behind them about UNDER_VERTICES of the
    frame's vertices moved half an edge down the axis -- their other two coordinates are a vertex's exactly, so column_tri's tie rule
    decides which face of that vertex owns the crossing."""
    under = _under(name, f).copy()
    under[:, axis] -= 0.5 * edge_at(name, f)
    return np.ascontiguousarray(np.concatenate([points(name, f), under]))


@functools.lru_cache(maxsize=None)
def want_inside(name, f, axis, parity=False):
    """column_ref.points_inside of inside_points(name, f, axis) on frame f: (inside, n_above, n_below, w_above, w_below), all faces."""
    s = seq(name)
    return cref.points_inside(inside_points(name, f, axis), s.frames[f], s.vidx, axis, parity)


@functools.lru_cache(maxsize=None)
def inside_tie_covers(name, f, axis):
    """How many of the under-vertex points of inside_points(name, f, axis) are covered by a face with an exact zero among its three
    E: the covers the tie rule decided."""
    s = seq(name)
    p = inside_points(name, f, axis)[NQ:]
    r = cref.column_tri(p[:, None, :], s.frames[f][s.vidx.astype(np.int64)][None], axis)
    return int(((r["cover"] != 0) & (r["E"] == 0).any(axis=-1)).any(axis=1).sum())


def _pipeline(mode, v, vidx):
    if mode == "auto":
        off, span, lay = oracle.auto_frame(v, vidx)
        return oracle.pipeline(v, vidx, off=off, span=span, layout=lay)
    return oracle.pipeline(v, vidx)


@functools.lru_cache(maxsize=None)
def want_step(name, f):
    """oracle.pipeline on frame f in the sequence's Morton frame: keys, permutation, tree, the collision step's pairs and counters."""
    s = seq(name)
    return _pipeline(s.frame_mode, s.frames[f], s.vidx)


def root_box(v, vidx):
    """cd_root_box: (xmin, xmax, ymin, ymax, zmin, zmax) over the triangles' vertices."""
    p = np.asarray(v, dtype=np.float64)[np.asarray(vidx).astype(np.int64).ravel()]
    return np.stack([p.min(axis=0), p.max(axis=0)], axis=1).ravel()


def want_root_box(name, f):
    s = seq(name)
    return root_box(s.frames[f], s.vidx)


def expected_swept(x0, x1_, vidx, step, m_bits, dist):
    """What cd_debug_swept, cd_debug_records and cd_export_keys return for a correct device, from the oracle's tree `step`
    (oracle.pipeline) and the restatement: the dict test_swept_gpu.py's _read makes (the static records hold their link and range words
    only here; their boxes, flag bits and the query boxes are pinned to records_ref.py's restatement by test_records_gpu.py)."""
    n = np.asarray(vidx).reshape(-1, 3).shape[0]
    none = np.zeros((0, 8), dtype=np.uint32)
    out = dict(perm=step["perm"], m_bits=int(m_bits), pad=sr.pad(int(m_bits), dist))
    if n < 2:
        return dict(out, srr=none, srl=none, rr=none, rl=none, up=np.zeros(0, dtype=np.int32))
    lo, hi = sr.swept_leaf_boxes(x0, x1_, vidx, step["perm"])
    (L, R, F, La), _ = sr.tree_from_karras(step["left"], step["right"], step["range_first"], step["range_last"])
    l_lo, l_hi, r_lo, r_hi = sr.swept_records((lo, hi), L, R, F, La)
    m = n - 1
    rr_, rl_ = np.zeros((n, 8), dtype=np.uint32), np.zeros((n, 8), dtype=np.uint32)
    rl_[:m, 0:3], rl_[:m, 3:6], rl_[:m, 6], rl_[:m, 7] = sr.bits(l_lo), sr.bits(l_hi), L.view(np.uint32), F.astype(np.uint32)
    rr_[:m, 0:3], rr_[:m, 3:6], rr_[:m, 6], rr_[:m, 7] = sr.bits(r_lo), sr.bits(r_hi), R.view(np.uint32), La.astype(np.uint32) | np.uint32(0x80000000)
    return dict(out, srr=rr_, srl=rl_, rr=rr_, rl=rl_, up=sr.parents(L, R))


@functools.lru_cache(maxsize=None)
def want_swept(name, f):
    s = seq(name)
    v, e = s.frames[f], x1(name, f)
    return expected_swept(v, e, s.vidx, want_step(name, f), sr.m_bits(v, e, s.vidx), ccd_dist(name, f))


@functools.lru_cache(maxsize=None)
def want_candidates(name, f):
    """n_candidates of cd_find_ccd on frame f (the pairs of query box and leaf box: independent of the tree's shape)."""
    s = seq(name)
    v, e = s.frames[f], x1(name, f)
    lo, hi = sr.swept_leaf_boxes(v, e, s.vidx, want_step(name, f)["perm"])
    return sr.expected_candidates(lo, hi, sr.pad(sr.m_bits(v, e, s.vidx), ccd_dist(name, f)))


@functools.lru_cache(maxsize=None)
def ccd_shard_load(name, f):
    """The largest number of candidates one shard of cd_find_ccd's candidate buffer is asked to hold on frame f: the descent runs 64
    queries (sorted leaves) a block and block b reserves in shard b & 63 (cd_proximity.h).  Above SHARD_FIRST the pass has to grow."""
    s = seq(name)
    v, e = s.frames[f], x1(name, f)
    lo, hi = sr.swept_leaf_boxes(v, e, s.vidx, want_step(name, f)["perm"])
    qlo, qhi = sr.query_boxes(lo, hi, sr.pad(sr.m_bits(v, e, s.vidx), ccd_dist(name, f)))
    n = lo.shape[0]
    per_query = np.zeros(n, dtype=np.int64)
    for r0 in range(0, n, 512):
        r1 = min(n, r0 + 512)
        ok = np.all((qlo[r0:r1, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= qhi[r0:r1, None, :]), axis=-1)
        ok &= np.arange(n)[None, :] > np.arange(r0, r1)[:, None]
        per_query[r0:r1] = ok.sum(axis=1)
    per_block = np.add.reduceat(per_query, np.arange(0, n, 64))
    return int(np.bincount(np.arange(per_block.shape[0]) & 63, weights=per_block).max())


SHARD_FIRST = 4096              # slots a shard of the first proximity / CCD candidate buffer has: max(4096, 16 n / 64), 4096 up to 16 k triangles


# ---------------------------------------------------------------- the comparisons (each raises AssertionError; test_moving_inputs.py plants the error)
def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def read_swept(cd, other=None):
    """test_swept_gpu.py's _read: the swept tree `cd` holds with the static records and the order it lies over."""
    srr, srl, up, mb, pad = cd.debug_swept(other)
    owner = cd if other is None else other
    rec_r, rec_l, _, _ = owner.debug_records()
    _, perm = owner.export_keys()
    return dict(srr=srr, srl=srl, up=up, m_bits=mb, pad=pad, rr=rec_r, rl=rec_l, perm=perm)


def same_prox(got, want, what=""):
    """got: find_proximity's (pairs, dists, n, rc); want: the restatement's sorted (pairs, dists)."""
    assert got[3] == 0 and got[2] == want[0].shape[0], (what, got[3], got[2], want[0].shape[0])
    _same_prox(got, want)


def same_ccd(got, want, what="", info=None, counts=None):
    """got: find_ccd's (pairs, toi, dists, n, rc); want: the restatement's sorted (pairs, toi, dists); info / counts: cd_ccd_info
    against the restatement's (pairs through the gate, evaluations), as test_ccd_gpu.py compares them."""
    assert got[4] == 0 and got[3] == want[0].shape[0], (what, got[4], got[3], want[0].shape[0])
    _same_ccd(got, want)
    if info is not None:
        assert (info.n_tested, info.n_evals) == tuple(counts), (what, info.n_tested, info.n_evals, counts)
        assert info.n_candidates >= info.n_tested, what


def same_any_hit(face, n_hits, rays_, verts, vidx, want, what=""):
    """test_any_hit_is_defined_where_it_is_defined's rule: WHETHER there is a hit is defined, and the triangle returned is one ray_tri hits."""
    assert np.array_equal(face != MISS, want[0] != MISS), what
    k = np.nonzero(face != MISS)[0]
    nt = np.asarray(vidx).shape[0]
    assert (face[k] < nt).all(), what
    tris = np.asarray(verts, dtype=np.float64)[np.asarray(vidx).astype(np.int64)]
    assert rr.ray_tri_np(rays_[k], tris[face[k]])[0].all(), what
    assert n_hits == k.size, what


def same_any_within(face, n_found, pts, rm, verts, vidx, want, what=""):
    """test_any_within_is_defined_where_it_is_defined's rule, for points."""
    assert np.array_equal(face != MISS, want[0] != MISS), what
    k = np.nonzero(face != MISS)[0]
    nt = np.asarray(vidx).shape[0]
    assert (face[k] < nt).all(), what
    tris = np.asarray(verts, dtype=np.float64)[np.asarray(vidx).astype(np.int64)]
    assert (ptr.pt_tri_np(pts[k], tris[face[k]])[0] <= np.broadcast_to(rm, (pts.shape[0],))[k]).all(), what
    assert n_found == k.size, what


def same_swept(t, x0, x1_, vidx, m_bits, dist, what="", leaves_perm_a=None, a=None, n_candidates=None):
    """The read-back `t` (read_swept) of the swept tree over (x0, x1_, vidx) against the restatement: links, up[], every box float, M
    and the pad, as test_swept_gpu.py's _check_self / _check_between do.  n_candidates: the descent's count, compared with the
    restatement's (self; between two meshes with a = (x0, x1, vidx, perm) of the query side)."""
    n = np.asarray(vidx).reshape(-1, 3).shape[0]
    lo, hi = sr.swept_leaf_boxes(x0, x1_, vidx, t["perm"])
    if n < 2:
        assert t["srr"].shape[0] == 0 and t["srl"].shape[0] == 0 and t["up"].shape[0] == 0, what
        halves = 0
    else:
        assert t["srr"].shape[0] == n, (what, t["srr"].shape[0], n)
        halves = sr.compare_links(t["rr"], t["rl"], t["srr"], t["srl"], t["up"])
        want = sr.swept_records((lo, hi), *sr.tree_from_records(t["rr"], t["rl"]))
        assert sr.compare_records(t["srr"], t["srl"], want, t["up"], what, leaves=(lo, hi)) == halves == 2 * (n - 1)
    p = sr.compare_pad(t["m_bits"], t["pad"], m_bits, dist)
    if n_candidates is not None:
        if a is None:
            sr.compare_count(n_candidates, sr.expected_candidates(lo, hi, p), what)
        else:
            lo_a, hi_a = sr.swept_leaf_boxes(*a)
            sr.compare_count(n_candidates, sr.expected_candidates(lo_a, hi_a, p, lo, hi), what)
    return halves


def same_root_box(got, want, what=""):
    assert np.array_equal(_bits(got), _bits(want)), (what, np.asarray(got).tolist(), np.asarray(want).tolist())


def same_step(pairs, n, rc, pairs_tested, step, what=""):
    """A collision step's own result against oracle.pipeline's: the pair set, the count and pairs_tested."""
    assert rc == 0 and n == step["stats"].n_pairs, (what, rc, n, step["stats"].n_pairs)
    assert np.array_equal(oracle.pair_set(pairs), oracle.pair_set(step["pairs"])), what
    assert pairs_tested == step["stats"].pairs_tested, (what, pairs_tested, step["stats"].pairs_tested)


def _same_bytes(got, want, what):
    """Two arrays of one type and shape with the same bytes: no tolerance, -0.0 is not 0.0 and a NaN equals only itself."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    if g.tobytes() != w.tobytes():
        bad = np.nonzero((g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1)).any(axis=1))[0]
        raise AssertionError((what, "rows that differ", bad.size, bad[:4].tolist()))


def witness_rows(got) -> wr.Rows:
    """A witness call's (pairs, [toi,] dists, n, rc, Witness) as witness_ref's Rows, sorted by (face a, face b)."""
    *cols, _, _, wit = got
    toi = cols[1] if len(cols) == 3 else None
    return wr.Rows(*wr.sort_rows(wit.faces, cols[0], toi, cols[-1], wit.points, wit.bary, wit.feature))


def witness_call(rows: wr.Rows, rc=0):
    """What a witness call that found `rows` returns."""
    cols = (rows.pairs, rows.dists) if rows.toi is None else (rows.pairs, rows.toi, rows.dists)
    return cols + (rows.faces.shape[0], rc, mi355cd.Witness(rows.faces, rows.points, rows.bary, rows.feature))


def same_witness(got, want: wr.Rows, what=""):
    """got: the tuple of cd_find_proximity_witness / cd_find_ccd_witness or of their between-mesh forms; want: witness_ref's Rows.
    The return code, the count, then every column of the rows in (face a, face b) order by its bytes."""
    n, rc = got[-3], got[-2]
    assert rc == 0 and n == want.faces.shape[0], (what, rc, n, want.faces.shape[0])
    g = witness_rows(got)
    assert (g.toi is None) == (want.toi is None), what
    for k in wr.Rows._fields:
        if getattr(want, k) is not None:
            _same_bytes(getattr(g, k), getattr(want, k), (what, k))


def contour_rows(got, tested=None) -> ir.Rows:
    """A contour call's (pairs, n, rc, Contour) as isect_ref's Rows, sorted by (face a, face b)."""
    pairs, _, _, con = got
    n = con.faces.shape[0]
    return ir.Rows(*ir.sort_got(con.faces, pairs, con.code, con.param.reshape(n, 6), con.points.reshape(n, 6)), tested)


def contour_call(rows: ir.Rows, rc=0):
    """What a contour call that found `rows` returns."""
    return rows.pairs, rows.faces.shape[0], rc, mi355cd.Contour(rows.faces, rows.code, rows.param.reshape(-1, 2, 3), rows.points.reshape(-1, 2, 3))


def same_contour(got, want: ir.Rows, what="", tested=None):
    """got: cd_find_collisions_contour's / cd_find_collisions_between_contour's tuple; want: isect_ref's Rows; tested: the call's
    n_tested, compared with the restatement's where the restatement has one."""
    assert got[2] == 0 and got[1] == want.faces.shape[0], (what, got[2], got[1], want.faces.shape[0])
    g = contour_rows(got)
    for k in ("faces", "pairs", "code", "param", "points"):
        _same_bytes(getattr(g, k), getattr(want, k), (what, k))
    if tested is not None and want.tested is not None:
        assert tested == want.tested, (what, tested, want.tested)


def item_rows(got):
    """The tuple of cd_points_within / cd_cast_rays_all / cd_sweep_points_all / cd_boxes_overlap_all / cd_planes_cut_all /
    cd_segments_within / cd_sweep_segments_all -- (rows, values ..., n, rc) -- as within_ref's PointRows / RayRows, sweep_ref's SweepRows,
    box_ref's BoxRows, plane_ref's PlaneRows, segment_ref's SegRows or swept_segment_ref's SweepSegRows (told apart by their number of
    columns), sorted by (item, face); the call fitted its capacity."""
    *cols, n, rc = got
    assert rc == 0 and n == cols[0].shape[0], (rc, n, cols[0].shape[0])
    return ROW_KINDS[len(cols)](*wn.sort_rows(*cols))


ROW_KINDS = {len(t._fields): t for t in (wn.PointRows, wn.RayRows, sw.SweepRows, bx.BoxRows, plr.PlaneRows, sg.SegRows, ssr.SweepSegRows)}
assert len(ROW_KINDS) == 7


def item_call(rows, rc=0):
    """What an all-results call that found `rows` returns."""
    return tuple(rows) + (rows.rows.shape[0], rc)


def same_item_rows(got, want, what=""):
    """got: an all-results call's tuple; want: the restatement's rows (or item_rows of another call).  The return code, the count, the
    set of (item, face), then every column of the rows in that order bit for bit (within_ref.same_rows)."""
    n, rc = got[-2], got[-1]
    assert rc == 0 and n == want.rows.shape[0] == got[0].shape[0], (what, rc, n, want.rows.shape[0], got[0].shape[0])
    assert len(got) - 2 == len(want), what
    wn.same_rows(got[:-2], want, what)


def first_contact_call(rows: sw.SweepRows, n):
    """What cd_sweep_points returns on n items whose rows are `rows`."""
    first = sw.first_of(rows, n)
    return first + (mi355cd.CdPointInfo(int((first[0] != sw.NONE).sum()), 0, 0),)


def same_first_contact(got, rows: sw.SweepRows, n, what=""):
    """got: cd_sweep_points' (face, ids, toi, dist, closest, uv, feature, side, info); rows: the restatement's rows of the same n items.
    All eight outputs are sweep_ref.first_of of the rows, by their bytes, and n_found is the number of items with a row."""
    want = sw.first_of(rows, n)
    for k, (a, b) in enumerate(zip(got[:8], want)):
        _same_bytes(a, b, (what, "first contact, output", k))
    found = int(np.unique(rows.rows[:, 0]).size)
    assert got[8].n_found == found, (what, got[8].n_found, found)


def box_count_call(rows: bx.BoxRows, n, any=False):
    """What cd_boxes_count (with any: CD_BOX_ANY) returns on n boxes whose rows are `rows`."""
    c, ci = bx.counts_of(rows, n)
    info = mi355cd.CdBoxInfo(int((c > 0).sum()), 0, 0)
    return ((c > 0).astype(np.uint32), None, info) if any else (c, ci, info)


def same_box_counts(got, rows: bx.BoxRows, n, what="", any=False):
    """got: cd_boxes_count's (count, n_inside, info); rows: the rows of the same n boxes.  count and n_inside are the per-item sums of
    the rows (with any: count is "has a row" and n_inside None), n_found the boxes with a row.  node_visits and tri_tests: not compared."""
    c, ci = bx.counts_of(rows, n)
    if any:
        assert got[1] is None, what
        _same_bytes(got[0], (c > 0).astype(np.uint32), (what, "any"))
    else:
        _same_bytes(got[0], c, (what, "count"))
        _same_bytes(got[1], ci, (what, "n_inside"))
    assert got[2].n_found == int((c > 0).sum()), (what, got[2].n_found, int((c > 0).sum()))


def plane_count_call(cls):
    """What cd_planes_count returns on planes whose classes are `cls`."""
    c = plr.counts_of_classes(cls)
    return c + (mi355cd.CdPlaneInfo(int((c[0] > 0).sum()), 0, 0),)


def same_plane_counts(got, cls, what=""):
    """got: cd_planes_count's (n_cut, n_below, n_above, info); cls: plane_ref.classes_ref of the same planes.  The three counts are
    counts_of_classes, they add up to the number of faces, n_found is the planes that cut a face."""
    want = plr.counts_of_classes(cls)
    for k, a, b in zip(("n_cut", "n_below", "n_above"), got[:3], want):
        _same_bytes(a, b, (what, k))
    assert (got[0].astype(np.int64) + got[1] + got[2] == cls.shape[1]).all(), what
    assert got[3].n_found == int((want[0] > 0).sum()), (what, got[3].n_found)


def segment_closest_call(rows: sg.SegRows, n):
    """What cd_segments_closest returns on n segments whose rows are `rows`."""
    first = sg.closest_of(rows, n)
    return first + (mi355cd.CdSegmentInfo(int((first[0] != sg.NONE).sum()), 0, 0),)


def same_segment_closest(got, rows: sg.SegRows, n, what=""):
    """got: cd_segments_closest's (face, ids, dist, s, on_seg, on_tri, uv, feature, end, cross, side, info); rows: rows of the same n
    segments.  All eleven outputs are segment_ref.closest_of of the rows, by their bytes; n_found is the segments with a row."""
    for k, (a, b) in enumerate(zip(got[:11], sg.closest_of(rows, n))):
        _same_bytes(a, b, (what, "closest, output", k))
    found = int(np.unique(rows.rows[:, 0]).size)
    assert got[11].n_found == found, (what, got[11].n_found, found)


def same_segment_any(face, info, rows: sg.SegRows, n, what=""):
    """CD_SEGMENT_ANY: WHETHER a segment has a row is defined, and the face returned is one of its rows'."""
    has = wn.rows_per_item(rows, n) > 0
    assert np.array_equal(face != sg.NONE, has) and info.n_found == int(has.sum()), (what, info.n_found, int(has.sum()))
    key = lambda r: (r[:, 0].astype(np.uint64) << np.uint64(32)) | r[:, 1].astype(np.uint64)
    k = np.flatnonzero(has)
    assert np.isin(key(np.stack([k.astype(np.uint32), face[k]], axis=1)), key(rows.rows)).all(), what


def sweep_segments_call(rows: ssr.SweepSegRows, n):
    """What cd_sweep_segments returns on n items whose rows are `rows`."""
    first = ssr.first_of(rows, n)
    return first + (mi355cd.CdPointInfo(int((first[0] != ssr.NONE).sum()), 0, 0),)


def same_sweep_segments(got, rows: ssr.SweepSegRows, n, what=""):
    """got: cd_sweep_segments' (face, ids, toi, dist, s, on_seg, on_tri, uv, feature, end, cross, side, info); rows: rows of the same n
    items.  All twelve outputs are swept_segment_ref.first_of of the rows, by their bytes; n_found is the items with a row."""
    for k, (a, b) in enumerate(zip(got[:12], ssr.first_of(rows, n))):
        _same_bytes(a, b, (what, "first contact, output", k))
    found = int(np.unique(rows.rows[:, 0]).size)
    assert got[12].n_found == found, (what, got[12].n_found, found)


def unordered_pairs(pairs):
    """oracle.pair_set of the pairs as (smaller ID, larger ID)."""
    p = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    return oracle.pair_set(np.stack([p.min(axis=1), p.max(axis=1)], axis=1))


def same_pair_set(pairs, want_pairs, what=""):
    """The contour call's pairs against the collision step's: one set."""
    assert np.array_equal(unordered_pairs(pairs), unordered_pairs(want_pairs)), what


def nearest_call(rows: nr.NearestRows):
    """What cd_nearest_between with a witness returns for `rows`."""
    found = int((rows.faces[:, 0] != nr.NONE).sum())
    return mi355cd.Nearest(rows.faces, rows.ids, rows.dist, mi355cd.Witness(rows.faces, rows.points, rows.bary, rows.feature), mi355cd.CdNearestInfo(found, 0, 0))


def same_nearest(got, want: nr.NearestRows, what=""):
    """got: a Nearest with its witness (rows in a's face order, or the one row of CD_NEAREST_MIN); want: nearest_ref's NearestRows."""
    w = got.witness
    for k, x, y in (("faces", got.faces, want.faces), ("ids", got.ids, want.ids), ("dist", got.dist, want.dist), ("witness faces", w.faces, want.faces),
                    ("points", w.points, want.points), ("bary", w.bary, want.bary), ("feature", w.feature, want.feature)):
        _same_bytes(x, y, (what, k))
    found = int((want.faces[:, 0] != nr.NONE).sum())
    assert got.info.n_found == found, (what, got.info.n_found, found)


def nearest_self_call(res):
    """What cd_nearest_self with a witness returns for (rows, played faces)."""
    rows, played = res
    found = int((rows.faces[:, 0] != nr.NONE).sum())
    return mi355cd.Nearest(rows.faces, rows.ids, rows.dist, mi355cd.Witness(played, rows.points, rows.bary, rows.feature), mi355cd.CdNearestInfo(found, 0, 0))


def same_nearest_self(got, want, what=""):
    """got: cd_nearest_self's Nearest with its witness; want: nearest_self_ref's (NearestRows, played faces).  test_nearest_self_gpu.py's
    _same: faces, IDs, the bits of dist, played faces, points, barycentrics, features and n_found (that module imports this one, so
    it is imported at the first call)."""
    from test_nearest_self_gpu import _same
    _same(got, want, what)


def inside_call(want):
    """What cd_points_inside returns for the restatement's five arrays."""
    return tuple(want) + (mi355cd.CdInsideInfo(int(np.asarray(want[0]).sum()), 0, 0),)


# ---------------------------------------------------------------- between two meshes
BETWEEN_FRAMES = 6
APART = "both_move_apart"
BETWEEN_SCHEDULES = ("a_moves", "b_moves", "both_move", APART)
BETWEEN_DIST = SLIDE_QUAD[0] / 4
BETWEEN_CCD_DIST = SLIDE_QUAD[0] / 10
NEAREST_R = 2 * SLIDE_QUAD[0]   # cd_nearest_between's radii: NEAREST_R and a quarter of it; +inf for CD_NEAREST_MIN
# APART: sheet b lifted along y, the direction the sheets' heights are measured in, by another amount every frame: enough to clear
# sheet a where the two are placed in that frame, and little enough to leave them within BETWEEN_CCD_DIST of each other, so that the
# proximity and CCD queries still find pairs (tests/test_moving_inputs.py pins the separation distances: 0.004 to 0.009)
APART_LIFT = (0.025, 0.032, 0.036, 0.030, 0.022, 0.034)
APART_INF_FRAMES = (1, 2)       # the frames whose per-triangle rows at rmax = +inf are restated over all a x b pairs, roles (a, b) only


@functools.lru_cache(maxsize=None)
def between_meshes():
    """The two sheets of `slide` as meshes of their own: (va, ia, vb, ib), each with 0-based vertex indices."""
    v, i = _slide_base()
    half, na = v.shape[0] // 2, i.shape[0] // 2
    assert i[:na].max() < half and i[na:].min() >= half
    return np.ascontiguousarray(v[:half]), np.ascontiguousarray(i[:na]), np.ascontiguousarray(v[half:]), np.ascontiguousarray((i[na:] - half).astype(np.uint32))


def _lifted(v, dy):
    w = v.copy()
    w[:, 1] = np.float32(w[:, 1] + np.float32(dy))
    return w


def between_place(schedule, f):
    """Where the sheets are in frame f: (a's quads along x, b's quads along z, b's lift along y).  a slides along x, b along z, one quad
    a frame (0, 1, 2, 1, 0, 1: inside the reference's frame), whichever the schedule moves.  Every reference of a frame is a function
    of this alone (the schedules and frames that share a place share its references)."""
    at = 2 - abs(2 - f % 4)
    return (at if schedule != "b_moves" else 0, at if schedule != "a_moves" else 0, APART_LIFT[f] if schedule == APART else 0.0)


@functools.lru_cache(maxsize=None)
def _placed(place):
    va, ia, vb, ib = between_meshes()
    qa, qb, lift = place
    wb = _shifted(vb, 0, qb)
    return _shifted(va, qa, 0), _lifted(wb, lift) if lift else wb


@functools.lru_cache(maxsize=None)
def between_positions(schedule):
    """Per frame (va, vb, a moved, b moved)."""
    out = []
    for f in range(BETWEEN_FRAMES):
        wa, wb = _placed(between_place(schedule, f))
        out.append((wa, wb, f > 0 and schedule != "b_moves", f > 0 and schedule != "a_moves"))
    return out


@functools.lru_cache(maxsize=None)
def _x1_placed(place):
    wa, wb = _placed(place)
    return br.motion(wa, 0.15 * SLIDE_QUAD[0], 11), br.motion(wb, 0.15 * SLIDE_QUAD[0], 12)


def between_x1(schedule, f):
    return _x1_placed(between_place(schedule, f))


def between_x1_moving(schedule, f):
    """between_x1 with None for the mesh the schedule never moves (a static obstacle: cd_find_ccd_between's NULL end positions)."""
    ea, eb = between_x1(schedule, f)
    return None if schedule == "b_moves" else ea, None if schedule == "a_moves" else eb


def _roles(place, swap):
    """(va, ia, ea, vb, ib, eb) of the place in the roles (a, b), or (b, a) with swap."""
    wa, wb = _placed(place)
    _, ia, _, ib = between_meshes()
    ea, eb = _x1_placed(place)
    return (wb, ib, eb, wa, ia, ea) if swap else (wa, ia, ea, wb, ib, eb)


@functools.lru_cache(maxsize=None)
def _want_plain_between(place, swap):
    wa, ia, ea, wb, ib, eb = _roles(place, swap)
    return dict(contact=br.contact_pairs(wa, ia, wb, ib, brute=False), prox=br.proximity_pairs(wa, ia, wb, ib, BETWEEN_DIST, brute=False),
                ccd=br.ccd_pairs(wa, ia, wb, ib, BETWEEN_CCD_DIST, ea, eb, brute=False))       # (the grid's candidates: 1.3 M pairs otherwise)


@functools.lru_cache(maxsize=None)
def _want_rows_between(place, swap):
    wa, ia, ea, wb, ib, eb = _roles(place, swap)
    near = nr.rows_of_all_pairs(wa, ia, wb, ib, rmax=NEAREST_R)
    near_q = nr.within(near, NEAREST_R / 4)
    return dict(prox_witness=wr.witness_pairs_between(wa, ia, wb, ib, BETWEEN_DIST), contour=ir.contour_pairs_between(wa, ia, wb, ib),
                near=near, near_q=near_q, near_min=nr.nearest_min(near), near_q_min=nr.nearest_min(near_q))


@functools.lru_cache(maxsize=None)
def _want_ccd_witness_between(place, swap, a_ends, b_ends):
    wa, ia, ea, wb, ib, eb = _roles(place, swap)
    return wr.witness_pairs_between(wa, ia, wb, ib, BETWEEN_CCD_DIST, ccd=True, va1=ea if a_ends else None, vb1=eb if b_ends else None)


@functools.lru_cache(maxsize=None)
def want_between(schedule, f, swap=False):
    """The references of frame f in the roles (a, b), or (b, a) with swap.  contact, prox, ccd: between_ref's pairs (CCD with both
    meshes moving to between_x1).  prox_witness, ccd_witness: witness_ref's Rows (CCD to between_x1_moving: None for a mesh the
    schedule does not move).  contour: isect_ref's Rows.  near, near_q: nearest_ref's rows at NEAREST_R and a quarter of it, near_min,
    near_q_min: their CD_NEAREST_MIN row; near_min is the row at rmax = +inf too wherever `near` finds anything."""
    place = between_place(schedule, f)
    ea, eb = between_x1_moving(schedule, f)
    ends = (eb is not None, ea is not None) if swap else (ea is not None, eb is not None)
    return dict(_want_plain_between(place, swap), **_want_rows_between(place, swap), ccd_witness=_want_ccd_witness_between(place, swap, *ends))


@functools.lru_cache(maxsize=None)
def want_between_inf(f):
    """APART's per-triangle rows of frame f at rmax = +inf, roles (a, b): nearest_ref.nearest_rows, every a x b pair."""
    assert f in APART_INF_FRAMES
    wa, ia, _, wb, ib, _ = _roles(between_place(APART, f), False)
    return nr.nearest_rows(wa, ia, wb, ib, np.inf)
