"""ctypes binding of libmi355cd.so (include/mi355cd.h) -- plumbing for tests/ and bench.py.

This is NOT a second implementation: every method is one call through the C ABI.  There is no CPU
fallback; if the shared library is missing or no HIP device is present the constructor raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libmi355cd.so")

CD_OK, CD_OVERFLOW = 0, 1
CD_ERR_ARG, CD_ERR_ORDER, CD_ERR_NO_DEVICE, CD_ERR_INDEX = -1001, -1002, -1003, -1004
CD_FRAME_REFERENCE, CD_FRAME_AUTO, CD_FRAME_CUSTOM = 0, 1, 2
CD_ERR_SORT, CD_ERR_IO, CD_ERR_FORMAT = -1005, -1006, -1007
CD_OPT_TRAVERSAL, CD_OPT_QUERIES_PER_WAVE, CD_OPT_SORT_FULL, CD_OPT_STAGE_TIMING, CD_OPT_KERNEL_STAMPS, CD_OPT_GRAPH, CD_OPT_POLL = 0, 1, 2, 3, 4, 5, 6
CD_OPT_CELL_TABLE = 7
CD_OPT_ORDER_HINT = 8
# cd_debug_option keys (measurement hooks / test switches; not part of the mirrored interface)
CD_DBG_LDS_PAD, CD_DBG_EXACT_BLOCKS, CD_DBG_NO_SHARED_PATH, CD_DBG_DIAG, CD_DBG_STAGEWISE_BUILD, CD_DBG_SPLIT_CROSS = 0, 1, 2, 3, 4, 5
CD_DBG_SORT_WINDOWS, CD_DBG_GET_SORT_FORM = 7, 8
CD_DBG_POLL_SCAN, CD_DBG_GET_POLL_STALE, CD_DBG_GET_POLL_FALLBACKS, CD_DBG_GET_POLLED_STEPS, CD_DBG_GET_TREE_WAS_FUSED = 10, 11, 12, 13, 14
CD_DBG_GET_ORDER_STATE = 15
CD_DBG_GET_POLL_FB_WHY, CD_DBG_GET_POLL_MAX_WAIT_US = 16, 17
CD_DBG_REPORT_COPIES = 6
CD_DBG_STORE_QBOX = 9
CD_DBG_BIG_OFFSETS = 18
CD_DBG_GET_GRAPH_CAPTURES, CD_DBG_GET_GRAPH_REPLAYS = 19, 20
CD_DBG_SORT_CELLS, CD_DBG_GET_SORT_CELLS, CD_DBG_GET_CELL_STAT = 21, 22, 23

QUERY_DTYPE = np.dtype([("v", "<f8", (9,)), ("id", "<u4"), ("vidx", "<u4", (3,))])
assert QUERY_DTYPE.itemsize == 88


class CdStats(C.Structure):
    _fields_ = [("ms_morton", C.c_float), ("ms_sort", C.c_float), ("ms_hierarchy", C.c_float),
                ("ms_refit", C.c_float), ("ms_traverse", C.c_float), ("ms_check", C.c_float),
                ("traverse_launches", C.c_uint32), ("stack_overflows", C.c_uint32),
                ("n_pairs", C.c_uint64), ("pairs_tested", C.c_uint64), ("node_visits", C.c_uint64),
                ("wave_steps", C.c_uint64), ("candidates", C.c_uint64),
                ("ms_descend", C.c_float), ("ms_exact", C.c_float), ("sort_passes", C.c_uint32), ("ms_pipeline", C.c_float),
                ("ms_build_block", C.c_float), ("ms_descend_clock", C.c_float)]


# every symbol include/mi355cd.h declares (tests check the library exports exactly these)
CD_MULTI_SELF_PEER, CD_MULTI_TIMING, CD_MULTI_SELF_SLICE, CD_MULTI_CROSS_SERIAL, CD_MULTI_INJECT_FAILURE, CD_MULTI_PRIORITY_STREAM = 1, 2, 4, 8, 16, 32
CD_MULTI_INJECT_ALLOC_FAILURE = 64
CD_ERR_RCCL, CD_ERR_PEER, CD_ERR_INJECTED = -1008, -1009, -1010


class CdCcdInfo(C.Structure):
    _fields_ = [("n_candidates", C.c_uint64), ("n_tested", C.c_uint64), ("n_evals", C.c_uint64), ("n_unresolved", C.c_uint64)]


class CdRayInfo(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64)]


CD_RAY_ANY = 1
RAY_MISS = 0xFFFFFFFF


class CdPointInfo(C.Structure):
    _fields_ = [("n_found", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64)]


CD_POINT_ANY = 1
POINT_NONE = 0xFFFFFFFF


class CdPointRows(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("dist", C.c_void_p), ("closest", C.c_void_p), ("uv", C.c_void_p), ("feature", C.c_void_p), ("side", C.c_void_p)]


class CdRayRows(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("t", C.c_void_p), ("uv", C.c_void_p), ("side", C.c_void_p)]


WITHIN_SHARD_FIRST = 1 << 14        # cd_within.h: candidates a shard in the first allocation of the all-results item queries
WITHIN_SHARDS = 64                  # cd_traverse.h NSHARD


class _PointRowArrays:
    """The arrays of a points_within call with room for cap rows, and the cd_point_rows that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.ids = np.empty(n, dtype=np.uint32)
        self.dist = np.empty(n, dtype=np.float64)
        self.closest = np.empty((n, 3), dtype=np.float64)
        self.uv = np.empty((n, 2), dtype=np.float64)
        self.feature = np.empty(n, dtype=np.uint8)
        self.side = np.empty(n, dtype=np.uint8)
        self.out = CdPointRows(self.ids.ctypes.data, self.dist.ctypes.data, self.closest.ctypes.data, self.uv.ctypes.data, self.feature.ctypes.data,
                               self.side.ctypes.data)

    def take(self, got):
        return tuple(a[:got].copy() for a in (self.ids, self.dist, self.closest, self.uv, self.feature, self.side))


class _RayRowArrays:
    """The arrays of a cast_rays_all call with room for cap rows, and the cd_ray_rows that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.ids = np.empty(n, dtype=np.uint32)
        self.t = np.empty(n, dtype=np.float64)
        self.uv = np.empty((n, 2), dtype=np.float64)
        self.side = np.empty(n, dtype=np.uint8)
        self.out = CdRayRows(self.ids.ctypes.data, self.t.ctypes.data, self.uv.ctypes.data, self.side.ctypes.data)

    def take(self, got):
        return tuple(a[:got].copy() for a in (self.ids, self.t, self.uv, self.side))


class CdSweepRows(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("toi", C.c_void_p), ("dist", C.c_void_p), ("closest", C.c_void_p), ("uv", C.c_void_p), ("feature", C.c_void_p),
                ("side", C.c_void_p)]


SWEEP_NONE = 0xFFFFFFFF


class _SweepRowArrays:
    """The arrays of a sweep_points_all call with room for cap rows, and the cd_sweep_rows that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.ids = np.empty(n, dtype=np.uint32)
        self.toi = np.empty(n, dtype=np.float64)
        self.dist = np.empty(n, dtype=np.float64)
        self.closest = np.empty((n, 3), dtype=np.float64)
        self.uv = np.empty((n, 2), dtype=np.float64)
        self.feature = np.empty(n, dtype=np.uint8)
        self.side = np.empty(n, dtype=np.uint8)
        self.out = CdSweepRows(self.ids.ctypes.data, self.toi.ctypes.data, self.dist.ctypes.data, self.closest.ctypes.data, self.uv.ctypes.data,
                               self.feature.ctypes.data, self.side.ctypes.data)

    def take(self, got):
        return tuple(a[:got].copy() for a in (self.ids, self.toi, self.dist, self.closest, self.uv, self.feature, self.side))


class CdNearestInfo(C.Structure):
    _fields_ = [("n_found", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64)]


CD_NEAREST_MIN = 1
NEAREST_NONE = 0xFFFFFFFF


class CdInsideInfo(C.Structure):
    _fields_ = [("n_inside", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64)]


CD_INSIDE_PARITY = 1


class CdBoxInfo(C.Structure):
    _fields_ = [("n_found", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64)]


class CdBoxRows(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("inside", C.c_void_p)]


CD_BOX_ANY = 1


class _BoxRowArrays:
    """The arrays of a boxes_overlap_all call with room for cap rows, and the cd_box_rows that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.ids = np.empty(n, dtype=np.uint32)
        self.inside = np.empty(n, dtype=np.uint8)
        self.out = CdBoxRows(self.ids.ctypes.data, self.inside.ctypes.data)

    def take(self, got):
        return tuple(a[:got].copy() for a in (self.ids, self.inside))


class CdPlaneInfo(C.Structure):
    _fields_ = [("n_found", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64)]


class CdPlaneRows(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("seg", C.c_void_p), ("edge", C.c_void_p), ("t", C.c_void_p), ("on", C.c_void_p)]


CD_PLANE_ABOVE, CD_PLANE_BELOW, CD_PLANE_CUT = 0, 1, 2
CD_PLANE_SLAB = 256                 # mi355cd.h: leaves of the tree a lane of the plane queries walks (tests/test_planes_abi.py compares)


class _PlaneRowArrays:
    """The arrays of a planes_cut_all call with room for cap rows, and the cd_plane_rows that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.ids = np.empty(n, dtype=np.uint32)
        self.seg = np.empty((n, 2, 3), dtype=np.float64)
        self.edge = np.empty((n, 2), dtype=np.uint8)
        self.t = np.empty((n, 2), dtype=np.float64)
        self.on = np.empty(n, dtype=np.uint8)
        self.out = CdPlaneRows(self.ids.ctypes.data, self.seg.ctypes.data, self.edge.ctypes.data, self.t.ctypes.data, self.on.ctypes.data)

    def take(self, got):
        return tuple(a[:got].copy() for a in (self.ids, self.seg, self.edge, self.t, self.on))


class CdSegmentInfo(C.Structure):
    _fields_ = [("n_found", C.c_uint64), ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64)]


class CdSegmentRows(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("dist", C.c_void_p), ("s", C.c_void_p), ("on_seg", C.c_void_p), ("on_tri", C.c_void_p), ("uv", C.c_void_p),
                ("feature", C.c_void_p), ("end", C.c_void_p), ("cross", C.c_void_p), ("side", C.c_void_p)]


CD_SEGMENT_ANY = 1
SEGMENT_NONE = 0xFFFFFFFF


class _SegmentRowArrays:
    """The arrays of a segments_within / segments_closest call with room for cap rows, and the cd_segment_rows that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.ids = np.empty(n, dtype=np.uint32)
        self.dist = np.empty(n, dtype=np.float64)
        self.s = np.empty(n, dtype=np.float64)
        self.on_seg = np.empty((n, 3), dtype=np.float64)
        self.on_tri = np.empty((n, 3), dtype=np.float64)
        self.uv = np.empty((n, 2), dtype=np.float64)
        self.feature, self.end, self.cross, self.side = (np.empty(n, dtype=np.uint8) for _ in range(4))
        self.out = CdSegmentRows(*(a.ctypes.data for a in self._all()))

    def _all(self):
        return (self.ids, self.dist, self.s, self.on_seg, self.on_tri, self.uv, self.feature, self.end, self.cross, self.side)

    def take(self, got):
        return tuple(a[:got].copy() for a in self._all())


class CdSweepSegmentRows(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("toi", C.c_void_p), ("dist", C.c_void_p), ("s", C.c_void_p), ("on_seg", C.c_void_p), ("on_tri", C.c_void_p),
                ("uv", C.c_void_p), ("feature", C.c_void_p), ("end", C.c_void_p), ("cross", C.c_void_p), ("side", C.c_void_p)]


class _SweepSegmentRowArrays:
    """The arrays of a sweep_segments_all / sweep_segments call with room for cap rows, and the cd_sweep_segment_rows that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.ids = np.empty(n, dtype=np.uint32)
        self.toi = np.empty(n, dtype=np.float64)
        self.dist = np.empty(n, dtype=np.float64)
        self.s = np.empty(n, dtype=np.float64)
        self.on_seg = np.empty((n, 3), dtype=np.float64)
        self.on_tri = np.empty((n, 3), dtype=np.float64)
        self.uv = np.empty((n, 2), dtype=np.float64)
        self.feature, self.end, self.cross, self.side = (np.empty(n, dtype=np.uint8) for _ in range(4))
        self.out = CdSweepSegmentRows(*(a.ctypes.data for a in self._all()))

    def _all(self):
        return (self.ids, self.toi, self.dist, self.s, self.on_seg, self.on_tri, self.uv, self.feature, self.end, self.cross, self.side)

    def take(self, got):
        return tuple(a[:got].copy() for a in self._all())


class Nearest(collections.namedtuple("Nearest", "faces ids dist witness info")):
    """cd_nearest_between's rows: faces u32[n, 2] (face of self, face of other; NEAREST_NONE twice when nothing is within rmax),
    ids u32[n, 2], dist f64[n] (+inf then), witness (a Witness over the same rows, or None), info (CdNearestInfo)."""
    __slots__ = ()


class CdWitnessOut(C.Structure):
    _fields_ = [("faces", C.c_void_p), ("points", C.c_void_p), ("bary", C.c_void_p), ("feature", C.c_void_p)]


FEATURE_NONE = 7                    # tri_witness: a pair in contact (or six coincident points) has no closest points


class Witness(collections.namedtuple("Witness", "faces points bary feature")):
    """Where the distances of the reported pairs are attained (cd_witness_out), row k for pairs[k]: faces u32[n, 2] (indices in the
    face list of the triangles that played A and B), points f64[n, 2, 3] (qa, qb), bary f64[n, 2, 2] ((ua, va), (ub, vb)),
    feature u8[n, 2] (0 face, 1-3 edge 01 / 12 / 20, 4-6 vertex 0 / 1 / 2, 7 none: the pair is in contact)."""
    __slots__ = ()


class _WitnessArrays:
    """The four arrays of a witness call with room for cap rows, and the cd_witness_out that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.faces = np.empty((n, 2), dtype=np.uint32)
        self.points = np.empty((n, 2, 3), dtype=np.float64)
        self.bary = np.empty((n, 2, 2), dtype=np.float64)
        self.feature = np.empty((n, 2), dtype=np.uint8)
        self.out = CdWitnessOut(self.faces.ctypes.data, self.points.ctypes.data, self.bary.ctypes.data, self.feature.ctypes.data)

    def take(self, got):
        return Witness(self.faces[:got].copy(), self.points[:got].copy(), self.bary[:got].copy(), self.feature[:got].copy())


class CdContourOut(C.Structure):
    _fields_ = [("faces", C.c_void_p), ("code", C.c_void_p), ("param", C.c_void_p), ("points", C.c_void_p)]


TERM_NONE = 7                       # tri_isect: a missing endpoint (fewer than two of the six edge-against-face terms hit)


class Contour(collections.namedtuple("Contour", "faces code param points")):
    """The intersection segments of the reported pairs (cd_contour_out), row k for pairs[k]: faces u32[n, 2] (indices in the face list of
    the triangles that played A and B), code u8[n, 3] (endpoint 0 and 1 as term | side << 3, 7 = missing; the mask of the terms that
    hit: 0-2 A's edges 01 / 12 / 20 against B's face, 3-5 B's edges against A's face), param f64[n, 2, 3] ((t, u, v) of the two
    endpoints: t along the piercing edge, (u, v) on the pierced face), points f64[n, 2, 3]."""
    __slots__ = ()

    @property
    def term(self):
        """u8[n, 2]: the term of each endpoint (7: missing)."""
        return self.code[:, :2] & 7

    @property
    def side(self):
        """u8[n, 2]: 1 where the piercing edge meets the face that runs counter-clockwise as seen from the edge's start."""
        return self.code[:, :2] >> 3

    @property
    def mask(self):
        return self.code[:, 2]


class _ContourArrays:
    """The four arrays of a contour call with room for cap rows, and the cd_contour_out that points at them."""

    def __init__(self, cap):
        n = max(cap, 1)
        self.faces = np.empty((n, 2), dtype=np.uint32)
        self.code = np.empty((n, 3), dtype=np.uint8)
        self.param = np.empty((n, 2, 3), dtype=np.float64)
        self.points = np.empty((n, 2, 3), dtype=np.float64)
        self.out = CdContourOut(self.faces.ctypes.data, self.code.ctypes.data, self.param.ctypes.data, self.points.ctypes.data)

    def take(self, got):
        return Contour(self.faces[:got].copy(), self.code[:got].copy(), self.param[:got].copy(), self.points[:got].copy())


class CdMultiInfo(C.Structure):
    _fields_ = [("world", C.c_uint32), ("rank", C.c_uint32), ("n_peers", C.c_uint32), ("host_syncs", C.c_uint32), ("attempts", C.c_uint32),
                ("failed_rank_plus1", C.c_uint32), ("sent_queries", C.c_uint64), ("recv_queries", C.c_uint64), ("local_pairs", C.c_uint64),
                ("cross_pairs", C.c_uint64), ("pairs_tested", C.c_uint64), ("query_cap", C.c_uint64),
                ("ms_tree", C.c_float), ("ms_allgather", C.c_float), ("ms_pack", C.c_float), ("ms_counts", C.c_float),
                ("ms_exchange", C.c_float), ("ms_local", C.c_float), ("ms_cross", C.c_float), ("pad1", C.c_float)]


EXPORTS = [
    "cd_load_obj", "cd_free_obj", "cd_create", "cd_destroy", "cd_update_vertices", "cd_set_morton_frame", "cd_get_morton_frame", "cd_set_morton_frame_layout", "cd_morton_sort",
    "cd_build_hierarchy", "cd_refit_boxes", "cd_check_internal", "cd_check_leaves",
    "cd_check_triangle_idx", "cd_find_collisions", "cd_build_tree", "cd_self_collide", "cd_sorted_pairs", "cd_collision_triangles", "cd_brute_force",
    "cd_test_pairs", "cd_export_keys", "cd_export_tree", "cd_get_stats", "cd_debug_counters", "cd_debug_records", "cd_debug_swept", "cd_num_triangles",
    "cd_set_option", "cd_set_vertex_id_base", "cd_root_box", "cd_pack_queries", "cd_find_collisions_queries", "cd_version",
    "cd_debug_option", "cd_debug_hint", "cd_debug_hint_set", "cd_morton3d_points", "cd_morton3d_points_layout", "cd_expand64_values", "cd_box_pairs", "cd_tri_contact_points", "cd_alloc_host_pairs", "cd_free_host_pairs",
    "cd_multi_unique_id", "cd_multi_create", "cd_multi_create_from_comm", "cd_multi_destroy", "cd_multi_set_flags", "cd_multi_step",
    "cd_find_proximity", "cd_self_proximity", "cd_tri_distance_points",
    "cd_find_ccd", "cd_self_ccd", "cd_ccd_points",
    "cd_find_collisions_between", "cd_find_proximity_between", "cd_find_ccd_between",
    "cd_cast_rays", "cd_ray_tri_points",
    "cd_closest_points", "cd_pt_tri_points",
    "cd_find_proximity_witness", "cd_find_proximity_between_witness", "cd_find_ccd_witness", "cd_find_ccd_between_witness", "cd_tri_witness_points",
    "cd_find_collisions_contour", "cd_find_collisions_between_contour", "cd_tri_isect_points",
    "cd_nearest_between", "cd_nearest_self",
    "cd_points_within", "cd_cast_rays_all",
    "cd_sweep_points_all", "cd_sweep_points", "cd_pt_advance_points",
    "cd_points_inside", "cd_signed_distance", "cd_column_tri_points",
    "cd_boxes_overlap_all", "cd_boxes_count", "cd_box_tri_points",
    "cd_planes_cut_all", "cd_planes_count", "cd_plane_tri_points",
    "cd_segments_within", "cd_segments_closest", "cd_seg_tri_points",
    "cd_sweep_segments_all", "cd_sweep_segments", "cd_seg_advance_points",
]

_lib = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    global _lib
    if _lib is None:
        # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 (same sonames as /opt/rocm's).  Two HIP
        # runtimes in one process do not work -- the second one finds no GPU -- so when torch is installed its copy is
        # loaded first and serves this library too.  (Plumbing only: nothing here computes with torch.)
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if _lib is not None:
        return _lib
    path = os.environ.get("MI355CD_LIB", path)          # A/B runs of two builds (tools/)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not built: run __graft_entry__.build() (there is no CPU fallback)")
    lib = C.CDLL(path)
    vp, u32p, u64p, i32p, dp = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lib.cd_load_obj.argtypes = [C.c_char_p, C.POINTER(dp), u32p, C.POINTER(u32p), u32p, C.c_int]
    lib.cd_free_obj.argtypes = [dp, u32p]
    lib.cd_free_obj.restype = None
    lib.cd_create.argtypes = [C.POINTER(vp), vp, C.c_uint32, vp, vp, C.c_uint32]
    lib.cd_destroy.argtypes = [vp]
    lib.cd_destroy.restype = None
    lib.cd_update_vertices.argtypes = [vp, vp]
    lib.cd_set_morton_frame.argtypes = [vp, C.c_int, vp, vp]
    lib.cd_get_morton_frame.argtypes = [vp, vp, vp, u64p]
    lib.cd_set_morton_frame_layout.argtypes = [vp, vp, vp, C.c_uint64]
    lib.cd_morton_sort.argtypes = [vp]
    lib.cd_build_hierarchy.argtypes = [vp, u32p]
    lib.cd_refit_boxes.argtypes = [vp]
    lib.cd_check_internal.argtypes = [vp, vp]
    lib.cd_check_leaves.argtypes = [vp, vp]
    lib.cd_check_triangle_idx.argtypes = [vp, C.c_uint32, u32p]
    lib.cd_find_collisions.argtypes = [vp, vp, C.c_uint64, u64p]
    lib.cd_build_tree.argtypes = [vp]
    lib.cd_self_collide.argtypes = [vp, vp, C.c_uint64, u64p]
    lib.cd_sorted_pairs.argtypes = [vp, vp, C.c_uint64, u64p]
    lib.cd_collision_triangles.argtypes = [vp, vp, C.c_uint64, u64p]
    lib.cd_brute_force.argtypes = [vp, C.c_int, vp, C.c_uint64, u64p]
    lib.cd_test_pairs.argtypes = [vp, vp, C.c_uint64, vp]
    lib.cd_export_keys.argtypes = [vp, vp, vp]
    lib.cd_export_tree.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.cd_get_stats.argtypes = [vp, C.POINTER(CdStats)]
    lib.cd_debug_counters.argtypes = [vp, vp]
    lib.cd_debug_records.argtypes = [vp, vp, vp, vp]
    lib.cd_debug_swept.argtypes = [vp, C.c_int, vp, vp, u32p, C.POINTER(C.c_float), u32p]
    lib.cd_debug_hint.argtypes = [vp, vp, vp, vp]
    lib.cd_debug_hint_set.argtypes = [vp, vp]
    lib.cd_num_triangles.argtypes = [vp, u32p]
    lib.cd_set_option.argtypes = [vp, C.c_int, C.c_int64]
    lib.cd_set_vertex_id_base.argtypes = [vp, C.c_uint32]
    lib.cd_root_box.argtypes = [vp, vp]
    lib.cd_pack_queries.argtypes = [vp, vp, vp, C.c_uint64, u64p]
    lib.cd_find_collisions_queries.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p]
    lib.cd_version.restype = C.c_char_p
    lib.cd_alloc_host_pairs.argtypes = [C.c_uint64, C.POINTER(u32p)]
    lib.cd_free_host_pairs.argtypes = [u32p]
    lib.cd_free_host_pairs.restype = None
    lib.cd_morton3d_points.argtypes = [vp, C.c_uint64, vp, vp, vp]
    lib.cd_morton3d_points_layout.argtypes = [vp, C.c_uint64, vp, vp, C.c_uint64, vp]
    lib.cd_expand64_values.argtypes = [vp, C.c_uint64, vp]
    lib.cd_debug_option.argtypes = [vp, C.c_int, C.c_int64, C.POINTER(C.c_int64)]
    lib.cd_box_pairs.argtypes = [vp, vp, C.c_uint64, vp, vp]
    lib.cd_tri_contact_points.argtypes = [vp, C.c_uint64, vp]
    lib.cd_find_proximity.argtypes = [vp, C.c_double, vp, vp, C.c_uint64, u64p, u64p]
    lib.cd_self_proximity.argtypes = [vp, C.c_double, vp, vp, C.c_uint64, u64p, u64p]
    lib.cd_tri_distance_points.argtypes = [vp, C.c_uint64, vp]
    lib.cd_find_ccd.argtypes = [vp, vp, C.c_double, vp, vp, vp, C.c_uint64, u64p, vp]
    lib.cd_self_ccd.argtypes = [vp, vp, C.c_double, vp, vp, vp, C.c_uint64, u64p, vp]
    lib.cd_ccd_points.argtypes = [vp, C.c_uint64, C.c_double, vp, vp, vp]
    lib.cd_find_collisions_between.argtypes = [vp, vp, vp, C.c_uint64, u64p, u64p]
    lib.cd_find_proximity_between.argtypes = [vp, vp, C.c_double, vp, vp, C.c_uint64, u64p, u64p]
    lib.cd_find_ccd_between.argtypes = [vp, vp, vp, vp, C.c_double, vp, vp, vp, C.c_uint64, u64p, vp]
    lib.cd_cast_rays.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.cd_ray_tri_points.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp]
    lib.cd_closest_points.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cd_pt_tri_points.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, vp]
    wp = C.POINTER(CdWitnessOut)
    lib.cd_find_proximity_witness.argtypes = lib.cd_find_proximity.argtypes + [wp]
    lib.cd_find_proximity_between_witness.argtypes = lib.cd_find_proximity_between.argtypes + [wp]
    lib.cd_find_ccd_witness.argtypes = lib.cd_find_ccd.argtypes + [wp]
    lib.cd_find_ccd_between_witness.argtypes = lib.cd_find_ccd_between.argtypes + [wp]
    lib.cd_tri_witness_points.argtypes = [vp, C.c_uint64, vp, vp, vp, vp]
    cp = C.POINTER(CdContourOut)
    lib.cd_find_collisions_contour.argtypes = [vp, vp, C.c_uint64, u64p, u64p, cp]
    lib.cd_find_collisions_between_contour.argtypes = lib.cd_find_collisions_between.argtypes + [cp]
    lib.cd_tri_isect_points.argtypes = [vp, C.c_uint64, vp, vp, vp]
    lib.cd_nearest_between.argtypes = [vp, vp, C.c_double, C.c_int, vp, vp, vp, wp, C.POINTER(CdNearestInfo)]
    lib.cd_nearest_self.argtypes = [vp, C.c_double, C.c_int, vp, vp, vp, wp, C.POINTER(CdNearestInfo)]
    lib.cd_points_within.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, C.POINTER(CdPointRows)]
    lib.cd_cast_rays_all.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, C.POINTER(CdRayRows)]
    lib.cd_sweep_points_all.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, u64p, C.POINTER(CdSweepRows), C.POINTER(CdCcdInfo)]
    lib.cd_sweep_points.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(CdPointInfo)]
    lib.cd_pt_advance_points.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    lib.cd_points_inside.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.POINTER(CdInsideInfo)]
    lib.cd_signed_distance.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.POINTER(CdPointInfo)]
    lib.cd_column_tri_points.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, vp, vp, vp, vp]
    lib.cd_boxes_overlap_all.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, C.POINTER(CdBoxRows)]
    lib.cd_boxes_count.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, vp, C.POINTER(CdBoxInfo)]
    lib.cd_box_tri_points.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
    lib.cd_planes_cut_all.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, C.POINTER(CdPlaneRows)]
    lib.cd_planes_count.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.POINTER(CdPlaneInfo)]
    lib.cd_plane_tri_points.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, vp]
    lib.cd_segments_within.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, u64p, u64p, C.POINTER(CdSegmentRows)]
    lib.cd_segments_closest.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, C.POINTER(CdSegmentRows), C.POINTER(CdSegmentInfo)]
    lib.cd_seg_tri_points.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cd_sweep_segments_all.argtypes = [vp, vp, vp, C.c_uint64, vp, vp, C.c_uint64, u64p, C.POINTER(CdSweepSegmentRows), C.POINTER(CdCcdInfo)]
    lib.cd_sweep_segments.argtypes = [vp, vp, vp, C.c_uint64, vp, C.c_int, vp, C.POINTER(CdSweepSegmentRows), C.POINTER(CdPointInfo)]
    lib.cd_seg_advance_points.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.cd_multi_unique_id.argtypes = [vp]
    lib.cd_multi_create.argtypes = [C.POINTER(vp), vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_int]
    lib.cd_multi_create_from_comm.argtypes = [C.POINTER(vp), vp, vp, C.c_uint64, C.c_int]
    lib.cd_multi_destroy.argtypes = [vp]
    lib.cd_multi_destroy.restype = None
    lib.cd_multi_set_flags.argtypes = [vp, C.c_int]
    lib.cd_multi_step.argtypes = [vp, vp, C.c_uint64, u64p, C.POINTER(CdMultiInfo)]
    for name in EXPORTS:
        if name not in ("cd_destroy", "cd_version", "cd_free_obj", "cd_multi_destroy", "cd_free_host_pairs"):
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


class CdError(RuntimeError):
    def __init__(self, fn: str, rc: int):
        super().__init__(f"{fn} failed with status {rc}")
        self.rc = rc


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _verts_end(v, nv, what, optional=False):
    """The end positions of a CCD call as f64[nv, 3] (optional: None stays None, that mesh does not move)."""
    if v is None and optional:
        return None
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.shape != (nv, 3):
        raise ValueError(f"{what} must be [{nv}, 3], got {v.shape}")
    return v


class CollisionDetector:
    """One cd_ctx.  Methods mirror the reference harness's stage order (main.cu:64-146)."""

    def __init__(self, verts: np.ndarray, vidx: np.ndarray, ids: np.ndarray | None = None):
        self.lib = load_library()
        self.verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        self.vidx = np.ascontiguousarray(vidx, dtype=np.uint32).reshape(-1, 3)
        self.ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
        self.nv, self.nt = self.verts.shape[0], self.vidx.shape[0]
        self._ctx = C.c_void_p()
        rc = self.lib.cd_create(C.byref(self._ctx), _ptr(self.verts), self.nv, _ptr(self.vidx), _ptr(self.ids), self.nt)
        if rc != CD_OK:
            self._ctx = C.c_void_p()
            raise CdError("cd_create", rc)

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self.lib.cd_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, fn, rc, allow=(CD_OK,)):
        if rc not in allow:
            raise CdError(fn, rc)
        return rc

    # ---- stages
    def set_morton_frame(self, mode=CD_FRAME_REFERENCE, offset=None, span=None):
        off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64)
        sp = None if span is None else np.ascontiguousarray(span, dtype=np.float64)
        self._chk("cd_set_morton_frame", self.lib.cd_set_morton_frame(self._ctx, mode, _ptr(off), _ptr(sp)))

    def get_morton_frame(self):
        """(offset[3], span[3], layout word) of the frame the last sort used (cd_get_morton_frame)."""
        off = np.zeros(3, dtype=np.float64); sp = np.zeros(3, dtype=np.float64); lay = C.c_uint64(0)
        self._chk("cd_get_morton_frame", self.lib.cd_get_morton_frame(self._ctx, _ptr(off), _ptr(sp), C.byref(lay)))
        return off, sp, int(lay.value)

    def set_morton_frame_layout(self, offset, span, layout: int):
        off = np.ascontiguousarray(offset, dtype=np.float64); sp = np.ascontiguousarray(span, dtype=np.float64)
        self._chk("cd_set_morton_frame_layout", self.lib.cd_set_morton_frame_layout(self._ctx, _ptr(off), _ptr(sp), int(layout)))

    def keep_auto_frame(self):
        """The frame CD_FRAME_AUTO computed in the last sort becomes the context's fixed frame (the AUTO pass over the triangles leaves the step)."""
        off, sp, lay = self.get_morton_frame()
        self.set_morton_frame_layout(off, sp, lay)
        return off, sp, lay

    def set_option(self, key: int, value: int):
        self._chk("cd_set_option", self.lib.cd_set_option(self._ctx, key, value))

    def debug_set(self, key: int, value: int):
        self._chk("cd_debug_option", self.lib.cd_debug_option(self._ctx, key, value, None))

    def debug_get(self, key: int) -> int:
        out = C.c_int64(0)
        self._chk("cd_debug_option", self.lib.cd_debug_option(self._ctx, key, 0, C.byref(out)))
        return out.value

    def update_vertices(self, verts):
        v = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        assert v.shape[0] == self.nv
        self.verts = v
        self._chk("cd_update_vertices", self.lib.cd_update_vertices(self._ctx, _ptr(v)))

    def morton_sort(self):
        self._chk("cd_morton_sort", self.lib.cd_morton_sort(self._ctx))

    def build_hierarchy(self) -> int:
        w = C.c_uint32(0)
        self._chk("cd_build_hierarchy", self.lib.cd_build_hierarchy(self._ctx, C.byref(w)))
        return w.value

    def build_tree(self):
        self._chk("cd_build_tree", self.lib.cd_build_tree(self._ctx))

    def refit_boxes(self):
        self._chk("cd_refit_boxes", self.lib.cd_refit_boxes(self._ctx))

    def check_internal(self):
        out = np.zeros(5, dtype=np.uint32)
        self._chk("cd_check_internal", self.lib.cd_check_internal(self._ctx, _ptr(out)))
        return out

    def check_leaves(self):
        out = np.zeros(4, dtype=np.uint32)
        self._chk("cd_check_leaves", self.lib.cd_check_leaves(self._ctx, _ptr(out)))
        return out

    def check_triangle_idx(self, maxv: int) -> int:
        out = C.c_uint32(0)
        self._chk("cd_check_triangle_idx", self.lib.cd_check_triangle_idx(self._ctx, maxv, C.byref(out)))
        return out.value

    def _pairs_call(self, fn, name, cap, *pre, copy=True):
        n = C.c_uint64(0)
        # the output buffer is kept between calls (a 4 M-pair buffer is 32 MB; allocating it per step costs more
        # than the step); callers get a copy of the filled prefix -- or, with copy=False, a VIEW of the buffer the C
        # call wrote into, valid until the next call on this object (what a C caller has; a per-frame loop needs no more)
        buf = None
        if cap:
            if getattr(self, "_pairbuf", None) is None or self._pairbuf.shape[0] != cap:
                self._pairbuf = np.empty((cap, 2), dtype=np.uint32)
                self._pairptr = _ptr(self._pairbuf)
            buf = self._pairbuf
        rc = fn(self._ctx, *pre, self._pairptr if cap else None, cap, C.byref(n))
        self._chk(name, rc, allow=(CD_OK, CD_OVERFLOW))
        got = min(n.value, cap)
        if buf is None:
            return np.zeros((0, 2), dtype=np.uint32), n.value, rc
        return (buf[:got].copy() if copy else buf[:got]), n.value, rc

    def _pair_query(self, name, pre, cap, toi=False, dists=False, ccd=False, extra=None):
        """A pair query into fresh arrays: the C function `name` called as (*pre, pairs, [toi], [dists], cap, &n, &count, [&extra.out]),
        count being a CdCcdInfo (ccd) or n_tested; extra: a _WitnessArrays / _ContourArrays.  Returns (count, the public tuple): the
        arrays the call has clipped to min(n, cap) and copied, n, rc, and extra's rows."""
        arrays = [np.empty((max(cap, 1), 2), dtype=np.uint32)] + [np.empty(max(cap, 1), dtype=np.float64) for has in (toi, dists) if has]
        n, count = C.c_uint64(0), CdCcdInfo() if ccd else C.c_uint64(0)
        last = () if extra is None else (C.byref(extra.out),)
        rc = getattr(self.lib, name)(*pre, _ptr(arrays[0]) if cap else None, *map(_ptr, arrays[1:]), cap, C.byref(n), C.byref(count), *last)
        self._chk(name, rc, allow=(CD_OK, CD_OVERFLOW))
        got = min(n.value, cap)
        out = [a[:got].copy() for a in arrays] + [n.value, rc] + ([] if extra is None else [extra.take(got)])
        return (count if ccd else count.value), tuple(out)

    def find_proximity(self, dist: float, cap: int = 1 << 20):
        """cd_find_proximity on the tree that is there: (pairs[n, 2] (smaller ID, larger ID), dists[n], n, rc); n may exceed cap
        (rc = CD_OVERFLOW, the first cap pairs are returned).  self.proximity_tested: exact distance evaluations made."""
        self.proximity_tested, out = self._pair_query("cd_find_proximity", (self._ctx, float(dist)), cap, dists=True)
        return out

    def self_proximity(self, dist: float, cap: int = 1 << 20):
        """cd_self_proximity: build the tree, then find_proximity, with one host synchronisation."""
        self.proximity_tested, out = self._pair_query("cd_self_proximity", (self._ctx, float(dist)), cap, dists=True)
        return out

    def find_proximity_witness(self, dist: float, cap: int = 1 << 20):
        """cd_find_proximity_witness: find_proximity's (pairs, dists, n, rc) and a Witness whose row k says where dists[k] is attained."""
        self.proximity_tested, out = self._pair_query("cd_find_proximity_witness", (self._ctx, float(dist)), cap, dists=True, extra=_WitnessArrays(cap))
        return out

    def find_ccd_witness(self, verts_end, dist: float, cap: int = 1 << 20):
        """cd_find_ccd_witness: find_ccd's (pairs, toi, dists, n, rc) and a Witness taken at the evaluation that reported each pair."""
        pre = (self._ctx, _ptr(_verts_end(verts_end, self.nv, "verts_end")), float(dist))
        self.ccd_info, out = self._pair_query("cd_find_ccd_witness", pre, cap, toi=True, dists=True, ccd=True, extra=_WitnessArrays(cap))
        return out

    def find_proximity_between_witness(self, other, dist: float, cap: int = 1 << 20):
        """cd_find_proximity_between_witness: find_proximity_between's (pairs, dists, n, rc) and a Witness (A: self's triangle; faces
        index each context's own face list)."""
        pre = (self._ctx, other._ctx, float(dist))
        self.between_tested, out = self._pair_query("cd_find_proximity_between_witness", pre, cap, dists=True, extra=_WitnessArrays(cap))
        return out

    def find_ccd_between_witness(self, other, dist: float, verts_end=None, other_verts_end=None, cap: int = 1 << 20):
        """cd_find_ccd_between_witness: find_ccd_between's (pairs, toi, dists, n, rc) and a Witness."""
        pre = self._ccd_between_pre(other, dist, verts_end, other_verts_end)
        self.ccd_info, out = self._pair_query("cd_find_ccd_between_witness", pre, cap, toi=True, dists=True, ccd=True, extra=_WitnessArrays(cap))
        return out

    def find_ccd(self, verts_end, dist: float, cap: int = 1 << 20):
        """cd_find_ccd on the tree that is there, the vertices moving linearly to verts_end: (pairs[n, 2] (smaller ID, larger ID),
        toi[n], dists[n], n, rc); n may exceed cap (rc = CD_OVERFLOW, the first cap pairs are returned).  A returned distance > dist
        marks a pair left unresolved.  self.ccd_info: candidates, pairs through the gate, evaluations, unresolved pairs."""
        pre = (self._ctx, _ptr(_verts_end(verts_end, self.nv, "verts_end")), float(dist))
        self.ccd_info, out = self._pair_query("cd_find_ccd", pre, cap, toi=True, dists=True, ccd=True)
        return out

    def self_ccd(self, verts_end, dist: float, cap: int = 1 << 20):
        """cd_self_ccd: build the tree on the current vertices, then find_ccd, with one host synchronisation."""
        pre = (self._ctx, _ptr(_verts_end(verts_end, self.nv, "verts_end")), float(dist))
        self.ccd_info, out = self._pair_query("cd_self_ccd", pre, cap, toi=True, dists=True, ccd=True)
        return out

    # ---- queries between this mesh (a) and another context's (b): pairs (ID in self, ID in other), self's triangle first
    def find_collisions_contour(self, cap: int = 1 << 20):
        """cd_find_collisions_contour: (pairs[n, 2] (smaller ID, larger ID), n, rc, Contour) -- find_collisions' pair set from a pass of
        its own, and per pair the segment the two triangles cut each other in.  self.contour_tested: pairs that reached tri_contact.  The
        tree must be built from the current vertices."""
        self.contour_tested, out = self._pair_query("cd_find_collisions_contour", (self._ctx,), cap, extra=_ContourArrays(cap))
        return out

    def find_collisions_between_contour(self, other, cap: int = 1 << 20):
        """cd_find_collisions_between_contour: find_collisions_between's (pairs, n, rc) and a Contour (A: self's triangle; faces index each
        context's own face list)."""
        self.between_tested, out = self._pair_query("cd_find_collisions_between_contour", (self._ctx, other._ctx), cap, extra=_ContourArrays(cap))
        return out

    def find_collisions_between(self, other, cap: int = 1 << 20):
        """cd_find_collisions_between(self, other): (pairs[n, 2] (ID in self, ID in other), n, rc); n may exceed cap (rc = CD_OVERFLOW,
        the first cap pairs are returned).  self.between_tested: pairs whose FP64 boxes overlap strictly.  Both trees must be built."""
        self.between_tested, out = self._pair_query("cd_find_collisions_between", (self._ctx, other._ctx), cap)
        return out

    def find_proximity_between(self, other, dist: float, cap: int = 1 << 20):
        """cd_find_proximity_between(self, other, dist): (pairs[n, 2] (ID in self, ID in other), dists[n], n, rc).
        self.between_tested: exact distance evaluations made."""
        self.between_tested, out = self._pair_query("cd_find_proximity_between", (self._ctx, other._ctx, float(dist)), cap, dists=True)
        return out

    def _ccd_between_pre(self, other, dist, verts_end, other_verts_end):
        va = _verts_end(verts_end, self.nv, "verts_end", optional=True)
        vb = _verts_end(other_verts_end, other.nv, "other_verts_end", optional=True)
        return self._ctx, _ptr(va), other._ctx, _ptr(vb), float(dist)

    def find_ccd_between(self, other, dist: float, verts_end=None, other_verts_end=None, cap: int = 1 << 20):
        """cd_find_ccd_between: self's vertices move to verts_end, other's to other_verts_end (None: that mesh does not move):
        (pairs[n, 2] (ID in self, ID in other), toi[n], dists[n], n, rc).  self.ccd_info: as find_ccd's."""
        pre = self._ccd_between_pre(other, dist, verts_end, other_verts_end)
        self.ccd_info, out = self._pair_query("cd_find_ccd_between", pre, cap, toi=True, dists=True, ccd=True)
        return out

    # ---- ray queries against this mesh (cd_cast_rays)
    def cast_rays(self, origins, dirs, tmax=np.inf, any_hit: bool = False):
        """cd_cast_rays on the tree that is there.  origins, dirs: [n, 3]; tmax: a scalar or [n] (t is in units of dirs, which are not
        normalised; the range is [0, tmax]).  Closest hit: (face[n] (index into the face list, RAY_MISS = 0xFFFFFFFF for a miss),
        ids[n], t[n] (+inf for a miss), uv[n, 2], side[n], info) -- of the triangles ray_tri hits, the smallest (t, ID, face index).
        any_hit: (face[n], info); face is RAY_MISS or SOME hit triangle -- which one is not defined, whether there is one is.
        Rays are walked in the order given: keep coherent rays next to each other."""
        rays = pack_rays(origins, dirs, tmax)
        n = rays.shape[0]
        face = np.empty(n, dtype=np.uint32)
        info = CdRayInfo()
        if any_hit:
            rc = self.lib.cd_cast_rays(self._ctx, _ptr(rays), n, CD_RAY_ANY, _ptr(face), None, None, None, None, C.byref(info))
            self._chk("cd_cast_rays", rc)
            return face, info
        ids = np.empty(n, dtype=np.uint32)
        t = np.empty(n, dtype=np.float64)
        uv = np.empty((n, 2), dtype=np.float64)
        side = np.empty(n, dtype=np.uint8)
        rc = self.lib.cd_cast_rays(self._ctx, _ptr(rays), n, 0, _ptr(face), _ptr(ids), _ptr(t), _ptr(uv), _ptr(side), C.byref(info))
        self._chk("cd_cast_rays", rc)
        return face, ids, t, uv, side, info

    # ---- closest-point queries against this mesh (cd_closest_points)
    def closest_points(self, points, rmax=np.inf, any_within: bool = False):
        """cd_closest_points on the tree that is there.  points: [n, 3]; rmax: a scalar or [n], the search radius (+inf: the nearest
        triangle wherever it is).  -> (face[n] (index into the face list, POINT_NONE = 0xFFFFFFFF when nothing is within rmax), ids[n],
        dist[n] (+inf then), closest[n, 3], uv[n, 2], feature[n] (0 face, 1-3 edge 01 / 12 / 20, 4-6 vertex 0 / 1 / 2), side[n], info)
        -- of the triangles with pt_tri's dist <= rmax, the smallest (dist, ID, face index).  side is the side of that triangle's
        plane, not an inside / outside test.  any_within: (face[n], info); face is POINT_NONE or SOME triangle within rmax -- which
        one is not defined, whether there is one is.
        Projecting mesh a's vertices onto mesh b is  b.closest_points(a_verts): closest is the projection, (face, uv) where it lies.
        Points are walked in the order given: keep spatially coherent points next to each other."""
        pts = pack_points(points, rmax)
        n = pts.shape[0]
        face = np.empty(n, dtype=np.uint32)
        info = CdPointInfo()
        if any_within:
            rc = self.lib.cd_closest_points(self._ctx, _ptr(pts), n, CD_POINT_ANY, _ptr(face), None, None, None, None, None, None, C.byref(info))
            self._chk("cd_closest_points", rc)
            return face, info
        ids = np.empty(n, dtype=np.uint32)
        dist = np.empty(n, dtype=np.float64)
        closest = np.empty((n, 3), dtype=np.float64)
        uv = np.empty((n, 2), dtype=np.float64)
        feature = np.empty(n, dtype=np.uint8)
        side = np.empty(n, dtype=np.uint8)
        rc = self.lib.cd_closest_points(self._ctx, _ptr(pts), n, 0, _ptr(face), _ptr(ids), _ptr(dist), _ptr(closest), _ptr(uv), _ptr(feature), _ptr(side),
                                        C.byref(info))
        self._chk("cd_closest_points", rc)
        return face, ids, dist, closest, uv, feature, side, info

    # ---- all-results item queries against this mesh (cd_points_within, cd_cast_rays_all)
    def points_within(self, points, rmax, cap: int = 1 << 20):
        """cd_points_within on the tree that is there.  points: [n, 3]; rmax: a scalar or [n].  -> (rows[n, 2] (point index, face index),
        ids[n], dist[n], closest[n, 3], uv[n, 2], feature[n], side[n], n, rc): one row for EVERY (point, triangle) with pt_tri's
        dist <= rmax, with pt_tri's values; n may exceed cap (rc = CD_OVERFLOW, cap rows are returned).  The vertex-face pairs of a
        repulsion pass are  b.points_within(a_verts, thickness).  The rows come in no order; grouped by point, nearest first:
            o = np.lexsort((rows[:, 1], ids, dist, rows[:, 0]))
        whose first row a point is closest_points' answer.  self.within_tested: pt_tri evaluations made.  Points are walked in the
        order given: keep spatially coherent points next to each other; a point with rmax = +inf walks the whole tree in one lane."""
        pts = pack_points(points, rmax)
        self.within_tested, (rows, n, rc, vals) = self._pair_query("cd_points_within", (self._ctx, _ptr(pts), pts.shape[0]), cap, extra=_PointRowArrays(cap))
        return (rows, *vals, n, rc)

    def cast_rays_all(self, origins, dirs, tmax=np.inf, cap: int = 1 << 20):
        """cd_cast_rays_all on the tree that is there.  origins, dirs, tmax: as cast_rays takes them.  -> (rows[n, 2] (ray index, face
        index), ids[n], t[n], uv[n, 2], side[n], n, rc): one row for EVERY (ray, triangle) that ray_tri hits over [0, tmax], with
        ray_tri's values; n may exceed cap (rc = CD_OVERFLOW, cap rows are returned).  The rows come in no order; grouped by ray, in
        the order the ray meets them:
            o = np.lexsort((rows[:, 1], ids, t, rows[:, 0]))
        whose first row a ray is cast_rays' closest hit.  self.rays_all_tested: ray_tri evaluations made."""
        rays = pack_rays(origins, dirs, tmax)
        self.rays_all_tested, (rows, n, rc, vals) = self._pair_query("cd_cast_rays_all", (self._ctx, _ptr(rays), rays.shape[0]), cap, extra=_RayRowArrays(cap))
        return (rows, *vals, n, rc)

    # ---- swept-point queries against this mesh as it moves (cd_sweep_points_all, cd_sweep_points)
    def _sweep_pre(self, p0, p1, dist, verts_end, skip_vertex):
        items = pack_sweeps(p0, p1, dist)
        n = items.shape[0]
        x1 = _verts_end(verts_end, self.nv, "verts_end", optional=True)
        skip = None
        if skip_vertex is not None:
            skip = np.ascontiguousarray(skip_vertex, dtype=np.uint32).reshape(-1)
            if skip.shape[0] != n:
                raise ValueError(f"skip_vertex must be [{n}], got {skip.shape}")
        return items, n, x1, skip

    def sweep_points_all(self, p0, p1, dist, verts_end=None, skip_vertex=None, cap: int = 1 << 20):
        """cd_sweep_points_all on the tree that is there.  p0, p1: [n, 3], the points at the start and the end of the step; dist: a scalar
        or [n], finite and > 0; verts_end: [nv, 3], the mesh at the end of the step (None: it does not move); skip_vertex: [n] vertex
        indices (SWEEP_NONE = 0xFFFFFFFF: none) whose triangles are not tested for that item.  -> (rows[n, 2] (item index, face index),
        ids[n], toi[n], dist[n], closest[n, 3], uv[n, 2], feature[n], side[n], n, rc): one row for EVERY (item, triangle) the
        advancement reports, with toi and pt_tri's values of the reporting evaluation; n may exceed cap (rc = CD_OVERFLOW, cap rows are
        returned).  A row with dist > the item's dist is unresolved.  self.sweep_info (CdCcdInfo): candidates, pairs through the gate,
        pt_tri evaluations, unresolved rows.  The vertex-face half of a cloth's own CCD pass is
            cd.sweep_points_all(x0, x1, thickness, verts_end=x1, skip_vertex=np.arange(nv))."""
        items, n, x1, skip = self._sweep_pre(p0, p1, dist, verts_end, skip_vertex)
        rows = np.empty((max(cap, 1), 2), dtype=np.uint32)
        arrays = _SweepRowArrays(cap)
        nrows, info = C.c_uint64(0), CdCcdInfo()
        rc = self.lib.cd_sweep_points_all(self._ctx, _ptr(x1), _ptr(items), n, _ptr(skip), _ptr(rows) if cap else None, cap, C.byref(nrows), C.byref(arrays.out),
                                          C.byref(info))
        self._chk("cd_sweep_points_all", rc, allow=(CD_OK, CD_OVERFLOW))
        self.sweep_info = info
        got = min(nrows.value, cap)
        return (rows[:got].copy(), *arrays.take(got), nrows.value, rc)

    def sweep_points(self, p0, p1, dist, verts_end=None, skip_vertex=None):
        """cd_sweep_points on the tree that is there; arguments as sweep_points_all takes them.  -> (face[n] (SWEEP_NONE = 0xFFFFFFFF: the
        point comes within dist of no triangle), ids[n], toi[n] (+inf then), dist[n], closest[n, 3], uv[n, 2], feature[n], side[n], info):
        per item the row of sweep_points_all with the smallest (toi, ID, face index)."""
        items, n, x1, skip = self._sweep_pre(p0, p1, dist, verts_end, skip_vertex)
        face = np.empty(n, dtype=np.uint32)
        ids = np.empty(n, dtype=np.uint32)
        toi = np.empty(n, dtype=np.float64)
        d = np.empty(n, dtype=np.float64)
        closest = np.empty((n, 3), dtype=np.float64)
        uv = np.empty((n, 2), dtype=np.float64)
        feature = np.empty(n, dtype=np.uint8)
        side = np.empty(n, dtype=np.uint8)
        info = CdPointInfo()
        rc = self.lib.cd_sweep_points(self._ctx, _ptr(x1), _ptr(items), n, _ptr(skip), 0, _ptr(face), _ptr(ids), _ptr(toi), _ptr(d), _ptr(closest), _ptr(uv),
                                      _ptr(feature), _ptr(side), C.byref(info))
        self._chk("cd_sweep_points", rc)
        return face, ids, toi, d, closest, uv, feature, side, info

    # ---- nearest triangle of another mesh, and the separation distance (cd_nearest_between)
    def nearest_between(self, other, rmax=np.inf, minimum: bool = False, witness: bool = False):
        """cd_nearest_between on the two trees that are there, self as a.  -> Nearest(faces, ids, dist, witness, info): one row per
        triangle of self in face-list order -- of other's triangles with tri_distance <= rmax the smallest (dist, ID, face index) --
        or, with minimum, the ONE row of the separation distance: the smallest (dist, ID a, face a, ID b, face b) over all pairs.
        Nothing within rmax: faces NEAREST_NONE, dist +inf, everything else 0.  witness: a Witness of the rows' pairs (else None)."""
        n = 1 if minimum else self.nt
        faces = np.empty((n, 2), dtype=np.uint32)
        ids = np.empty((n, 2), dtype=np.uint32)
        dist = np.empty(n, dtype=np.float64)
        wa = _WitnessArrays(n) if witness else None
        info = CdNearestInfo()
        rc = self.lib.cd_nearest_between(self._ctx, other._ctx, float(rmax), CD_NEAREST_MIN if minimum else 0, _ptr(faces), _ptr(ids), _ptr(dist),
                                         C.byref(wa.out) if witness else None, C.byref(info))
        self._chk("cd_nearest_between", rc)
        return Nearest(faces, ids, dist, wa.take(n) if witness else None, info)

    # ---- nearest non-neighbouring triangle of the mesh itself, and its clearance (cd_nearest_self)
    def nearest_self(self, rmax=np.inf, minimum: bool = False, witness: bool = False):
        """cd_nearest_self on the tree that is there.  -> Nearest(faces, ids, dist, witness, info): one row per triangle in face-list
        order -- of the triangles that share no vertex index with it and have tri_distance <= rmax the smallest (dist, ID, face index);
        the pair's distance is cd_find_proximity's, bit for bit -- or, with minimum, the ONE row of the mesh's clearance: the smallest
        (dist, own ID, own face, partner ID, partner face).  Nothing within rmax: faces NEAREST_NONE, dist +inf, everything else 0.
        witness: a Witness of the rows' pairs (else None); its faces are the ones that played A and B, not (own, partner)."""
        n = 1 if minimum else self.nt
        faces = np.empty((n, 2), dtype=np.uint32)
        ids = np.empty((n, 2), dtype=np.uint32)
        dist = np.empty(n, dtype=np.float64)
        wa = _WitnessArrays(n) if witness else None
        info = CdNearestInfo()
        rc = self.lib.cd_nearest_self(self._ctx, float(rmax), CD_NEAREST_MIN if minimum else 0, _ptr(faces), _ptr(ids), _ptr(dist),
                                      C.byref(wa.out) if witness else None, C.byref(info))
        self._chk("cd_nearest_self", rc)
        return Nearest(faces, ids, dist, wa.take(n) if witness else None, info)

    # ---- inside / outside and signed distance for points (cd_points_inside, cd_signed_distance)
    def points_inside(self, points, axis: int = 2, parity: bool = False):
        """cd_points_inside on the tree that is there.  points: [n, 3]; axis: the direction of the line through each point along which
        the surface's crossings are counted.  -> (inside[n] (bool), n_above[n], n_below[n], w_above[n], w_below[n], info): the faces
        that cover the point above / below it along the axis, each crossing owned by exactly one face, and the sums of their
        orientations.  inside = w_above != 0 (the winding number), or with parity n_above odd.  On a closed, consistently oriented
        mesh w_above + w_below == 0; a point where it is not had a hole or an open mesh on its line.  A contained object that
        find_collisions_between cannot see:  body.points_inside(object_verts).all().
        Points are walked in the order given, each along its whole line: keep spatially coherent points next to each other."""
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        n = pts.shape[0]
        inside = np.empty(n, dtype=np.uint8)
        n_above = np.empty(n, dtype=np.uint32)
        n_below = np.empty(n, dtype=np.uint32)
        w_above = np.empty(n, dtype=np.int32)
        w_below = np.empty(n, dtype=np.int32)
        info = CdInsideInfo()
        rc = self.lib.cd_points_inside(self._ctx, _ptr(pts), n, int(axis), CD_INSIDE_PARITY if parity else 0, _ptr(inside), _ptr(n_above), _ptr(n_below),
                                       _ptr(w_above), _ptr(w_below), C.byref(info))
        self._chk("cd_points_inside", rc)
        return inside.astype(bool), n_above, n_below, w_above, w_below, info

    def signed_distance(self, points, axis: int = 2, parity: bool = False):
        """cd_signed_distance on the tree that is there.  points: [n, 3].  -> (sdist[n], face[n], ids[n], closest[n, 3], uv[n, 2],
        feature[n], inside[n] (bool), info): closest_points' nearest triangle for every point with the distance negated where
        points_inside(points, axis, parity) says inside (a distance of 0 stays +0); closest is the push-out target."""
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
        n = pts.shape[0]
        sdist = np.empty(n, dtype=np.float64)
        face = np.empty(n, dtype=np.uint32)
        ids = np.empty(n, dtype=np.uint32)
        closest = np.empty((n, 3), dtype=np.float64)
        uv = np.empty((n, 2), dtype=np.float64)
        feature = np.empty(n, dtype=np.uint8)
        inside = np.empty(n, dtype=np.uint8)
        info = CdPointInfo()
        rc = self.lib.cd_signed_distance(self._ctx, _ptr(pts), n, int(axis), CD_INSIDE_PARITY if parity else 0, _ptr(sdist), _ptr(face), _ptr(ids),
                                         _ptr(closest), _ptr(uv), _ptr(feature), _ptr(inside), C.byref(info))
        self._chk("cd_signed_distance", rc)
        return sdist, face, ids, closest, uv, feature, inside.astype(bool), info

    # ---- box queries against this mesh (cd_boxes_overlap_all, cd_boxes_count)
    def boxes_overlap_all(self, lo, hi, cap: int = 1 << 20):
        """cd_boxes_overlap_all on the tree that is there.  lo, hi: [n, 3], the closed boxes [lo, hi].  -> (rows[n, 2] (box index, face
        index), ids[n], inside[n] (bool), n, rc): one row for EVERY (box, triangle) that box_tri hits -- the triangle meets the closed
        box; inside: all three of its vertices lie in it.  n may exceed cap (rc = CD_OVERFLOW, cap rows are returned).  The rows come
        in no order.  self.boxes_tested: box_tri evaluations made.  Boxes are walked in the order given: keep spatially coherent boxes
        next to each other; a box around the whole mesh walks the whole tree in one lane (boxes_count does not)."""
        boxes = pack_boxes(lo, hi)
        self.boxes_tested, (rows, n, rc, vals) = self._pair_query("cd_boxes_overlap_all", (self._ctx, _ptr(boxes), boxes.shape[0]), cap, extra=_BoxRowArrays(cap))
        return (rows, vals[0], vals[1].astype(bool), n, rc)

    def boxes_count(self, lo, hi, any: bool = False):
        """cd_boxes_count on the tree that is there.  lo, hi: [n, 3].  -> (count[n], n_inside[n], info): the number of rows each box has
        in boxes_overlap_all and the number of those with inside; with any, count is 0 / 1 (the box meets a triangle: an occupancy
        grid is one box a voxel) and n_inside is None.  info: CdBoxInfo (boxes with count > 0, boxes tested, box_tri evaluations).
        A subtree that lies inside the box is counted without being walked."""
        boxes = pack_boxes(lo, hi)
        n = boxes.shape[0]
        count = np.empty(n, dtype=np.uint32)
        n_inside = None if any else np.empty(n, dtype=np.uint32)
        info = CdBoxInfo()
        rc = self.lib.cd_boxes_count(self._ctx, _ptr(boxes), n, CD_BOX_ANY if any else 0, _ptr(count), _ptr(n_inside), C.byref(info))
        self._chk("cd_boxes_count", rc)
        return count, n_inside, info

    # ---- plane queries against this mesh (cd_planes_cut_all, cd_planes_count)
    def planes_cut_all(self, normals, d, cap: int = 1 << 20):
        """cd_planes_cut_all on the tree that is there.  normals: [n, 3], d: [n], the planes normal . x = d.  -> (rows[m, 2] (plane
        index, face index), ids[m], seg[m, 2, 3] (a, b), edge[m, 2], t[m, 2], on[m], m, rc): one row for EVERY (plane, triangle) that
        plane_tri classes CUT -- some but not all of its vertices lie below the plane -- with the segment a -> b along which the plane
        cuts it.  On a closed outward mesh the segments of a plane are closed loops, counter-clockwise seen from the normal's tip, and
        the a are the b bit for bit.  m may exceed cap (rc = CD_OVERFLOW, cap rows are returned).  The rows come in no order.
        self.planes_tested: plane_tri evaluations made.  One plane is walked by many lanes (CD_PLANE_SLAB leaves each)."""
        planes = pack_planes(normals, d)
        self.planes_tested, (rows, n, rc, vals) = self._pair_query("cd_planes_cut_all", (self._ctx, _ptr(planes), planes.shape[0]), cap, extra=_PlaneRowArrays(cap))
        return (rows, *vals, n, rc)

    def planes_count(self, normals, d):
        """cd_planes_count on the tree that is there.  -> (n_cut[n], n_below[n], n_above[n], info): per plane the number of rows it has
        in planes_cut_all, the faces wholly below it and the faces with no vertex below it; the three add up to the number of faces.
        info: CdPlaneInfo (planes with n_cut > 0, boxes tested, plane_tri evaluations).  A subtree on one side of the plane is
        counted without being walked."""
        planes = pack_planes(normals, d)
        n = planes.shape[0]
        n_cut, n_below, n_above = (np.empty(n, dtype=np.uint32) for _ in range(3))
        info = CdPlaneInfo()
        rc = self.lib.cd_planes_count(self._ctx, _ptr(planes), n, _ptr(n_cut), _ptr(n_below), _ptr(n_above), C.byref(info))
        self._chk("cd_planes_count", rc)
        return n_cut, n_below, n_above, info

    # ---- segment queries against this mesh (cd_segments_within, cd_segments_closest)
    def segments_within(self, a, b, r, cap: int = 1 << 20):
        """cd_segments_within on the tree that is there.  a, b: [n, 3], the segments' ends (a == b: a point); r: a scalar or [n], the
        radius.  -> (rows[m, 2] (segment index, face index), ids[m], dist[m], s[m], on_seg[m, 3], on_tri[m, 3], uv[m, 2], feature[m],
        end[m], cross[m], side[m], m, rc): one row for EVERY (segment, triangle) with seg_tri's dist <= r, with seg_tri's values --
        the closest points on the segment (at parameter s; end 1 / 2: it is a / b) and on the triangle (uv, feature as pt_tri's);
        cross = 1: the segment crosses the face (dist 0, the points are the crossing).  m may exceed cap (rc = CD_OVERFLOW, cap rows
        are returned).  The edge-edge and edge-face pairs of a repulsion pass are  b.segments_within(a_verts[e[:, 0]], a_verts[e[:, 1]],
        thickness).  The rows come in no order; grouped by segment, nearest first:
            o = np.lexsort((rows[:, 1], ids, dist, rows[:, 0]))
        whose first row a segment is segments_closest's answer.  self.segments_tested: seg_tri evaluations made.  Segments are walked
        in the order given: keep spatially coherent ones next to each other; one with r = +inf walks the whole tree in one lane."""
        segs = pack_segments(a, b, r)
        self.segments_tested, (rows, n, rc, vals) = self._pair_query("cd_segments_within", (self._ctx, _ptr(segs), segs.shape[0]), cap, extra=_SegmentRowArrays(cap))
        return (rows, *vals, n, rc)

    def segments_closest(self, a, b, rmax=np.inf, any_within: bool = False):
        """cd_segments_closest on the tree that is there.  a, b: [n, 3]; rmax: a scalar or [n], the search radius.  -> (face[n]
        (SEGMENT_NONE = 0xFFFFFFFF when nothing is within rmax), ids[n], dist[n] (+inf then), s[n], on_seg[n, 3], on_tri[n, 3],
        uv[n, 2], feature[n], end[n], cross[n], side[n], info): of the triangles with seg_tri's dist <= rmax the smallest (dist, ID,
        face index) -- the smallest row of segments_within, bit for bit.  any_within: (face[n], info); face is SEGMENT_NONE or SOME
        triangle within rmax -- which one is not defined, whether there is one is."""
        segs = pack_segments(a, b, rmax)
        n = segs.shape[0]
        face = np.empty(n, dtype=np.uint32)
        info = CdSegmentInfo()
        if any_within:
            rc = self.lib.cd_segments_closest(self._ctx, _ptr(segs), n, CD_SEGMENT_ANY, _ptr(face), None, C.byref(info))
            self._chk("cd_segments_closest", rc)
            return face, info
        arrays = _SegmentRowArrays(n)
        rc = self.lib.cd_segments_closest(self._ctx, _ptr(segs), n, 0, _ptr(face), C.byref(arrays.out), C.byref(info))
        self._chk("cd_segments_closest", rc)
        return (face, *arrays.take(n), info)

    # ---- swept-segment queries against this mesh as it moves (cd_sweep_segments_all, cd_sweep_segments)
    def _sweep_segments_pre(self, a0, b0, a1, b1, dist, verts_end, skip_vertices):
        items = pack_swept_segments(a0, b0, a1, b1, dist)
        n = items.shape[0]
        x1 = _verts_end(verts_end, self.nv, "verts_end", optional=True)
        skip = None
        if skip_vertices is not None:
            skip = np.ascontiguousarray(skip_vertices, dtype=np.uint32)
            if skip.shape != (n, 2):
                raise ValueError(f"skip_vertices must be [{n}, 2], got {skip.shape}")
        return items, n, x1, skip

    def sweep_segments_all(self, a0, b0, a1, b1, dist, verts_end=None, skip_vertices=None, cap: int = 1 << 20):
        """cd_sweep_segments_all on the tree that is there.  a0, b0, a1, b1: [n, 3], the segments' two ends at the start and at the end
        of the step (a0 == b0 and a1 == b1: a moving point); dist: a scalar or [n], finite and > 0; verts_end: [nv, 3], the mesh at
        the end of the step (None: it does not move); skip_vertices: [n, 2] vertex indices (SWEEP_NONE = 0xFFFFFFFF: none) whose
        triangles are not tested for that item.  -> (rows[m, 2] (item index, face index), ids[m], toi[m], dist[m], s[m], on_seg[m, 3],
        on_tri[m, 3], uv[m, 2], feature[m], end[m], cross[m], side[m], m, rc): one row for EVERY (item, triangle) the advancement
        reports, with toi and seg_tri's values of the reporting evaluation; m may exceed cap (rc = CD_OVERFLOW, cap rows are
        returned).  A row with dist > the item's dist is unresolved.  self.sweep_segments_info (CdCcdInfo): candidates, pairs through
        the gate, seg_tri evaluations, unresolved rows.  The edge-edge half of a cloth's own CCD pass, e its [ne, 2] edges, is
            cd.sweep_segments_all(x0[e[:, 0]], x0[e[:, 1]], x1[e[:, 0]], x1[e[:, 1]], thickness, verts_end=x1, skip_vertices=e)."""
        items, n, x1, skip = self._sweep_segments_pre(a0, b0, a1, b1, dist, verts_end, skip_vertices)
        rows = np.empty((max(cap, 1), 2), dtype=np.uint32)
        arrays = _SweepSegmentRowArrays(cap)
        nrows, info = C.c_uint64(0), CdCcdInfo()
        rc = self.lib.cd_sweep_segments_all(self._ctx, _ptr(x1), _ptr(items), n, _ptr(skip), _ptr(rows) if cap else None, cap, C.byref(nrows), C.byref(arrays.out),
                                            C.byref(info))
        self._chk("cd_sweep_segments_all", rc, allow=(CD_OK, CD_OVERFLOW))
        self.sweep_segments_info = info
        got = min(nrows.value, cap)
        return (rows[:got].copy(), *arrays.take(got), nrows.value, rc)

    def sweep_segments(self, a0, b0, a1, b1, dist, verts_end=None, skip_vertices=None):
        """cd_sweep_segments on the tree that is there; arguments as sweep_segments_all takes them.  -> (face[n] (SWEEP_NONE =
        0xFFFFFFFF: the segment comes within dist of no triangle), ids[n], toi[n] (+inf then), dist[n], s[n], on_seg[n, 3],
        on_tri[n, 3], uv[n, 2], feature[n], end[n], cross[n], side[n], info): per item the row of sweep_segments_all with the smallest
        (toi, ID, face index), bit for bit."""
        items, n, x1, skip = self._sweep_segments_pre(a0, b0, a1, b1, dist, verts_end, skip_vertices)
        face = np.empty(n, dtype=np.uint32)
        arrays = _SweepSegmentRowArrays(n)
        info = CdPointInfo()
        rc = self.lib.cd_sweep_segments(self._ctx, _ptr(x1), _ptr(items), n, _ptr(skip), 0, _ptr(face), C.byref(arrays.out), C.byref(info))
        self._chk("cd_sweep_segments", rc)
        return (face, *arrays.take(n), info)

    def find_collisions(self, cap: int = 1 << 20):
        return self._pairs_call(self.lib.cd_find_collisions, "cd_find_collisions", cap)

    def self_collide(self, cap: int = 1 << 20, copy: bool = True):
        return self._pairs_call(self.lib.cd_self_collide, "cd_self_collide", cap, copy=copy)

    def self_collide_into(self, buf: np.ndarray):
        """cd_self_collide and cd_get_stats with every ctypes argument built ONCE (a per-frame loop: the marshalling of the
        generic path costs several microseconds a step).  buf: caller-owned uint32[cap, 2], reused.  Returns (n_pairs, rc);
        the pairs are buf[:min(n_pairs, cap)], the statistics self.fast_stats (a CdStats refreshed by every call)."""
        fc = getattr(self, "_fast", None)
        if fc is None or fc[0] is not buf:
            n = C.c_uint64(0)
            self.fast_stats = CdStats()
            fc = self._fast = (buf, _ptr(buf), C.c_uint64(buf.shape[0]), n, C.byref(n), C.byref(self.fast_stats),
                               self.lib.cd_self_collide, self.lib.cd_get_stats)
        rc = fc[6](self._ctx, fc[1], fc[2], fc[4])
        if rc != CD_OK and rc != CD_OVERFLOW:
            raise CdError("cd_self_collide", rc)
        fc[7](self._ctx, fc[5])
        return fc[3].value, rc

    def sorted_pairs(self, cap: int = 1 << 20):
        """Pair list of the last traversal, sorted by (a, b) on the device."""
        return self._pairs_call(self.lib.cd_sorted_pairs, "cd_sorted_pairs", cap)

    def collision_triangles(self, cap: int = 1 << 21):
        """Sorted distinct triangle IDs of the last traversal's pairs (main.cu:33-45), built on the device."""
        n = C.c_uint64(0)
        buf = np.empty(cap, dtype=np.uint32)
        rc = self.lib.cd_collision_triangles(self._ctx, _ptr(buf), cap, C.byref(n))
        self._chk("cd_collision_triangles", rc, allow=(CD_OK, CD_OVERFLOW))
        return buf[:min(n.value, cap)].copy(), n.value, rc

    def brute_force(self, box_filter: bool = True, cap: int = 1 << 20):
        return self._pairs_call(self.lib.cd_brute_force, "cd_brute_force", cap, 1 if box_filter else 0)

    def test_pairs(self, pairs: np.ndarray) -> np.ndarray:
        p = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        out = np.zeros(p.shape[0], dtype=np.uint8)
        self._chk("cd_test_pairs", self.lib.cd_test_pairs(self._ctx, _ptr(p), p.shape[0], _ptr(out)))
        return out

    # ---- read-back
    def export_keys(self):
        keys = np.zeros(self.nt, dtype=np.uint64)
        perm = np.zeros(self.nt, dtype=np.uint32)
        self._chk("cd_export_keys", self.lib.cd_export_keys(self._ctx, _ptr(keys), _ptr(perm)))
        return keys, perm

    def export_tree(self, with_boxes: bool = True):
        n = self.nt
        parent = np.zeros(2 * n - 1, dtype=np.int32)
        left = np.zeros(max(n - 1, 0), dtype=np.int32)
        right = np.zeros(max(n - 1, 0), dtype=np.int32)
        boxes = np.zeros((2 * n - 1, 6), dtype=np.float64) if with_boxes else None
        bounded = np.zeros(max(n - 1, 0), dtype=np.uint32) if with_boxes else None
        self._chk("cd_export_tree", self.lib.cd_export_tree(self._ctx, _ptr(parent), _ptr(left), _ptr(right), _ptr(boxes), _ptr(bounded)))
        return parent, left, right, boxes, bounded

    def stats(self) -> CdStats:
        s = CdStats()
        self._chk("cd_get_stats", self.lib.cd_get_stats(self._ctx, C.byref(s)))
        return s

    def debug_counters(self) -> np.ndarray:
        out = np.zeros(12, dtype=np.uint64)
        self._chk("cd_debug_counters", self.lib.cd_debug_counters(self._ctx, out.ctypes.data))
        return out

    def debug_hint(self, with_order: bool = True, with_tri: bool = False):
        g = (self.nt + 63) // 64
        cost = np.zeros(g, dtype=np.uint32); order = np.zeros(g, dtype=np.uint32); tri = np.zeros(self.nt, dtype=np.uint8)
        self._chk("cd_debug_hint", self.lib.cd_debug_hint(self._ctx, _ptr(cost), _ptr(order) if with_order else None, _ptr(tri) if with_tri else None))
        return (cost, (order if with_order else None), tri) if with_tri else (cost, (order if with_order else None))

    def debug_hint_set(self, order: np.ndarray):
        o = np.ascontiguousarray(order, dtype=np.uint32)
        self._chk("cd_debug_hint_set", self.lib.cd_debug_hint_set(self._ctx, _ptr(o)))

    def debug_records(self):
        """(right halves u32[n, 8], left halves u32[n, 8], query boxes u32[n, 8], root split) of the current tree."""
        n = self.nt
        recs = np.zeros((2 * n, 8), dtype=np.uint32)
        qb = np.zeros((n, 8), dtype=np.uint32)
        root = C.c_int32(0)
        self._chk("cd_debug_records", self.lib.cd_debug_records(self._ctx, recs.ctypes.data, qb.ctypes.data, C.byref(root)))
        return recs[:n], recs[n:], qb, int(root.value)

    def debug_swept(self, other=None):
        """(right halves u32[n, 8], left halves u32[n, 8], up i32[2n - 1], m_bits, pad as an fp32 scalar) of the swept tree the last CCD
        pass left: this context's own (find_ccd / self_ccd), or with `other` the one this context holds of `other` after
        find_ccd_between(other).  n = 1: no records, the arrays come back empty."""
        which = 0 if other is None else 1
        m, pad, got = C.c_uint32(0), C.c_float(0.0), C.c_uint32(0)
        self._chk("cd_debug_swept", self.lib.cd_debug_swept(self._ctx, which, None, None, None, None, C.byref(got)))   # the size first
        n = got.value
        if n != (self.nt if other is None else other.nt):
            raise ValueError(f"the swept tree there has {n} leaves: not this mesh's")
        if n < 2:                                                              # no records: only M and the pad are there
            self._chk("cd_debug_swept", self.lib.cd_debug_swept(self._ctx, which, None, None, C.byref(m), C.byref(pad), None))
            none = np.zeros((0, 8), dtype=np.uint32)
            return none, none, np.zeros(0, dtype=np.int32), int(m.value), np.float32(pad.value)
        recs = np.zeros((2 * n, 8), dtype=np.uint32)
        up = np.zeros(2 * n - 1, dtype=np.int32)
        self._chk("cd_debug_swept", self.lib.cd_debug_swept(self._ctx, which, recs.ctypes.data, up.ctypes.data, C.byref(m), C.byref(pad), None))
        return recs[:n], recs[n:], up, int(m.value), np.float32(pad.value)

    # ---- cross-rank pass
    def set_vertex_id_base(self, base: int):
        self._chk("cd_set_vertex_id_base", self.lib.cd_set_vertex_id_base(self._ctx, base))

    def root_box(self) -> np.ndarray:
        b = np.zeros(6, dtype=np.float64)
        self._chk("cd_root_box", self.lib.cd_root_box(self._ctx, _ptr(b)))
        return b

    def pack_queries_into(self, box, d_out_ptr: int, cap: int):
        """Compact overlapping leaves into a caller-owned DEVICE buffer (e.g. torch tensor data_ptr)."""
        b = np.ascontiguousarray(box, dtype=np.float64)
        n = C.c_uint64(0)
        rc = self.lib.cd_pack_queries(self._ctx, _ptr(b), C.c_void_p(d_out_ptr), cap, C.byref(n))
        self._chk("cd_pack_queries", rc, allow=(CD_OK, CD_OVERFLOW))
        return n.value, rc

    def find_collisions_queries(self, d_queries_ptr: int, nq: int, cap: int = 1 << 20):
        return self._pairs_call(self.lib.cd_find_collisions_queries, "cd_find_collisions_queries", cap,
                                C.c_void_p(d_queries_ptr), C.c_uint64(nq))


def load_obj(path: str, threads: int = 0):
    """cd_load_obj through the C ABI -> (verts float64[V,3], vidx uint32[N,3]).  Host only, needs no GPU."""
    lib = load_library()
    pv, pf = C.POINTER(C.c_double)(), C.POINTER(C.c_uint32)()
    nv, nt = C.c_uint32(0), C.c_uint32(0)
    rc = lib.cd_load_obj(path.encode(), C.byref(pv), C.byref(nv), C.byref(pf), C.byref(nt), threads)
    if rc != CD_OK:
        raise CdError("cd_load_obj", rc)
    try:
        verts = np.ctypeslib.as_array(pv, shape=(nv.value, 3)).copy()
        vidx = np.ctypeslib.as_array(pf, shape=(nt.value, 3)).copy()
    finally:
        lib.cd_free_obj(pv, pf)
    return verts, vidx


class HostPairs:
    """cd_alloc_host_pairs: a uint32[cap, 2] array in pinned host memory the library lets the GPU write straight into
    (.array; hand it to CollisionDetector.self_collide_into).  Freed by close() / the context manager."""

    def __init__(self, cap: int):
        self.lib = load_library()
        self._p = C.POINTER(C.c_uint32)()
        rc = self.lib.cd_alloc_host_pairs(cap, C.byref(self._p))
        if rc != CD_OK:
            raise CdError("cd_alloc_host_pairs", rc)
        self.array = np.ctypeslib.as_array(self._p, shape=(cap, 2))

    def close(self):
        if self._p:
            self.array = None
            self.lib.cd_free_host_pairs(self._p)
            self._p = C.POINTER(C.c_uint32)()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def morton3d_points(xyz, offset=None, span=None) -> np.ndarray:
    """morton.h:70-89 morton3D on explicit points, on the device (cd_morton3d_points)."""
    p = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    off = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64)
    sp = None if span is None else np.ascontiguousarray(span, dtype=np.float64)
    keys = np.zeros(p.shape[0], dtype=np.uint64)
    rc = load_library().cd_morton3d_points(_ptr(p), p.shape[0], _ptr(off), _ptr(sp), _ptr(keys))
    if rc != CD_OK:
        raise CdError("cd_morton3d_points", rc)
    return keys


def morton3d_points_layout(xyz, offset, span, layout: int) -> np.ndarray:
    """The key of explicit points in a frame with a key layout (cd_morton3d_points_layout; layout 0 = morton3d_points)."""
    p = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    off = np.ascontiguousarray(offset, dtype=np.float64); sp = np.ascontiguousarray(span, dtype=np.float64)
    keys = np.zeros(p.shape[0], dtype=np.uint64)
    rc = load_library().cd_morton3d_points_layout(_ptr(p), p.shape[0], _ptr(off), _ptr(sp), int(layout), _ptr(keys))
    if rc != CD_OK:
        raise CdError("cd_morton3d_points_layout", rc)
    return keys


def expand64_values(v) -> np.ndarray:
    """morton.h:7-29 expand64Bits on explicit values, on the device (cd_expand64_values)."""
    a = np.ascontiguousarray(v, dtype=np.uint64).ravel()
    out = np.zeros(a.shape[0], dtype=np.uint64)
    rc = load_library().cd_expand64_values(_ptr(a), a.shape[0], _ptr(out))
    if rc != CD_OK:
        raise CdError("cd_expand64_values", rc)
    return out


def box_pairs(a, b, want_merged=True):
    """box.cuh:40-43 checkBoxOverlap and box.cuh:24-32 Box::merge on explicit boxes, on the device (cd_box_pairs)."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 6); b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1, 6)
    ov = np.zeros(a.shape[0], dtype=np.uint8)
    mg = np.zeros_like(a) if want_merged else None
    rc = load_library().cd_box_pairs(_ptr(a), _ptr(b), a.shape[0], _ptr(ov), _ptr(mg))
    if rc != CD_OK:
        raise CdError("cd_box_pairs", rc)
    return ov, mg


def tri_contact_points(tri) -> np.ndarray:
    """tri_contact.cuh:19-78 checkTriangleContact on explicit vertex positions [n, 6, 3], on the device (cd_tri_contact_points)."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 18)
    out = np.zeros(t.shape[0], dtype=np.uint8)
    rc = load_library().cd_tri_contact_points(_ptr(t), t.shape[0], _ptr(out))
    if rc != CD_OK:
        raise CdError("cd_tri_contact_points", rc)
    return out


def tri_distance_points(tri) -> np.ndarray:
    """tri_distance (0 for a pair in contact, else the minimum over the 15 feature pairs) on explicit vertex positions [n, 6, 3],
    on the device (cd_tri_distance_points)."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 18)
    out = np.zeros(t.shape[0], dtype=np.float64)
    rc = load_library().cd_tri_distance_points(_ptr(t), t.shape[0], _ptr(out))
    if rc != CD_OK:
        raise CdError("cd_tri_distance_points", rc)
    return out


def tri_witness_points(tri):
    """tri_witness (where tri_distance is attained) on explicit vertex positions [n, 6, 3], on the device (cd_tri_witness_points):
    (dist[n], points[n, 2, 3] (qa, qb), bary[n, 2, 2] ((ua, va), (ub, vb)), feature[n, 2])."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 18)
    n = t.shape[0]
    dist = np.zeros(n, dtype=np.float64)
    points = np.zeros((n, 2, 3), dtype=np.float64)
    bary = np.zeros((n, 2, 2), dtype=np.float64)
    feature = np.zeros((n, 2), dtype=np.uint8)
    rc = load_library().cd_tri_witness_points(_ptr(t), n, _ptr(dist), _ptr(points), _ptr(bary), _ptr(feature))
    if rc != CD_OK:
        raise CdError("cd_tri_witness_points", rc)
    return dist, points, bary, feature


def tri_isect_points(tri, want_param=True, want_points=True):
    """tri_isect (the segment two triangles cut each other in) on explicit vertex positions [n, 6, 3], on the device
    (cd_tri_isect_points): (code[n, 3] (endpoint 0, endpoint 1 as term | side << 3, the mask), param[n, 2, 3] ((t, u, v) of the two
    endpoints), points[n, 2, 3]); param / points are None when not wanted (the call then gets NULL)."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 18)
    n = t.shape[0]
    code = np.zeros((n, 3), dtype=np.uint8)
    param = np.zeros((n, 2, 3), dtype=np.float64) if want_param else None
    points = np.zeros((n, 2, 3), dtype=np.float64) if want_points else None
    rc = load_library().cd_tri_isect_points(_ptr(t), n, _ptr(code), _ptr(param), _ptr(points))
    if rc != CD_OK:
        raise CdError("cd_tri_isect_points", rc)
    return code, param, points


def pack_rays(origins, dirs, tmax=np.inf) -> np.ndarray:
    """[n, 7] doubles (o, d, tmax), the layout cd_cast_rays and cd_ray_tri_points take."""
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f"origins {o.shape} and dirs {d.shape} differ")
    rays = np.empty((o.shape[0], 7), dtype=np.float64)
    rays[:, 0:3] = o
    rays[:, 3:6] = d
    rays[:, 6] = tmax
    return rays


def ray_tri_points(rays, tris):
    """ray_tri (the per-pair predicate of cd_cast_rays) on explicit operands, on the device (cd_ray_tri_points): rays [n, 7]
    (o, d, tmax), tris [n, 3, 3] -> (hit[n] bool, t[n], uv[n, 2], side[n]); t, uv, side are 0 on a miss."""
    r = np.ascontiguousarray(np.asarray(rays, dtype=np.float64).reshape(-1, 7))
    p = np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 9))
    if r.shape[0] != p.shape[0]:
        raise ValueError(f"{r.shape[0]} rays against {p.shape[0]} triangles")
    n = r.shape[0]
    hit = np.zeros(n, dtype=np.uint8)
    t = np.zeros(n, dtype=np.float64)
    uv = np.zeros((n, 2), dtype=np.float64)
    side = np.zeros(n, dtype=np.uint8)
    rc = load_library().cd_ray_tri_points(_ptr(r), _ptr(p), n, _ptr(hit), _ptr(t), _ptr(uv), _ptr(side))
    if rc != CD_OK:
        raise CdError("cd_ray_tri_points", rc)
    return hit.astype(bool), t, uv, side


def pack_points(points, rmax=np.inf) -> np.ndarray:
    """[n, 4] doubles (x, y, z, rmax), the layout cd_closest_points takes."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pts = np.empty((p.shape[0], 4), dtype=np.float64)
    pts[:, 0:3] = p
    pts[:, 3] = rmax
    return pts


def pt_tri_points(points, tris):
    """pt_tri (the per-pair predicate of cd_closest_points) on explicit operands, on the device (cd_pt_tri_points): points [n, 3],
    tris [n, 3, 3] -> (dist[n], closest[n, 3], uv[n, 2], feature[n], side[n])."""
    q = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    p = np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 9))
    if q.shape[0] != p.shape[0]:
        raise ValueError(f"{q.shape[0]} points against {p.shape[0]} triangles")
    n = q.shape[0]
    dist = np.zeros(n, dtype=np.float64)
    closest = np.zeros((n, 3), dtype=np.float64)
    uv = np.zeros((n, 2), dtype=np.float64)
    feature = np.zeros(n, dtype=np.uint8)
    side = np.zeros(n, dtype=np.uint8)
    rc = load_library().cd_pt_tri_points(_ptr(q), _ptr(p), n, _ptr(dist), _ptr(closest), _ptr(uv), _ptr(feature), _ptr(side))
    if rc != CD_OK:
        raise CdError("cd_pt_tri_points", rc)
    return dist, closest, uv, feature, side


def column_tri_points(points, tris, axis: int = 2):
    """column_tri (the per-pair predicate of cd_points_inside) on explicit operands, on the device (cd_column_tri_points): points
    [n, 3], tris [n, 3, 3], axis 0..2 -> (cover[n] (int8: 0 / +1 / -1), above[n] (bool), E[n, 3], zc[n], S[n])."""
    q = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    p = np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 9))
    if q.shape[0] != p.shape[0]:
        raise ValueError(f"{q.shape[0]} points against {p.shape[0]} triangles")
    n = q.shape[0]
    cover = np.zeros(n, dtype=np.int8)
    above = np.zeros(n, dtype=np.uint8)
    E = np.zeros((n, 3), dtype=np.float64)
    zc = np.zeros(n, dtype=np.float64)
    S = np.zeros(n, dtype=np.float64)
    rc = load_library().cd_column_tri_points(_ptr(q), _ptr(p), n, int(axis), _ptr(cover), _ptr(above), _ptr(E), _ptr(zc), _ptr(S))
    if rc != CD_OK:
        raise CdError("cd_column_tri_points", rc)
    return cover, above.astype(bool), E, zc, S


def pack_boxes(lo, hi) -> np.ndarray:
    """[n, 6] doubles {x1, x2, y1, y2, z1, z2}, the layout cd_boxes_overlap_all, cd_boxes_count and cd_root_box use."""
    a = np.asarray(lo, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(hi, dtype=np.float64).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"{a.shape[0]} lower corners against {b.shape[0]} upper corners")
    return np.ascontiguousarray(np.stack([a, b], axis=2).reshape(-1, 6))


def box_tri_points(boxes, tris):
    """box_tri (the per-pair predicate of the box queries) on explicit operands, on the device (cd_box_tri_points): boxes [n, 6]
    {x1, x2, y1, y2, z1, z2}, tris [n, 3, 3] -> (hit[n] (bool), inside[n] (bool), code[n] (uint8: 0, or the first separating test))."""
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 6))
    p = np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 9))
    if b.shape[0] != p.shape[0]:
        raise ValueError(f"{b.shape[0]} boxes against {p.shape[0]} triangles")
    n = b.shape[0]
    hit = np.zeros(n, dtype=np.uint8)
    inside = np.zeros(n, dtype=np.uint8)
    code = np.zeros(n, dtype=np.uint8)
    rc = load_library().cd_box_tri_points(_ptr(b), _ptr(p), n, _ptr(hit), _ptr(inside), _ptr(code))
    if rc != CD_OK:
        raise CdError("cd_box_tri_points", rc)
    return hit.astype(bool), inside.astype(bool), code


def pack_planes(normals, d) -> np.ndarray:
    """[n, 4] doubles {nx, ny, nz, d}, the layout cd_planes_cut_all, cd_planes_count and cd_plane_tri_points take."""
    a = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(d, dtype=np.float64).reshape(-1)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"{a.shape[0]} normals against {b.shape[0]} offsets")
    return np.ascontiguousarray(np.concatenate([a, b[:, None]], axis=1))


def plane_tri_points(planes, tris):
    """plane_tri (the per-pair predicate of the plane queries) on explicit operands, on the device (cd_plane_tri_points): planes
    [n, 4] {nx, ny, nz, d}, tris [n, 3, 3] -> (cls[n] (uint8: CD_PLANE_ABOVE / BELOW / CUT), seg[n, 2, 3] (a, b), edge[n, 2], t[n, 2],
    on[n] (bit i: vertex i lies in the plane))."""
    b = np.ascontiguousarray(np.asarray(planes, dtype=np.float64).reshape(-1, 4))
    p = np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 9))
    if b.shape[0] != p.shape[0]:
        raise ValueError(f"{b.shape[0]} planes against {p.shape[0]} triangles")
    n = b.shape[0]
    cls, on = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    seg, edge, t = np.zeros((n, 2, 3)), np.zeros((n, 2), dtype=np.uint8), np.zeros((n, 2))
    rc = load_library().cd_plane_tri_points(_ptr(b), _ptr(p), n, _ptr(cls), _ptr(seg), _ptr(edge), _ptr(t), _ptr(on))
    if rc != CD_OK:
        raise CdError("cd_plane_tri_points", rc)
    return cls, seg, edge, t, on


def pack_segments(a, b, r=np.inf) -> np.ndarray:
    """[n, 7] doubles (a, b, r), the layout cd_segments_within and cd_segments_closest take."""
    p = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    if p.shape != q.shape:
        raise ValueError(f"{p.shape[0]} first ends against {q.shape[0]} second ends")
    segs = np.empty((p.shape[0], 7), dtype=np.float64)
    segs[:, 0:3] = p
    segs[:, 3:6] = q
    segs[:, 6] = r
    return segs


def seg_tri_points(segs, tris):
    """seg_tri (the per-pair predicate of the segment queries) on explicit operands, on the device (cd_seg_tri_points): segs [n, 6]
    (a, b), tris [n, 3, 3] -> (dist[n], s[n], on_seg[n, 3], on_tri[n, 3], uv[n, 2], feature[n], end[n], cross[n], side[n])."""
    q = np.ascontiguousarray(np.asarray(segs, dtype=np.float64).reshape(-1, 6))
    p = np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 9))
    if q.shape[0] != p.shape[0]:
        raise ValueError(f"{q.shape[0]} segments against {p.shape[0]} triangles")
    n = q.shape[0]
    dist, s, on_seg, on_tri, uv = np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 2))
    feature, end, cross, side = (np.zeros(n, dtype=np.uint8) for _ in range(4))
    rc = load_library().cd_seg_tri_points(_ptr(q), _ptr(p), n, _ptr(dist), _ptr(s), _ptr(on_seg), _ptr(on_tri), _ptr(uv), _ptr(feature), _ptr(end), _ptr(cross),
                                          _ptr(side))
    if rc != CD_OK:
        raise CdError("cd_seg_tri_points", rc)
    return dist, s, on_seg, on_tri, uv, feature, end, cross, side


def pack_swept_segments(a0, b0, a1, b1, dist) -> np.ndarray:
    """[n, 13] doubles (a0, b0, a1, b1, dist), the layout cd_sweep_segments_all, cd_sweep_segments and cd_seg_advance_points take."""
    pts = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (a0, b0, a1, b1)]
    if any(x.shape != pts[0].shape for x in pts):
        raise ValueError(f"a0, b0, a1, b1 differ in shape: {[x.shape for x in pts]}")
    items = np.empty((pts[0].shape[0], 13), dtype=np.float64)
    for k, x in enumerate(pts):
        items[:, 3 * k:3 * k + 3] = x
    items[:, 12] = dist
    return items


def seg_advance_points(items, tris):
    """seg_advance (the per-pair function of the swept-segment queries) on explicit operands, on the device (cd_seg_advance_points):
    items [n, 13] (a0, b0, a1, b1, dist), tris [n, 6, 3] (the triangle's vertices at the start, then at the end) -> (toi[n] (+inf: not
    reported), dist[n], s[n], on_seg[n, 3], on_tri[n, 3], uv[n, 2], feature[n], end[n], cross[n], side[n], evals[n]), the values those
    of the last evaluation made."""
    it = np.ascontiguousarray(np.asarray(items, dtype=np.float64).reshape(-1, 13))
    t = np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 18))
    if it.shape[0] != t.shape[0]:
        raise ValueError(f"{it.shape[0]} items against {t.shape[0]} triangles")
    n = it.shape[0]
    toi, dist, s, on_seg, on_tri, uv = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 2))
    feature, end, cross, side = (np.zeros(n, dtype=np.uint8) for _ in range(4))
    ev = np.zeros(n, dtype=np.uint32)
    rc = load_library().cd_seg_advance_points(_ptr(it), _ptr(t), n, _ptr(toi), _ptr(dist), _ptr(s), _ptr(on_seg), _ptr(on_tri), _ptr(uv), _ptr(feature), _ptr(end),
                                              _ptr(cross), _ptr(side), _ptr(ev))
    if rc != CD_OK:
        raise CdError("cd_seg_advance_points", rc)
    return toi, dist, s, on_seg, on_tri, uv, feature, end, cross, side, ev


def pack_sweeps(p0, p1, dist) -> np.ndarray:
    """[n, 7] doubles (p0, p1, dist), the layout cd_sweep_points_all, cd_sweep_points and cd_pt_advance_points take."""
    a = np.asarray(p0, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(p1, dtype=np.float64).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"p0 {a.shape} and p1 {b.shape} differ")
    items = np.empty((a.shape[0], 7), dtype=np.float64)
    items[:, 0:3] = a
    items[:, 3:6] = b
    items[:, 6] = dist
    return items


def pt_advance_points(items, tris):
    """pt_advance (the per-pair function of the swept-point queries) on explicit operands, on the device (cd_pt_advance_points): items
    [n, 7] (p0, p1, dist), tris [n, 6, 3] (a0 a1 a2 at the start, b0 b1 b2 at the end) -> (toi[n] (+inf: not reported), dist[n],
    closest[n, 3], uv[n, 2], feature[n], side[n], evals[n]), the values those of the last evaluation made."""
    it = np.ascontiguousarray(np.asarray(items, dtype=np.float64).reshape(-1, 7))
    t = np.ascontiguousarray(np.asarray(tris, dtype=np.float64).reshape(-1, 18))
    if it.shape[0] != t.shape[0]:
        raise ValueError(f"{it.shape[0]} items against {t.shape[0]} triangles")
    n = it.shape[0]
    toi = np.zeros(n, dtype=np.float64)
    dist = np.zeros(n, dtype=np.float64)
    closest = np.zeros((n, 3), dtype=np.float64)
    uv = np.zeros((n, 2), dtype=np.float64)
    feature = np.zeros(n, dtype=np.uint8)
    side = np.zeros(n, dtype=np.uint8)
    ev = np.zeros(n, dtype=np.uint32)
    rc = load_library().cd_pt_advance_points(_ptr(it), _ptr(t), n, _ptr(toi), _ptr(dist), _ptr(closest), _ptr(uv), _ptr(feature), _ptr(side), _ptr(ev))
    if rc != CD_OK:
        raise CdError("cd_pt_advance_points", rc)
    return toi, dist, closest, uv, feature, side, ev


def ccd_points(tri, dist: float):
    """The per-pair continuous advancement (cd_ccd_points) on explicit positions [n, 12, 3] (A's and B's vertices at x0, then at x1):
    (toi[n] (+inf: not reported), dists[n], evals[n])."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 36)
    toi = np.zeros(t.shape[0], dtype=np.float64)
    d = np.zeros(t.shape[0], dtype=np.float64)
    ev = np.zeros(t.shape[0], dtype=np.uint32)
    rc = load_library().cd_ccd_points(_ptr(t), t.shape[0], float(dist), _ptr(toi), _ptr(d), _ptr(ev))
    if rc != CD_OK:
        raise CdError("cd_ccd_points", rc)
    return toi, d, ev


def version() -> str:
    return load_library().cd_version().decode()


def multi_unique_id() -> bytes:
    """ncclGetUniqueId through the library (128 bytes): made on one rank, handed to all."""
    lib = load_library()
    buf = C.create_string_buffer(128)
    rc = lib.cd_multi_unique_id(buf)
    if rc != CD_OK:
        raise CdError("cd_multi_unique_id", rc)
    return buf.raw


class MultiStep:
    """The multi-GPU step of libmi355cd.so (cd_multi_*): RCCL collectives issued by the C++ side, one process per GPU."""

    def __init__(self, cd: "CollisionDetector", unique_id: bytes, rank: int, world: int, query_cap_per_peer: int = 0, flags: int = 0,
                 nccl_comm: int | None = None):
        """unique_id / rank / world: the library creates (and owns) the communicator.  nccl_comm: an existing ncclComm_t (as an
        integer address) whose rank and size are used instead; it stays the caller's."""
        self.lib = cd.lib
        self.cd = cd
        self._m = C.c_void_p()
        if nccl_comm is not None:
            rc = self.lib.cd_multi_create_from_comm(C.byref(self._m), cd._ctx, C.c_void_p(nccl_comm), query_cap_per_peer, flags)
            name = "cd_multi_create_from_comm"
        else:
            rc = self.lib.cd_multi_create(C.byref(self._m), cd._ctx, C.c_char_p(unique_id), rank, world, query_cap_per_peer, flags)
            name = "cd_multi_create"
        if rc != CD_OK:
            raise CdError(name, rc)
        self._pairs = None

    def step(self, cap: int = 1 << 22, pairs: np.ndarray | None = None):
        """pairs: the caller's own C-contiguous uint32 array of at least cap rows of 2, written in place (rows behind cap are the
        caller's: a test keeps a canary there); None: a buffer the object keeps -- and with cap 0 a NULL pointer (count only)."""
        if pairs is not None:
            if pairs.dtype != np.uint32 or pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < cap or not pairs.flags.c_contiguous or not pairs.flags.writeable:
                raise ValueError("pairs must be a writable C-contiguous uint32 array of shape [>= cap, 2]")
            buf, ptr = pairs, C.c_void_p(pairs.ctypes.data)
        elif cap == 0:
            buf, ptr = np.empty((0, 2), dtype=np.uint32), C.c_void_p(None)
        else:
            if self._pairs is None or self._pairs.shape[0] < cap:
                self._pairs = np.empty((cap, 2), dtype=np.uint32)
            buf, ptr = self._pairs, C.c_void_p(self._pairs.ctypes.data)
        n = C.c_uint64(0)
        info = CdMultiInfo()
        rc = self.lib.cd_multi_step(self._m, ptr, cap, C.byref(n), C.byref(info))
        if rc < 0:
            raise CdError("cd_multi_step", rc)
        return buf[: min(n.value, cap)], int(n.value), rc, info

    def set_flags(self, flags: int):
        rc = self.lib.cd_multi_set_flags(self._m, flags)
        if rc != CD_OK:
            raise CdError("cd_multi_set_flags", rc)

    def close(self):
        if self._m:
            self.lib.cd_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
