/*
 * mi355cd.h -- C ABI of libmi355cd.so: MI355X-native (HIP, gfx950) triangle-mesh collision detection.
 *
 * Drop-in boundary for the CollisionDetection hot path of Asichurter/GPU-Computing-Course.  The
 * reference has no FFI; its boundary is the sequence of kernel call sites in CollisionDetection/main.cu.
 * Each export below names the call site (reference file:line) it replaces.  Host pointers in, the
 * library owns all device memory behind an opaque context; plain pointers and sizes only.
 *
 * Conventions
 *   - every function returns int: 0 = ok; <0 = -(hipError_t) or one of CD_ERR_*; >0 = CD_OVERFLOW
 *     (the reference prints and exits via HANDLE_ERROR, common/book.h:21-30; this library never exits).
 *   - one context per device; a context is not thread-safe; different contexts are independent.
 *   - all calls block until the stage has finished (the reference synchronises after every kernel,
 *     main.cu:93,100,109,...).  Per-stage device times are measured with HIP events on the
 *     context's own stream and read back through cd_get_stats().
 *   - node ids: internal node i -> i (root = 0, main.cu:142 passes &internal_nodes[0]);
 *     leaf j (Morton-sorted position) -> (n-1)+j.  -1 = NULL.
 *   - boxes are {x1,x2,y1,y2,z1,z2} doubles, the field order of box.cuh:9.
 */
#ifndef MI355CD_H
#define MI355CD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cd_ctx cd_ctx;

enum {
    CD_OK            = 0,
    CD_OVERFLOW      = 1,      /* more pairs than cap_pairs; *n_pairs holds the true count          */
    CD_ERR_ARG       = -1001,  /* null / zero-sized / inconsistent argument                         */
    CD_ERR_ORDER     = -1002,  /* stage called before the stage it depends on                       */
    CD_ERR_NO_DEVICE = -1003,  /* no HIP device: the library has no CPU fallback                    */
    CD_ERR_INDEX     = -1004,  /* a vertex index >= nv (checked at cd_create)                       */
    CD_ERR_SORT      = -1005,  /* a bounded device-side wait in the sort timed out (results invalid) */
    CD_ERR_IO        = -1006,  /* file cannot be opened / read                                      */
    CD_ERR_FORMAT    = -1007,  /* a `v` / `f` line is not in the reference's dialect, or no geometry */
    CD_ERR_RCCL      = -1008,  /* librccl could not be loaded, or an RCCL call failed (cd_multi_*)   */
    CD_ERR_PEER      = -1009,  /* cd_multi_*: ANOTHER rank failed in this step; every rank returned in the same step (that rank its own error) */
    CD_ERR_INJECTED  = -1010   /* cd_multi_step: the failure asked for with CD_MULTI_INJECT_FAILURE (tests)  */
};

/* Morton normalisation frame (morton.h:43-58 hard-codes one data set's bounds). */
enum {
    CD_FRAME_REFERENCE = 0,    /* the constants of morton.h:45,51,57 -> keys bit-identical to morton3D */
    CD_FRAME_AUTO      = 1,    /* from the mesh, computed on the device in every step: AABB of the centroids AND the
                                  key layout that suits it (below: "the adaptive frame")                      */
    CD_FRAME_CUSTOM    = 2     /* caller-supplied offset[3], span[3]                                   */
};

typedef struct cd_stats {
    /* device time of the last run of each stage, milliseconds (HIP events on the context stream) */
    float ms_morton;           /* centroid + Morton keys                    (load_obj.h:89-101)      */
    float ms_sort;             /* radix sort by key                         (load_obj.h:107)         */
    float ms_hierarchy;        /* leaf fill + Karras hierarchy              (main.cu:92,99)          */
    float ms_refit;            /* bottom-up AABB refit                      (main.cu:107)            */
    float ms_traverse;         /* traversal + exact test                    (main.cu:142)            */
    float ms_check;            /* verifier kernels                          (main.cu:115,123,131)    */
    uint32_t traverse_launches;/* kernel launches inside the last traversal (0: the step was a graph replay, CD_OPT_GRAPH) */
    uint32_t stack_overflows;  /* queries that needed the deep-stack fallback in the last traversal */
    uint64_t n_pairs;          /* contacts found by the last traversal      (main.cu:145 test_val)   */
    uint64_t pairs_tested;     /* (query, leaf) pairs with strictly overlapping AABBs                */
    uint64_t node_visits;      /* internal nodes visited                                             */
    uint64_t wave_steps;       /* descent-loop iterations summed over wavefronts (lane utilisation =  */
                               /* node_visits / (64 * wave_steps)); 0 for CD_OPT_TRAVERSAL 0           */
    uint64_t candidates;       /* (query, leaf) candidates the fp32 descent handed to the exact kernel */
    float ms_descend;          /* shallow pass: memset + descent kernel (part of ms_traverse)          */
    float ms_exact;            /* shallow pass: exact-test kernel        (part of ms_traverse)          */
    uint32_t sort_passes;      /* 8-bit key digits the last sort ordered globally: 2 (hybrid: by two passes or, for meshes */
                               /* in coherent order, by one launch that places keys by cell), 4 (half-key) or 8            */
    float ms_pipeline;         /* fused calls: pipeline start -> end of the traversal kernels, one event pair */
    float ms_build_block;      /* fused calls: the kernel that builds hierarchy + boxes + records of the 512-leaf     */
                               /* blocks (k_refit_seg_local<fused>), from its own dispatch packet; part of ms_refit  */
    float ms_descend_clock;    /* the descent kernel (CD_OPT_TRAVERSAL 3) timed by ITSELF: first wave start -> last wave end on the    */
                               /* device's constant-rate wall clock (s_memrealtime, hipDeviceAttributeWallClockRate).  Taken in every */
                               /* call at no cost; slightly below ms_descend (the dispatch packet's stamps also cover launch and the  */
                               /* end-of-kernel write-back).  0 when the traversal needed a deep pass or another variant ran           */
} cd_stats;

/* main.cu:64 loadObj (load_obj.h:24-103), host side, multi-threaded: parse `v x y z` (as float, widened to double)
 * and `f a/ta b/tb c/tc` (1-based) lines in file order.  Unlike the reference it does not compute Morton codes
 * or sort (cd_morton_sort does, on the GPU) and it returns an error instead of exiting.  The arrays are
 * malloc'ed; release them with cd_free_obj.  threads <= 0: one per hardware thread.  Needs no GPU. */
int cd_load_obj(const char *path, double **verts_xyz, uint32_t *nv, uint32_t **vidx3, uint32_t *nt, int threads);
void cd_free_obj(double *verts_xyz, uint32_t *vidx3);

/* main.cu:78-88  cudaMalloc + cudaMemcpy of vec3f[V], Triangle[N], u64[N], Node[N], Node[N-1].
 * verts_xyz: nv x 3 doubles (vec3f.cuh:14-23).  vidx3: nt x 3 vertex indices (triangle.cuh:9).
 * ids: nt triangle IDs (triangle.cuh:6; load_obj.h:94 uses the face ordinal) or NULL for 0..nt-1. */
int cd_create(cd_ctx **out, const double *verts_xyz, uint32_t nv,
              const uint32_t *vidx3, const uint32_t *ids, uint32_t nt);
void cd_destroy(cd_ctx *ctx);                                               /* main.cu:156-163 */

/* Replace vertex positions (same nv, same topology): the per-frame re-run of a cloth simulation. */
int cd_update_vertices(cd_ctx *ctx, const double *verts_xyz);

/* morton.h:43-58: choose the normalisation frame (default CD_FRAME_REFERENCE). offset/span are
 * read only for CD_FRAME_CUSTOM.  REFERENCE and CUSTOM interleave 20 bits an axis x, y, z exactly as morton.h:70-89.
 *
 * The adaptive frame (CD_FRAME_AUTO; not reference behaviour -- morton.h has its constants and nothing else).  For a mesh
 * those constants do not fit, the library takes offset / span from the bounds of the centroids and DEALS the 60 key bits to
 * the axes so that the cells of every tree level are near cubes in units of the triangles' own mean extent per axis (a thin,
 * long mesh normalised per axis with the fixed interleave gets cells of 400 : 1 and a poor tree).  The pair set does not
 * depend on the keys (any correct BVH gives the reference's set); the tree's cost does.  A layout is one 64-bit word:
 * bit 63 set | A | B << 2 | C << 4 | nA << 8 | nAB << 16 | nABC << 24 -- axes A, B, C (0 = x, 1 = y, 2 = z, by decreasing
 * weight); the key is, from its top bit down, nA bits of A's cell index, nAB pairs (A, B), nABC triples (A, B, C); a cell index along
 * an axis with b bits is floor(((p1 + p2 + p3) - 3 offset) * (2^b / (3 span))) clamped to [0, 2^b - 1];
 * nA + 2 nAB + 3 nABC <= 60.  0 = the reference's interleave.  Derivation and numbers: csrc/cd_math.h, DESIGN.md. */
int cd_set_morton_frame(cd_ctx *ctx, int mode, const double offset[3], const double span[3]);
/* The frame the last sort used -- offset, span, key layout (any may be NULL) -- and a frame WITH a layout installed as
 * CD_FRAME_CUSTOM: a frame CD_FRAME_AUTO computed once and the caller keeps (the AUTO pass over the triangles, ~11 us at
 * 1 M, leaves the step; a centroid that later leaves the frame takes the last cell of its axis), or one frame for all
 * the ranks of a job.  CD_ERR_ORDER before the first sort; CD_ERR_ARG for a word that is not a layout. */
int cd_get_morton_frame(cd_ctx *ctx, double offset[3], double span[3], uint64_t *layout);
int cd_set_morton_frame_layout(cd_ctx *ctx, const double offset[3], const double span[3], uint64_t layout);

/* morton.h:70-89 morton3D(x, y, z) and morton.h:7-29 expand64Bits(v) themselves, on n caller-supplied inputs (host
 * pointers; no context): the device functions cd_morton_sort uses, exposed so that the reference's own functions can be
 * compared value by value (tests/golden/morton_ref.npz holds outputs of the reference's morton.h compiled unmodified).
 * offset / span: both NULL = the constants of morton.h:45,51,57, else a custom frame.  Defined where the reference is
 * undefined: a negative or NaN normalised coordinate maps to cell 0 (morton.h:78's assert is compiled out in Release). */
int cd_morton3d_points(const double *xyz, uint64_t n, const double offset[3], const double span[3], uint64_t *keys);
/* the same in a frame with a key layout: what cd_morton_sort computes per triangle in such a frame, where xyz is the SUM p1 + p2 + p3 of the triangle's vertices per
 * axis (a cell there is floor((sum - 3 offset) * (2^bits / (3 span))), no division per key: csrc/cd_math.h); layout 0 = the call above, xyz the centroid */
int cd_morton3d_points_layout(const double *xyz, uint64_t n, const double offset[3], const double span[3], uint64_t layout, uint64_t *keys);
int cd_expand64_values(const uint64_t *v, uint64_t n, uint64_t *out);

/* box.cuh:40-43 checkBoxOverlap(a, b), box.cuh:24-32 Box::merge(a, b) and tri_contact.cuh:19-78 checkTriangleContact themselves, on n
 * caller-supplied operands (host pointers; no context), for the same purpose: tests/golden/contact_ref.npz holds outputs of the
 * reference's box.cuh / tri_contact.cuh compiled unmodified.  Boxes are {x1,x2,y1,y2,z1,z2} (box.cuh:9); overlap[k] = 0/1 and
 * merged (n x 6) may each be NULL (not both).  tri: n x 18 doubles = P1 P2 P3 Q1 Q2 Q3 positions; out[k] = 0/1 -- no ID rule and
 * no neighbour gate (those are cd_test_pairs). */
int cd_box_pairs(const double *a, const double *b, uint64_t n, uint8_t *overlap, double *merged);
int cd_tri_contact_points(const double *tri, uint64_t n, uint8_t *out);

/* load_obj.h:89-107: centroid + morton3D per face, then sort_by_key(mortons, triangles) -- on the GPU. */
int cd_morton_sort(cd_ctx *ctx);

/* main.cu:92 fillLeafNodes + main.cu:99 generateHierarchyParallel.  *parent_wrong_num is the counter
 * printed at main.cu:103 (children that already had a parent; 0 for a correct tree). May be NULL. */
int cd_build_hierarchy(cd_ctx *ctx, uint32_t *parent_wrong_num);

/* main.cu:107 calBoundingBox: leaf boxes (box.cuh:13-22) and bottom-up merge (box.cuh:24-32). */
int cd_refit_boxes(cd_ctx *ctx);

/* main.cu:115 checkInternalNodes: out = {nullParentNum, wrongBoundNum, nullChildNum, notInternalCount,
 * uninitBoxCount} in the order printed at main.cu:119. */
int cd_check_internal(cd_ctx *ctx, uint32_t out[5]);
/* main.cu:123 checkLeafNodes: out = {nullParentNum, nullTriangleNum, notLeafCount, illegalBoxCount}
 * (main.cu:127).  Triangle::selfCheck's hard-coded 632674 (triangle.cuh:13) is the context's nv. */
int cd_check_leaves(cd_ctx *ctx, uint32_t out[4]);
/* main.cu:131 checkTriangleIdx(leaves, vs, n, maxv, count). */
int cd_check_triangle_idx(cd_ctx *ctx, uint32_t maxv, uint32_t *out);

/* main.cu:142-146 findCollisions + D2H of count and pair list.  pairs: cap_pairs x 2 uint32,
 * interleaved (smaller ID, larger ID), unordered (atomicAdd append, collision.cuh:40-42).
 * pairs may be NULL with cap_pairs 0 (count only).  Returns CD_OVERFLOW when *n_pairs > cap_pairs
 * (the reference writes past its 500-pair buffer instead, main.cu:81). */
int cd_find_collisions(cd_ctx *ctx, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs);

/* main.cu:74,81 (the reference's colTris host array + cudaMalloc'd copy): an output buffer for cap_pairs pairs in PINNED host memory.
 * Optional: every entry point that returns pairs takes any host pointer; handed THIS buffer (the pointer as returned, cap_pairs up to
 * its capacity), cd_find_collisions / cd_self_collide let the GPU write the pairs straight into it -- no staging copy on the host
 * (~4 us of a 0.24 ms step at 20 k pairs).  Release with cd_free_host_pairs, after the last call that uses it. */
int cd_alloc_host_pairs(uint64_t cap_pairs, uint32_t **pairs);
void cd_free_host_pairs(uint32_t *pairs);

/* cd_morton_sort -> cd_build_hierarchy -> cd_refit_boxes queued back to back, one host synchronisation: the tree
 * without the traversal (the multi-GPU step exchanges query leaves while the local traversal runs). */
int cd_build_tree(cd_ctx *ctx);

/* Fused convenience call: cd_morton_sort -> cd_build_hierarchy -> cd_refit_boxes -> cd_find_collisions
 * queued back to back on the context stream with a single host synchronisation at the end. */
int cd_self_collide(cd_ctx *ctx, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs);

/* main.cu:149-154: the pair list of the LAST traversal, sorted ascending by (smaller ID, larger ID) on the device --
 * a deterministic order for diffing (the reference prints in atomicAdd arrival order).  Needs the last
 * cd_find_collisions / cd_self_collide to have had cap_pairs >= its n_pairs (else CD_OVERFLOW).
 * "The last traversal" is the last call that left ONE pair list on the device: cd_find_collisions, cd_self_collide (stream or graph
 * replay, into any buffer), cd_brute_force, cd_find_collisions_queries (its list: external queries against the local tree).  Calls that
 * run no such traversal leave the list as it was: cd_update_vertices followed by cd_build_tree (between the two there is no tree:
 * CD_ERR_ORDER) returns the previous step's list, and so it is after the proximity, CCD, between-mesh, ray and point queries.
 * Both calls need the tree of the current vertices to be there (CD_ERR_ORDER otherwise) -- also after cd_brute_force, which itself
 * needs none: build the tree first (cd_build_tree) when its list is to be post-processed.
 * cd_multi_step leaves two lists (local, cross) and no single one: after it both calls return CD_OVERFLOW when the step found any
 * pair, and n = 0 with CD_OK when it found none, until the next traversal named above.  A call that returns CD_OVERFLOW for a
 * truncated or absent list, or CD_ERR_ORDER, writes nothing -- neither the buffer nor the count; cap below the count: CD_OVERFLOW, the count, and
 * the first cap entries of the sorted result.  Both calls leave cd_stats and the list itself untouched and may be repeated. */
int cd_sorted_pairs(cd_ctx *ctx, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs);
/* main.cu:33-45 makeAndPrintSet: the sorted set of distinct triangle IDs that occur in the pair list,
 * built on the device (sort + unique).  *n = number of distinct IDs (may exceed cap -> CD_OVERFLOW). */
int cd_collision_triangles(cd_ctx *ctx, uint32_t *ids, uint64_t cap, uint64_t *n);

/* check.cuh:117-141 checkDirectComp: O(N^2) all-pairs on the device, no tree.  box_filter != 0 also
 * requires the strict leaf-AABB overlap the BVH path applies (collision.cuh:31-36). Same output format
 * as cd_find_collisions. */
int cd_brute_force(cd_ctx *ctx, int box_filter, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs);

/* tri_contact.cuh:80-87 checkTriangleContactHelper over an explicit list of triangle-index pairs
 * (original triangle order), including the neighborCount<1 gate of collision.cuh:38.  out[k] = 0/1. */
int cd_test_pairs(cd_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs, uint8_t *out);

/* Read-back for verification (the reference's tree is device pointers and cannot be exported). Any
 * pointer may be NULL.  keys/perm: nt entries, sorted order (perm[j] = original triangle of leaf j).
 * parent: 2nt-1; left/right: nt-1; boxes: (2nt-1) x 6; bounded: nt-1 (Node::bounded, bvh.cuh:28). */
int cd_export_keys(cd_ctx *ctx, uint64_t *keys, uint32_t *perm);
int cd_export_tree(cd_ctx *ctx, int32_t *parent, int32_t *left, int32_t *right, double *boxes,
                   uint32_t *bounded);

/* Tuning knobs; none of them changes results (pair sets, pairs_tested are identical for every setting). */
enum {
    CD_OPT_TRAVERSAL        = 0,   /* 0: lane-private FP64 descent, exact test inline (the reference's shape,        */
                                   /*    collision.cuh:19-71); 1: fp32 conservative descent of every query from the   */
                                   /*    root with a wavefront-shared LDS candidate queue + a second kernel for the   */
                                   /*    exact tests; 3 (default): half                                                */
                                   /*    traversal -- a query meets only the leaves to its right in Morton order and   */
                                   /*    every hit counts as the two ordered pairs the reference tests   */
    CD_OPT_SORT_FULL        = 2,   /* 0 (default): hybrid -- 2 global passes on 16 key bits (44..59, or 48..63 when a key reaches 2^60), the rest of the high half */
                                   /*    sorted inside LDS windows, stable fix-up of equal-high-half runs; falls back to 2, then  */
                                   /*    to 1, by itself when a run is too long.  2: half-key -- 4 global passes + the fix-up.   */
                                   /*    1: all 8 digit passes.  All give the identical stable order by the full 64-bit key.     */
    CD_OPT_KERNEL_STAMPS    = 4,   /* with CD_OPT_STAGE_TIMING 0: which time stamps a fused call still takes, a bit mask -- 1: the block-build   */
                                   /*    kernel (cd_stats.ms_build_block), 2: the descent kernel (ms_descend), 4: the exact kernel (with 2:      */
                                   /*    ms_exact, ms_traverse), 8: pipeline start (with 2 and 4: ms_pipeline).  Default 15.  A stamp rides on   */
                                   /*    its kernel's dispatch packet and still costs ~5 us of idle GPU; a field whose stamps are off reads 0    */
    CD_OPT_STAGE_TIMING     = 3,   /* 1 (default): HIP events around every stage (cd_stats.ms_morton ... ms_refit); 0: only the  */
                                   /*    events of the pipeline as a whole and of the descent kernel (ms_pipeline, ms_traverse,   */
                                   /*    ms_descend, ms_exact) -- each stage boundary costs a few idle microseconds                */
    CD_OPT_GRAPH            = 5,   /* 1: cd_self_collide replays its steady-state step -- the nine kernel launches -- as ONE hipGraph launch, captured on   */
                                   /*    the first eligible call (CD_OPT_STAGE_TIMING 0, CD_OPT_KERNEL_STAMPS 0, default sort / build / traversal, a previous */
                                   /*    step done); anything a replay cannot answer (a sort flag, an overflow, a deep pass) falls back to the stream path.  */
                                   /*    Default 0: measured equal to the stream path within noise -- the host is ahead of the GPU either way */
    CD_OPT_POLL             = 6,   /* 1 (default): with no time stamp pending (CD_OPT_STAGE_TIMING 0 and CD_OPT_KERNEL_STAMPS 0) a step's end is read off a   */
                                   /*    sequence word the report kernel stores last into pinned host memory (the host spins on its own memory; after 20 ms,   */
                                   /*    and every 64th step anyway, it synchronises the stream; so do the first two steps into a report area or a pinned    */
                                   /*    pair buffer the device has not written before); 0: always hipStreamSynchronize                                      */
    CD_OPT_CELL_TABLE       = 7,   /* 1 (default): when the vertices are uploaded (cd_create, cd_update_vertices) and some coordinate is not an fp32 value, a table of the   */
                                   /*    vertices' fp32 cells is built (which cells hold two distinct doubles), so that the fp32 boxes of the traversal keep equal bounds  */
                                   /*    equal: touching boxes do not overlap after rounding (a full-double mesh then steps as fast as its float-rounded copy; the table  */
                                   /*    costs the upload ~0.4 ms per million vertices).  0: no table, every coordinate that is not an fp32 value is rounded outward    */
                                   /*    (a full-double structured mesh: ~2 x the step time, nothing added to the upload).  Vertices that are all fp32 values -- what   */
                                   /*    the reference's loader produces, load_obj.h:38 -- never have a table                                                            */
    CD_OPT_ORDER_HINT       = 8,   /* 1 (default): the half traversal (CD_OPT_TRAVERSAL 3) of a fused call takes its groups of 64 leaves longest-first (per XCD; the kernel ends with its    */
                                   /*    unluckiest wave slot), by how long the PREVIOUS traversal's waves took -- remembered per triangle, so that the hint survives a mesh that moves and  */
                                   /*    sorts differently: 1 M cloth at rest -7 us per step, sheets moving a quad per frame -4 us.  Scheduling only: every group is traversed in every      */
                                   /*    step, results do not depend on it.  Trees of more than 2048 blocks (1 M triangles) and the stage-wise API run in the plain order.  0: always the   */
                                   /*    plain order.  2: the hint for larger trees too (an XCD's list sorted chunk by chunk of 2048 groups; measured slower there: 8 M 454 -> 471 us)    */
    CD_OPT_QUERIES_PER_WAVE = 1    /* variant 1: queries one wave works through with dynamic lane refill (x64)         */
};
int cd_set_option(cd_ctx *ctx, int key, int64_t value);

/* Measurement hooks of tools/ and switches the tests use to ask for one code path or another -- NOT part of the interface that mirrors the
 * reference, free to change, and in a key space of their own so that none of them can be mistaken for an option above.  Setters take
 * `value` and return CD_OK; getters (CD_DBG_GET_*) write *out.  None of the setters changes results. */
enum {
    CD_DBG_LDS_PAD            = 0,   /* extra dynamic LDS bytes per traversal workgroup (occupancy experiments)                              */
    CD_DBG_EXACT_BLOCKS       = 1,   /* workgroups of the exact kernel (default 1024)                                                         */
    CD_DBG_NO_SHARED_PATH     = 2,   /* variant 1 without the shared root path                                                                */
    CD_DBG_DIAG               = 3,   /* run the descent kernel's DIAG instance: per-phase step counts and s_memtime ticks -> cd_debug_counters */
    CD_DBG_STAGEWISE_BUILD    = 4,   /* fused entry points build the tree stage by stage (k_hierarchy + refit) instead of in one pass         */
    CD_DBG_SPLIT_CROSS        = 5,   /* the fused build's cross nodes by k_cross_meta + k_cross_records instead of k_cross_fused               */
    CD_DBG_REPORT_COPIES      = 6,   /* 1: the report kernel copies the first pairs into the host buffer (32 workgroups), as before round 4, instead of the exact kernel posting them (A/B) */
    CD_DBG_SORT_WINDOWS       = 7,   /* the in-LDS window sort behind the two global passes: 0 (default) windows of 2048 keys (512 threads, two workgroups a CU) until a run is too long   */
                                     /* for them, then 4096; 1 always windows of 4096 keys (one 1024-thread workgroup a CU); 2 always 2048.  Same keys and permutation either way (A/B, tests) */
    CD_DBG_GET_SORT_FORM      = 8,   /* the form the next sort takes: 0 two global passes on key bits 44..59 + window sorts (default), 1 the same on bits 48..63 (a key beyond 2^60: a  */
                                     /* centroid outside the Morton frame; retried as 0 every 64 sorts), 2 four passes + fix-up, 3 all eight passes (runs too long for the forms before)   */
    CD_DBG_STORE_QBOX         = 9,   /* 1: the fused build always stores the per-leaf query boxes (qbox[]); default 0: only when a reader is known -- the half traversal and the cross    */
                                     /* nodes take leaf boxes out of the records (round 6: 32 of the block build's 106 bytes a leaf).  Same records, same results (A/B, tests)              */
    CD_DBG_POLL_SCAN          = 10,  /* polled completion: poison the pair area before a step, scan it the moment the sequence word is seen   */
    CD_DBG_GET_POLL_STALE     = 11,  /* ... steps in which the scan found a pair missing (must stay 0)                                        */
    CD_DBG_GET_POLL_FALLBACKS = 12,  /* ... polled waits that ran into the 20 ms budget and ended in a stream synchronise                     */
    CD_DBG_GET_POLLED_STEPS   = 13,  /* ... reports whose end was read off the sequence word                                                  */
    CD_DBG_GET_POLL_FB_WHY    = 16,  /* ... why those waits ran out: bits 0..15 the stream was still busy at the time-out (the step was late), 16..31 the stream had drained and    */
                                     /* the word came with the synchronise (late in flight), 32..47 the word was not there after the drain (LOST: must stay 0)                          */
    CD_DBG_GET_POLL_MAX_WAIT_US = 17, /* ... the longest polled wait that ended in the word (sampled every 16th step), microseconds                                                   */
    CD_DBG_BIG_OFFSETS        = 18,  /* 1: the half traversal runs the instance that forms 64-bit record addresses (what trees of more than 2^27 leaves get) on a tree of any size (tests)  */
    CD_DBG_GET_GRAPH_CAPTURES = 19,  /* ... CD_OPT_GRAPH: steps captured as a graph on this context so far (a captured step kept across other calls: no new capture)    */
    CD_DBG_GET_GRAPH_REPLAYS  = 20,  /* ... CD_OPT_GRAPH: graph launches of captured steps so far                                              */
    CD_DBG_GET_TREE_WAS_FUSED = 14,  /* 1: the tree that is there was made by the one-pass build                                              */
    CD_DBG_GET_ORDER_STATE    = 15,  /* the order hint (CD_OPT_ORDER_HINT) as it stands: 0 none built yet; 1 a permutation of the groups of 64 leaves that differs from the plain order;    */
                                     /* 2 the plain order itself; -1 not a permutation (must never be)                                                                                        */
    CD_DBG_SORT_CELLS         = 21,  /* how sort forms 0 and 1 order their 16 global key bits: 0 (default) by the previous step's statistic -- one launch that places every key by its cell  */
                                     /* (k_cell_scatter) where the cell changes 8 times or fewer, on average, along 64 consecutive triangles, else the two onesweep passes; a context's first */
                                     /* step and the step after a redo take the passes; 1 always the passes; 2 always the cells.  Same keys and permutation either way (A/B, tests)           */
    CD_DBG_GET_SORT_CELLS     = 22,  /* ... 1: the last sort ordered its global bits by cells, 0: by the two passes                                                                            */
    CD_DBG_GET_CELL_STAT      = 23   /* ... the statistic of the last step: the cell changes along each 64 consecutive triangles (a group's first counts), summed over the ceil(n / 64) groups */
};
int cd_debug_option(cd_ctx *ctx, int key, int64_t value, int64_t *out);

int cd_get_stats(cd_ctx *ctx, cd_stats *out);
/* Diagnostics of the last traversal, filled only after cd_debug_option(ctx, CD_DBG_DIAG, 1, NULL): sums over the descent's waves of
 * {chain steps, chain hops inside / outside the query's 256-leaf block, descent visits inside / outside it, longest
 * chain of each wave, 6 spare}.  Not part of any result. */
int cd_debug_counters(cd_ctx *ctx, unsigned long long out[12]);
/* The order hint's arrays (CD_OPT_ORDER_HINT), any may be NULL: per group of 64 leaves (ceil(nt / 64) words each) the score the last fused build gave it and the order
 * made from the scores (CD_ERR_ORDER while the tree that is there has none); per triangle, by its index in the face list (nt bytes), the time class (1.28 us each) its
 * wave left in the last half traversal.  Not part of any result. */
int cd_debug_hint(cd_ctx *ctx, uint32_t *cost, uint32_t *order, uint8_t *tri);
/* ... and the other way: install `order` (a permutation of the groups, checked: CD_ERR_ARG otherwise) as the hint the next half traversal of the tree that is there takes
 * (experiments with predictors: build the tree with cd_build_tree, install, cd_find_collisions). */
int cd_debug_hint_set(cd_ctx *ctx, const uint32_t *order);
/* Diagnostics: the fp32 traversal records of the current tree as the descent reads them -- recs: n x 64 bytes (n x 32 bytes
 * of right halves {lo[3], hi[3], link, last | flags}, then n x 32 bytes of left halves {lo[3], hi[3], link, first}, both
 * indexed by split), qboxes: n x 32 bytes {lo[3], hi[3], flags, 0}, root: the root record's split.  Either may be NULL. */
int cd_debug_records(cd_ctx *ctx, void *recs, void *qboxes, int32_t *root);
/* Diagnostics: the swept tree of the last continuous collision pass as its descent read it.  between = 0: this context's own, left by
 * cd_find_ccd / cd_self_ccd; between = 1: the other mesh's, as this context (a) holds it after cd_find_ccd_between (n = b's triangles).
 * recs: n x 64 bytes in the layout of cd_debug_records (box floats: the swept boxes, true bounds; links and range words: the static
 * records'), up: 2n - 1 words, up[j] for leaf j and up[n + s] for the node named by split s = (parent split << 1) | side, -1 for the
 * root; both are left untouched when n = 1 (no records).  m_bits: the fp32 bits of M the descent made its pad from, n_leaves: n.
 * pad: NOT device data -- the descent computes its pad in registers; this is the host twin of that computation (the same FP64 sum
 * of dist and M, rounded up to fp32).  Any may be NULL.  CD_ERR_ORDER before the first such pass.  Nothing is launched. */
int cd_debug_swept(cd_ctx *ctx, int between, void *recs, int32_t *up, uint32_t *m_bits, float *pad, uint32_t *n_leaves);
int cd_num_triangles(cd_ctx *ctx, uint32_t *nt);

/* ---- multi-GPU cross-rank pass (new work defined by the north star; no reference call site) ----
 * Query record, 88 bytes, device resident: the three vertices, the triangle ID and its three GLOBAL
 * vertex indices (neighborCount, triangle.cuh:18-30, compares indices). */
typedef struct cd_query {
    double   v[9];
    uint32_t id;
    uint32_t vidx[3];
} cd_query;

/* Global id of local vertex 0 (default 0).  Local triangles index the context's own vertex array;
 * across ranks neighborCount must compare GLOBAL vertex ids, so cd_pack_queries adds this base to the
 * indices it emits and cd_find_collisions_queries adds it to the local leaves' indices before comparing. */
int cd_set_vertex_id_base(cd_ctx *ctx, uint32_t base);
/* AABB of the whole local tree (box of internal node 0). */
int cd_root_box(cd_ctx *ctx, double box[6]);
/* Compact the local leaves whose AABB strictly overlaps `box` (box.cuh:40-43) into d_out, a DEVICE
 * buffer of cap records owned by the caller (e.g. a torch tensor handed to RCCL). *n = number found
 * (may exceed cap -> CD_OVERFLOW, nothing beyond cap is written). */
int cd_pack_queries(cd_ctx *ctx, const double box[6], void *d_out, uint64_t cap, uint64_t *n);
/* Traverse nq external queries (DEVICE buffer of cd_query) against the local tree; a pair
 * (q.id, leaf.id) is reported when q.id < leaf.id (tri_contact.cuh:81), no shared vertex index and
 * the exact test passes.  Output as cd_find_collisions. */
int cd_find_collisions_queries(cd_ctx *ctx, const void *d_queries, uint64_t nq,
                               uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs);

/* ---- the multi-GPU step in C/C++ behind the ABI (the harness it slots into is main.cu:47-174) ----
 * One process per GPU, one cd_ctx per process holding that rank's object(s) with GLOBAL triangle IDs and a vertex-id
 * base (cd_set_vertex_id_base).  A step = box of the rank's triangles -> ncclAllGather of the boxes -> one pack launch for
 * all overlapping peers (straight from the triangles) -> ncclAllGather of the per-peer counts -> grouped ncclSend / ncclRecv
 * of the records, WHILE the rank sorts, builds and traverses its own tree -> the received queries against that tree.
 * The one decision that makes the ranks repeat part of the step together (slab capacity) is taken from data all ranks
 * hold, so no rank is left waiting in a collective.  RCCL is loaded at run time (dlopen "librccl.so"; the environment
 * variable MI355CD_RCCL_LIBRARY names another library that provides the same ten calls). */
typedef struct cd_multi cd_multi;
enum {
    CD_MULTI_SELF_PEER = 1,    /* test mode: a rank also exchanges with ITSELF (ncclSend / ncclRecv to its own rank), so a    */
                               /* 1-rank communicator exercises every phase; the cross pass then reports the local pairs again */
    CD_MULTI_TIMING    = 2,    /* record HIP events at the phase boundaries (cd_multi_info.ms_*); costs a few idle us each     */
    CD_MULTI_CROSS_SERIAL = 8, /* A/B switch: the pass over the received queries runs behind the local traversal on its stream  */
                               /* instead of beside it on the second stream                                                     */
    CD_MULTI_SELF_SLICE = 4,   /* with CD_MULTI_SELF_PEER: the rank exchanges only the tenth of its triangles at its upper x end */
                               /* with itself -- a one-GPU rehearsal at the scale of a 10 % neighbour overlap                  */
    CD_MULTI_PRIORITY_STREAM = 32, /* at creation only: the second stream (all-gathers, pack, send / receive, the pass over the received queries) gets the */
                               /* device's highest stream priority.  Measured on one GPU (self-peer rehearsal, 1 M triangles): the two streams' kernels */
                               /* then slow each other down -- 0.65 against 0.32 ms per step -- so it is off by default                                     */
    CD_MULTI_INJECT_FAILURE = 16, /* test hook: this rank's NEXT step fails locally (CD_ERR_INJECTED) before its pipeline starts; the flag */
                               /* clears itself.  Every other rank must return CD_ERR_PEER from the same step, none may block      */
    CD_MULTI_INJECT_ALLOC_FAILURE = 64 /* test hook: this rank's NEXT allocation of its send / receive slabs fails (as out of memory); the flag   */
                               /* clears itself.  The step in which that happens fails on every rank; the next one allocates again   */
};
typedef struct cd_multi_info {
    uint32_t world, rank;          /* as the communicator reports them                                        */
    uint32_t n_peers;              /* ranks this rank sent to or received from                                */
    uint32_t host_syncs;           /* host synchronisations of the step (2 unless a pass had to be redone)    */
    uint32_t attempts;             /* 1 + collective repeats (slabs grown)                                    */
    uint32_t failed_rank_plus1;    /* a step that returned CD_ERR_PEER / a local error: 1 + the lowest rank that published a failure, else 0 */
    uint64_t sent_queries, recv_queries, local_pairs, cross_pairs, pairs_tested, query_cap;
                                   /* pairs_tested (here and in cd_stats after the step): both passes', and summed over the ranks what ONE tree of  */
                                   /* all their triangles tests.  For that sum a rank of a single triangle -- no tree, its local pass tests nothing -- */
                                   /* adds the one hit of that leaf on itself (when its box has an interior) that the single tree's walk counts.     */
                                   /* cd_stats.stack_overflows after the step: the deferred items of both passes of THIS step (0 when neither       */
                                   /* pass deferred), not the last traversal's alone.                                                                */
    float ms_tree, ms_allgather, ms_pack, ms_counts, ms_exchange, ms_local, ms_cross;   /* CD_MULTI_TIMING; -1 = not measured.  NOT additive: */
                                   /* first stream: tree (Morton keys .. fused build), local (own traversal); second stream, beside them: allgather  */
                                   /* (from the step's start: box of the triangles + its all-gather), pack, counts (all-gather + copy to the host),  */
                                   /* exchange (send / receive), cross (end of the exchange -> end of the pass over the received queries)            */
    float pad1;
} cd_multi_info;
/* ncclGetUniqueId: 128 bytes, produced on one rank and handed to all (by whatever the launcher has: MPI, a file, ...). */
int cd_multi_unique_id(void *id128);
/* ncclCommInitRank(world, id, rank) on the current HIP device + the step's buffers.  COLLECTIVE: every rank of the communicator
 * calls it.  query_cap_per_peer: records per peer slab (0 = nt / 8 + 1024); the ranks agree on the LARGEST request here (one
 * 8-byte all-gather), so shards of unequal size start from a common capacity; it grows collectively when a step needs more.
 * One cd_multi per context (CD_ERR_ORDER otherwise).  Lifetime: cd_multi_destroy before cd_destroy; a context destroyed first
 * detaches the cd_multi, whose further steps return CD_ERR_ORDER.
 * Failure semantics of cd_multi_step: a rank whose own work fails still joins the step's collectives and publishes its error in
 * the count matrix; every rank then returns from the SAME step -- the failing rank its error, the others CD_ERR_PEER -- before
 * any send / receive is posted.  An error met after that point is returned to its caller and published by that rank's next step.
 * NOT covered by "every rank returns from the same step": (i) a rank whose RCCL all-gather cannot even be ENQUEUED (ncclAllGather
 * returns an error on that rank alone) -- its peers are inside the collective, the communicator is dead, and only destroying it
 * ends their wait; (ii) CD_ERR_ORDER / CD_ERR_RCCL / CD_ERR_ARG returned at the entry of cd_multi_step (context destroyed, no RCCL
 * library, null handle) and a failure of cd_multi_create before its small agreement buffers exist: those ranks never reach a collective,
 * so their peers must not call into one either -- these are programming or installation errors every rank of a job shares.
 * A failed allocation of the send / receive slabs (creation or growth) IS covered: the rank keeps its old buffers, publishes the
 * error, and allocates again at the start of its next step. */
int cd_multi_create(cd_multi **out, cd_ctx *ctx, const void *id128, int rank, int world, uint64_t query_cap_per_peer, int flags);
/* The same over a communicator the caller owns (an opaque ncclComm_t); it is not destroyed by cd_multi_destroy. */
int cd_multi_create_from_comm(cd_multi **out, cd_ctx *ctx, void *nccl_comm, uint64_t query_cap_per_peer, int flags);
void cd_multi_destroy(cd_multi *m);
/* Change CD_MULTI_* flags between steps (e.g. untimed steps first, then a few with CD_MULTI_TIMING). */
int cd_multi_set_flags(cd_multi *m, int flags);
/* One step.  pairs: local pairs first, then the cross pairs this rank owns (output format of cd_find_collisions);
 * returns CD_OVERFLOW when they do not fit cap_pairs (*n_pairs holds the true count).  info may be NULL. */
int cd_multi_step(cd_multi *m, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs, cd_multi_info *info);

/* ---- self-proximity (not reference behaviour) ----
 * tri_distance(A, B): 0 when the pair is in contact as cd_find_collisions decides it -- the FP64 boxes overlap strictly (box.cuh:40-43)
 * and tri_contact(A, B) holds (the 17-axis test of cd_tri_contact_points) -- so a pair the library calls in contact is always at
 * distance 0; otherwise the square root of the minimum squared distance over the 15 feature pairs (6 vertex-triangle, 9 edge-edge),
 * evaluated in FP64 with a fixed operation order (csrc/cd_math.h).  A degenerate triangle (zero area, collinear, a single point) has
 * the distance of the point set it is, except in a pair the library calls in contact: between two degenerate triangles (or a segment
 * lying in a triangle's plane) the 17-axis test can say "contact" for triangles apart, and when their boxes also overlap strictly
 * cd_find_collisions reports them -- such a pair is at 0.  Finite inputs never give NaN.  Non-finite vertices: the result is undefined.
 *
 * Every unordered pair of triangles (a, b) of this context with no shared vertex index (neighborCount < 1, as collision.cuh:38) and
 * tri_distance(a, b) <= dist.  pairs: interleaved (smaller ID, larger ID), unordered, as cd_find_collisions; tri_distance is evaluated
 * with the smaller ID's triangle as A (equal IDs: the smaller face index).  dists (may be NULL): dists[k] = tri_distance of pairs[k].
 * n_tested (may be NULL): exact distance evaluations made.  Needs a tree built from the current vertices (CD_ERR_ORDER otherwise,
 * including after cd_update_vertices without a rebuild).  dist must be finite and >= 0 (CD_ERR_ARG otherwise).  Returns CD_OVERFLOW
 * with the true *n_pairs when it exceeds cap_pairs; nothing is written past cap_pairs (pairs may be NULL with cap_pairs 0).
 * The result depends on the mesh and dist only: not on the Morton frame, CD_OPT_TRAVERSAL, CD_OPT_CELL_TABLE or how the tree was
 * built.  Scaling the mesh and dist by a power of two scales the distances and nothing else while the largest |coordinate| lies within
 * about 2^-320 .. 2^260 (fp32 overflow and subnormals included); beyond, the contact predicate that puts a pair
 * at 0 overflows or underflows as the reference's does, and the results follow it.  These calls leave cd_stats, the last collision pair list (cd_sorted_pairs, cd_collision_triangles) and a captured
 * CD_OPT_GRAPH step as they were; they keep device buffers of their own. */
int cd_find_proximity(cd_ctx *ctx, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs,
                      uint64_t *n_pairs, uint64_t *n_tested);
/* cd_build_tree + cd_find_proximity, queued back to back, one host synchronisation. */
int cd_self_proximity(cd_ctx *ctx, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs,
                      uint64_t *n_pairs, uint64_t *n_tested);
/* tri_distance on explicit positions (host pointers; no context): tri is n x 6 x 3 doubles (A's three vertices, then B's), as
 * cd_tri_contact_points.  The pin of the device function. */
int cd_tri_distance_points(const double *tri, uint64_t n, double *dist);

/* ---- continuous collision queries (not reference behaviour) ----
 * Vertices move linearly from x0 (this context's vertices, the tree's) to x1 = verts_end (host pointer, nv x 3 doubles, the layout of
 * cd_create's; uploaded by the call, never installed into the context): p(t) = p0 + t * (p1 - p0) per coordinate, t in [0, 1].
 * Every unordered pair (A, B) with no shared vertex index (as proximity), A the smaller ID (equal IDs: the smaller face index), whose
 * FP64 swept boxes (the box of each triangle's six points, x0 and x1) widened by dist (lo - dist, hi + dist) overlap (closed), is run
 * through conservative advancement with report threshold dist and target h = dist / 2:
 *   L = (max_i |dA_i - g| + max_j |dB_j - g|) (1 + 2^-20), d = p1 - p0 per vertex, g the mean of the six d;
 *   t = 0, d = tri_distance on x0 itself; then: d <= dist -> reported (t, d); L == 0 -> not reported; CCD_MAX_EVALS (1024)
 *   evaluations made -> reported UNRESOLVED (t, d) with d > dist; t' = t + (d - h) / L >= 1 -> one evaluation on x1 itself,
 *   reported (1, d1) when d1 <= dist, else not; otherwise t = t', d = tri_distance at p(t), again.
 * Guarantee: a pair whose exact linearly moving triangles come closer than h - delta (delta ~ 2^-38 of the pair's largest |coordinate|)
 * at some t* is reported with toi <= t*, and stays at least h - delta apart before toi.  The pairs with toi == 0 are cd_find_proximity's
 * on x0 with the same distances (for dist >= 2^-30 of the largest |coordinate|); every pair of cd_find_proximity on x1 is reported.
 * Scaling x0, x1 and dist by a power of two keeps the pairs and toi and scales the distances within cd_find_proximity's band of
 * coordinate magnitudes.
 * pairs: interleaved (smaller ID, larger ID), unordered; toi[k], dists[k] (either may be NULL): its time and distance.
 * info (may be NULL): candidates of the broad phase, pairs through the gate, tri_distance evaluations, unresolved pairs reported.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise).  dist must be finite and > 0, verts_end not NULL (CD_ERR_ARG
 * otherwise).  Returns CD_OVERFLOW with the true *n_pairs when it exceeds cap_pairs; nothing is written past cap_pairs.  These calls
 * leave the context's vertices, cd_stats, the last collision pair list, a captured CD_OPT_GRAPH step and the proximity buffers as they
 * were; they keep device buffers of their own. */
typedef struct cd_ccd_info { uint64_t n_candidates, n_tested, n_evals, n_unresolved; } cd_ccd_info;
int cd_find_ccd(cd_ctx *ctx, const double *verts_end, double dist, uint32_t *pairs, double *toi, double *dists,
                uint64_t cap_pairs, uint64_t *n_pairs, cd_ccd_info *info);
/* cd_build_tree on x0 + cd_find_ccd, queued back to back, one host synchronisation. */
int cd_self_ccd(cd_ctx *ctx, const double *verts_end, double dist, uint32_t *pairs, double *toi, double *dists,
                uint64_t cap_pairs, uint64_t *n_pairs, cd_ccd_info *info);
/* The per-pair advancement on explicit positions (host pointers; no context; no gate): tri is n x 36 doubles, A's three vertices then
 * B's at x0, then the same at x1.  toi[k] = +inf: not reported (dists[k] = the last distance evaluated); evals[k]: tri_distance
 * evaluations.  The pin of the device function. */
int cd_ccd_points(const double *tri, uint64_t n, double dist, double *toi, double *dists, uint32_t *evals);

/* ---- queries between two meshes (not reference behaviour) ----
 * The three questions above, asked of the triangles of context a against those of context b (two objects: a cloth and a body, an
 * obstacle, another garment).  A pair is (a's triangle, b's triangle), written (ID in a, ID in b) with each context's own IDs from
 * cd_create -- NOT reordered by ID; rows unordered, as cd_find_collisions.  The two contexts have separate vertex arrays, so there is
 * no neighbour filter, and cd_set_vertex_id_base plays no part.  Every per-pair predicate takes a's triangle as its first argument
 * (P / A); the self queries put the smaller ID there instead.  So between(a, b) is exactly the set of cross pairs of the self query on
 * the merged mesh whose triangles are a's first, with the smaller IDs, and whose vertices are a's, then b's offset by a's nv.
 *   contact   : the FP64 boxes overlap strictly (box.cuh:40-43) and tri_contact(a, b) holds.  n_tested (may be NULL): the (a, b) pairs
 *               whose FP64 boxes overlap strictly -- a number of the meshes alone.
 *   proximity : tri_distance(a, b) <= dist, tri_distance as cd_find_proximity defines it (a pair in contact, as the contact query
 *               decides it, is at 0).  dists (may be NULL).  n_tested (may be NULL): exact distance evaluations made.
 *   CCD       : cd_find_ccd's definition -- the FP64 swept-box gate widened by dist, conservative advancement with h = dist / 2,
 *               CCD_MAX_EVALS, unresolved pairs reported with d > dist -- with x0 each context's current vertices and x1 verts_end_a /
 *               verts_end_b (host pointers, the layout of cd_create's).  NULL: that mesh does not move (x1 = x0; a static obstacle);
 *               both may be NULL.  toi, dists, info (each may be NULL) mean what they mean for cd_find_ccd.
 * Errors: CD_ERR_ARG when a context is NULL, a == b (self queries have their own calls), the two contexts were created on different
 * HIP devices, or dist fails the rule of the self call (proximity: finite and >= 0; CCD: finite and > 0).  CD_ERR_ORDER unless BOTH
 * contexts have a tree built from their current vertices (cd_update_vertices without a rebuild counts as not built).  CD_OVERFLOW with
 * the true *n_pairs when the pairs do not fit cap_pairs; nothing is written past cap_pairs (pairs may be NULL with cap_pairs 0).
 * Guarantee: the result depends on the two meshes and dist only -- not on either context's Morton frame, CD_OPT_TRAVERSAL,
 * CD_OPT_CELL_TABLE or build variant, nor on which context's tree is walked.  The calls leave both contexts' state as it was: cd_stats,
 * the last pair list (cd_sorted_pairs, cd_collision_triangles), a captured CD_OPT_GRAPH step, the proximity and CCD buffers.  Their
 * device buffers belong to context a (grown on demand; cd_destroy frees them) and they run on a's stream.  Neither context may be used
 * by another thread during the call. */
int cd_find_collisions_between(cd_ctx *a, cd_ctx *b, uint32_t *pairs, uint64_t cap_pairs,
                               uint64_t *n_pairs, uint64_t *n_tested);
int cd_find_proximity_between(cd_ctx *a, cd_ctx *b, double dist, uint32_t *pairs, double *dists,
                              uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested);
int cd_find_ccd_between(cd_ctx *a, const double *verts_end_a, cd_ctx *b, const double *verts_end_b, double dist,
                        uint32_t *pairs, double *toi, double *dists, uint64_t cap_pairs, uint64_t *n_pairs,
                        cd_ccd_info *info);

/* ---- the closest points of proximity and CCD pairs: the witness (not reference behaviour) ----
 * tri_witness(A, B) -> (dist, feature_a, feature_b, ua, va, ub, vb, qa, qb): WHERE on the two triangles tri_distance(A, B) is attained.
 * FP64 in tri_distance's frame (translate to A's first vertex, scale by 2^-ex with |ex| clamped at 1000), with tri_distance's blocks and
 * operation order, IEEE divide and sqrt, no contraction (csrc/cd_math.h):
 *   dist = tri_distance(A, B), bit for bit: sqrt(best) 2^ex -- not |qa - qb| recomputed.
 *   A pair tri_distance puts at 0 through its early-outs -- the FP64 boxes overlap strictly and tri_contact holds, or the six points
 *   coincide -- has NO witness: feature_a = feature_b = 7 and every other output except dist is 0.  Interpenetration is CCD's to
 *   prevent; a pair in contact has no closest points.
 *   Otherwise the 33 terms of tri_distance are taken in this order, term 11 i + k for i = 0, 1, 2 (P = A, Q = B):
 *     k = 0         pt_face2(P_i; Q)      vertex i of A against B's face interior
 *     k = 1         pt_face2(Q_i; P)      vertex i of B against A's face interior
 *     k = 2, 3, 4   pt_seg2(P_i; Q's edges 01, 12, 20)
 *     k = 5, 6, 7   pt_seg2(Q_i; P's edges 01, 12, 20)
 *     k = 8, 9, 10  seg_seg2(P's edge (i, i+1); Q's edges 01, 12, 20), the interior critical point of the two segments
 *   and a later term replaces the running minimum only when it is STRICTLY smaller (an earlier term keeps a tie).  The distance does
 *   not depend on that order; the witness does, so the order and the tie rule are part of this contract.
 *   What the winning term gives, in pt_tri's coding (0 face, 1 / 2 / 3 edge 01 / 12 / 20, 4 / 5 / 6 vertex 0 / 1 / 2):
 *     a vertex i:  (u, v) = (0, 0), (1, 0), (0, 1);  feature 4 + i
 *     a face:      (u, v) = (fv, fw) of the face block (as pt_tri's);  feature 0
 *     an edge e with parameter t measured from vertex e (the clamped t of the segment block; for seg_seg2 its s on A's edge (i, i+1)
 *     from vertex i and its t on B's edge), exactly pt_tri's table:
 *       edge 01: (t, 0);  edge 12: (1 - t, t);  edge 20: (0, 1 - t);  feature 1 + e, or the vertex's code when t == 0 or t == 1
 *   qa = (wa A0 + ua A1) + va A2 per coordinate with wa = (1 - ua) - va, on the ORIGINAL vertices, as pt_tri forms q; qb likewise on B.
 * Finite input gives no NaN.  Both points lie on their triangles: u, v >= 0 and u + v <= 1 up to the rounding of 1 - t.
 * | |qa - qb| - dist | <= 2^-48 M with M the largest |coordinate| of the six vertices (a numpy prototype measured at most 2^-50.4 M
 * over 1.2 M pairs: unit soups, near pairs, pairs offset by 1e6 and by 2^40, integer-grid ties, slivers; tests/test_witness_ref.py
 * re-checks it on every input the tests use).  Scaling all six vertices by 2^k scales dist, qa and qb exactly and changes nothing in
 * the features or (u, v) over cd_find_proximity's band.
 *
 * The four calls below are cd_find_proximity, cd_find_proximity_between, cd_find_ccd and cd_find_ccd_between with one trailing
 * argument.  Each member of w holds cap_pairs rows -- faces 2, points 6 (qa, then qb), bary 4 (ua va ub vb), feature 2 elements a row
 * -- and may be NULL; a NULL w (or one whose members are all NULL) makes the call the plain one.  Row k describes pairs[k]:
 *   faces[2 k], faces[2 k + 1]: the indices in cd_create's face list of the triangles that played A and B.  Self calls: A is the
 *   smaller ID, then the smaller face index.  Between calls: A is a's triangle, and each index is into its own context's list.  (With
 *   custom or repeated IDs this is what tells which face a reported ID is.)
 *   The rest is tri_witness(A, B), evaluated with the arguments of the row's distance: dists[k] is the witness's dist, bit for bit.
 *   CCD: the witness is taken at the evaluation that reported the pair -- also for an unresolved pair, at its last evaluation, with
 *   d > dist.  The positions are x1 itself when toi[k] == 1, otherwise a + toi (b - a) per coordinate as the advancement forms p(t)
 *   (x0's values at toi == 0).
 * Everything else follows the plain calls: the errors, CD_OVERFLOW with the true *n_pairs and nothing written past cap_pairs in any
 * array, the "depends on the meshes and dist only" guarantee (per row: the order of the rows is as free as the plain calls'), the
 * context state the call leaves as it was.  The calls keep device buffers of their own (grown on demand; cd_destroy frees them) and
 * cost one more kernel over the reported pairs and one more host synchronisation. */
typedef struct cd_witness_out { uint32_t *faces; double *points; double *bary; uint8_t *feature; } cd_witness_out;
int cd_find_proximity_witness(cd_ctx *ctx, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs,
                              uint64_t *n_pairs, uint64_t *n_tested, const cd_witness_out *w);
int cd_find_proximity_between_witness(cd_ctx *a, cd_ctx *b, double dist, uint32_t *pairs, double *dists,
                                      uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested, const cd_witness_out *w);
int cd_find_ccd_witness(cd_ctx *ctx, const double *verts_end, double dist, uint32_t *pairs, double *toi, double *dists,
                        uint64_t cap_pairs, uint64_t *n_pairs, cd_ccd_info *info, const cd_witness_out *w);
int cd_find_ccd_between_witness(cd_ctx *a, const double *verts_end_a, cd_ctx *b, const double *verts_end_b, double dist,
                                uint32_t *pairs, double *toi, double *dists, uint64_t cap_pairs, uint64_t *n_pairs,
                                cd_ccd_info *info, const cd_witness_out *w);
/* tri_witness on explicit positions (host pointers; no context): tri is n x 18 doubles as for cd_tri_distance_points.  dist[k];
 * points[6 k ..]: qa, then qb; bary[4 k ..]: ua va ub vb; feature[2 k], feature[2 k + 1].  Every output except dist may be NULL.  The
 * pin of the device function. */
int cd_tri_witness_points(const double *tri, uint64_t n, double *dist, double *points, double *bary, uint8_t *feature);

/* ---- the intersection segment of pairs in contact: the contour (not reference behaviour) ----
 * The witness has nothing to say about a pair in contact (features 7 / 7).  For such a pair the answer is the segment in which the two
 * triangles cut each other: which edge of which triangle pierces the other's face, where on that edge and on that face, from which
 * side.  Chained over the pairs the segments are the intersection contour of the mesh(es).
 * tri_isect(A, B) -> (n, mask, two endpoints): six evaluations of ray_tri (the ray section below) in this order and a selection rule;
 * FP64, ray_tri's operation order, IEEE divide, no contraction, a NaN fails every comparison (csrc/cd_math.h):
 *   term k = 0, 1, 2: A's edge from A_k to A_(k+1 mod 3) against B's face (B0, B1, B2);
 *   term k = 3, 4, 5: B's edge from B_(k-3) to B_(k-2 mod 3) against A's face (A0, A1, A2);
 *   r_k = ray_tri(o, d, tmax = 1; p0, p1, p2) with o the edge's start and d = end - start per coordinate (one rounding).  On a hit
 *   x_k = o + t d per coordinate, the product rounded and then the sum: the point ray_tri's gate forms.
 *   mask: bit k is set when term k hit.
 *   No hit: n = 0, both endpoints have term 7 and everything else is 0 -- coplanar pairs (every edge is parallel to the other face),
 *   touching pairs that the gate or the range checks reject, degenerate triangles.
 *   One hit: n = 1; endpoint 0 is that term, endpoint 1 has term 7 and zeros.
 *   Two or more hits: n = 2.  The pairs (i, j), i < j, of hit terms are taken in lexicographic order, each with
 *   D = (dx dx + dy dy) + dz dz of x_i - x_j; a later pair replaces the kept one only when its D is STRICTLY larger (an earlier pair
 *   keeps a tie).  Endpoint 0 is i, endpoint 1 is j: the two hit points that lie farthest apart.  With exactly two hits -- every pair
 *   in general position -- these are the two hits in term order.
 *   Per endpoint: the term 0..5; ray_tri's t, the parameter along the piercing edge from its start; (u, v), the barycentrics on the
 *   pierced face (x = (1 - u - v) p0 + u p1 + v p2); side, 1 when the edge, in its direction, meets the face whose vertices run
 *   counter-clockwise as seen from the edge's start; the point x.
 * Finite input gives no NaN in any output.  Scaling all six vertices by 2^k scales x exactly and changes nothing else while the
 * coordinates stay inside ray_tri's band.  tri_isect(B, A) hits exactly the terms (k + 3) mod 6, with bit-identical t, u, v, side, x --
 * each term is the same ray_tri call; only the order of the two endpoints may differ.  Both endpoints lie on both triangles within
 * 2^-42 M, M the largest |coordinate| of the six vertices: a condition on the inputs, as the witness's bound (the numpy restatement
 * measured at most 2^-44.58 M over every input the tests use -- unit-cube pairs, pairs of diameter 0.2, the same offset by 2^20 + 0.37,
 * integer-grid pairs, slivers, degenerate triangles, the test meshes; tests/test_isect_ref.py re-checks it).  The definition applies no
 * contact test: a pair tri_contact rejects may have hits and a pair it accepts may have none (coplanar pairs); on inputs in general
 * position a pair in contact has exactly two.
 *
 * The two calls below are the contact queries with one trailing argument.  Each member of w holds cap_pairs rows -- faces 2, code 3,
 * param 6, points 6 elements a row -- and may be NULL.  Row k describes pairs[k]:
 *   faces[2 k], faces[2 k + 1]: the indices in cd_create's face list of the triangles that played A and B (with custom or repeated IDs
 *   this is what tells which face a reported ID is).
 *   code[3 k], code[3 k + 1]: endpoint 0 and endpoint 1 as term | side << 3, 7 for a missing endpoint;  code[3 k + 2]: the mask.
 *   param[6 k ..]: t, u, v of endpoint 0, then of endpoint 1.    points[6 k ..]: x of endpoint 0, then of endpoint 1.
 * cd_find_collisions_between_contour: the pair set, *n_tested, the errors and the overflow behaviour are cd_find_collisions_between's;
 * A is a's triangle and each face index is into its own context's list.  A NULL w (or one whose members are all NULL) makes it the
 * plain call.
 * cd_find_collisions_contour: as a set of (smaller ID, larger ID) rows the pair set is cd_find_collisions' on the same tree -- the FP64
 * boxes overlap strictly, no vertex index is shared, the IDs differ (pairs of equal IDs are never reported), and tri_contact holds with
 * the smaller ID's triangle as P.  A is the smaller ID's triangle.  *n_tested: the pairs that reach tri_contact (after the neighbour
 * filter, the ID rule and the strict box test), a number of the mesh alone -- not cd_stats' pairs_tested, which depends on the walk.
 * It needs a tree built from the current vertices (cd_build_tree, or a step): CD_ERR_ORDER otherwise.  CD_OVERFLOW with the true
 * *n_pairs when the pairs do not fit; nothing is written past cap_pairs in any array.  It is a pass of its own behind the tree, not
 * the collision path's: cd_stats, the last pair list (cd_sorted_pairs), the order hint, a captured step and every other query's
 * buffers stay as they were, and bench.py's step runs the kernels it ran before.  With a NULL w the call still runs and returns the
 * pairs: a second implementation of the pair set.
 * The result depends on the mesh(es) only, row by row (the order of the rows is free): not on the Morton frame, CD_OPT_TRAVERSAL, the
 * cell table or the build variant.  The calls keep device buffers of their own (grown on demand; cd_destroy frees them) and cost one
 * more kernel over the reported pairs and one more host synchronisation. */
typedef struct cd_contour_out { uint32_t *faces; uint8_t *code; double *param; double *points; } cd_contour_out;
int cd_find_collisions_contour(cd_ctx *ctx, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs,
                               uint64_t *n_tested, const cd_contour_out *w);
int cd_find_collisions_between_contour(cd_ctx *a, cd_ctx *b, uint32_t *pairs, uint64_t cap_pairs,
                                       uint64_t *n_pairs, uint64_t *n_tested, const cd_contour_out *w);
/* tri_isect on explicit positions (host pointers; no context): tri is n x 18 doubles as for cd_tri_contact_points.  code[3 k ..],
 * param[6 k ..], points[6 k ..] as above.  code is required; param and points may be NULL.  No finiteness check, no contact test, no
 * box test: the arithmetic decides.  The pin of the device function. */
int cd_tri_isect_points(const double *tri, uint64_t n, uint8_t *code, double *param, double *points);

/* ---- ray queries: closest hit and occlusion (not reference behaviour) ----
 * A ray is seven doubles: an origin o, a direction d and an upper end tmax.  o and d are finite and d is not all zero; d is NOT
 * normalised, so t is in units of d; 0 <= tmax <= +inf and the ray's parameter range is [0, tmax] (a segment from a to b: o = a,
 * d = b - a, tmax = 1).  ray_tri(ray, triangle p0 p1 p2), FP64 with a fixed operation order, IEEE divide and no contraction
 * (csrc/cd_math.h):
 *   e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1 . pv;  det == 0 -> miss (a parallel ray, or a degenerate triangle: segments
 *   and points are never hit);  inv = 1 / det, tv = o - p0;  u = (tv . pv) inv, u < 0 or u > 1 -> miss;  qv = tv x e1;
 *   v = (d . qv) inv, v < 0 or u + v > 1 -> miss;  t = (e2 . qv) inv, t < 0 or t > tmax -> miss;
 *   gate: P_a = o_a + t d_a per axis; G = 2^-30 max(|o_x|, |o_y|, |o_z|, the largest |coordinate| of p0, p1, p2); on every axis
 *   lo_a - G <= P_a <= hi_a + G with lo / hi the triangle's FP64 box (box.cuh:13-22), else miss;
 *   hit: (t, u, v, side), the hit point being (1 - u - v) p0 + u p1 + v p2; side = 1 when det > 0 (the ray meets the face whose
 *   vertices run counter-clockwise as seen from its origin), else 0.
 * There is no face culling, and any NaN produced on the way is a miss.  The gate rejects the hits that are rounding noise: on a sliver
 * the computed (t, u, v) can pass the range checks at a point nowhere near the triangle.  Scaling the ray and the triangle by 2^k
 * changes nothing in (t, u, v, side) while the largest |coordinate| stays within about 2^-300 .. 2^300 (products of three coordinate
 * differences must stay normal numbers; fp32 overflow and subnormals lie well inside that band); outside it the result follows the
 * arithmetic above, overflow included.
 *
 * cd_cast_rays, flags = 0 (closest hit): for ray k, of the triangles of this context that ray_tri hits, the one with the smallest
 * (t, triangle ID, face index) in lexicographic order -- so a ray through a shared edge or vertex has one defined answer.
 * face[k]: its index in cd_create's face list, 0xFFFFFFFF when nothing is hit; ids[k]: its ID; t[k], uv[2 k], uv[2 k + 1], side[k]:
 * ray_tri's values for it.  On a miss t[k] = +inf and the other outputs are 0.  ids, t, uv, side may each be NULL.
 * flags = CD_RAY_ANY (occlusion): face[k] = 0xFFFFFFFF for a miss and SOME triangle that ray_tri hits otherwise.  WHETHER there is one
 * is defined (exactly where the closest-hit call hits); WHICH one is returned is not (it depends on the tree and may change from
 * build to build).  ids, t, uv and side must be NULL.
 * info (may be NULL): rays that hit, boxes tested, ray_tri evaluations -- numbers of this tree, not of the mesh.
 * Guarantee: the closest-hit result depends on the mesh and the rays only -- not on the Morton frame, CD_OPT_TRAVERSAL,
 * CD_OPT_CELL_TABLE, the build variant or the order of the rays.  Rays are walked in the order given, one lane each, neighbours in
 * one wave: coherent rays (a camera's rows, a strand's segments) should be neighbours; the library does not sort them.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise, including after cd_update_vertices without a rebuild).
 * CD_ERR_ARG: a NULL context; NULL rays or face with n > 0; flags other than 0 / CD_RAY_ANY; with CD_RAY_ANY an output other than
 * face; a non-finite origin or direction, an all-zero direction, a tmax that is NaN or negative -- checked on the host before
 * anything is launched, and nothing is written then.  n = 0 returns CD_OK.  The call leaves cd_stats, the last pair list, the order
 * hint, a captured CD_OPT_GRAPH step and every other query's buffers as they were; it keeps device buffers of its
 * own (grown on demand; cd_destroy frees them) and runs on the context's stream with one host synchronisation. */
typedef struct cd_ray_info { uint64_t n_hits, node_visits, tri_tests; } cd_ray_info;
enum { CD_RAY_ANY = 1 };
int cd_cast_rays(cd_ctx *ctx, const double *rays, uint64_t n, int flags, uint32_t *face, uint32_t *ids, double *t,
                 double *uv, uint8_t *side, cd_ray_info *info);
/* ray_tri on explicit operands (host pointers; no context): ray is n x 7 doubles (o, d, tmax), tri n x 9 (p0, p1, p2).  hit[k] = 1 / 0;
 * t[k], uv[2 k], uv[2 k + 1], side[k] (each may be NULL): ray_tri's values, 0 on a miss.  No argument is checked for finiteness: the
 * arithmetic decides.  The pin of the device function. */
int cd_ray_tri_points(const double *ray, const double *tri, uint64_t n, uint8_t *hit, double *t, double *uv, uint8_t *side);

/* ---- closest-point queries: nearest triangle and within-radius (not reference behaviour) ----
 * A query point is four doubles (x, y, z, rmax): finite coordinates and a search radius 0 <= rmax <= +inf.
 * pt_tri(p; triangle p0 p1 p2) -> (dist, u, v, feature, side, q), FP64 with a fixed operation order, IEEE divide and sqrt and no
 * contraction (csrc/cd_math.h), built from tri_distance's blocks in tri_distance's frame:
 *   a = p0 - p, b = p1 - p, c = p2 - p (the query point becomes the origin O); m = the largest |component| of a, b, c;
 *   m == 0 (three coincident vertices at p): dist = 0, u = v = 0, feature = 4, side = 0, q = p0;
 *   else m = f 2^ex with f in [0.5, 1) and |ex| clamped at 1000; a, b, c are multiplied by 2^-ex (exact); then the minimum of four
 *   squared distances taken in this order, a later term replacing an earlier one only when strictly smaller (an earlier term keeps a tie):
 *     face:    with ab = b - a, ac = c - a, ap = O - a: d00 = ab.ab, d01 = ab.ac, d11 = ac.ac, d20 = ap.ab, d21 = ap.ac,
 *              den = d00 d11 - d01 d01; +inf unless den > 0; fv = (d11 d20 - d01 d21) / den, fw = (d00 d21 - d01 d20) / den; +inf unless
 *              fv >= 0, fw >= 0, fv + fw <= 1; the point (a + fv ab) + fw ac, its squared distance from O;  u = fv, v = fw, feature 0
 *     edge 01: segment (a, b): t = (ap.ab) / (ab.ab) clamped to [0, 1] (0 when ab.ab is not > 0), the point a + t ab;
 *              u = t, v = 0;      feature 1, or 4 (vertex 0) when t == 0, 5 (vertex 1) when t == 1
 *     edge 12: segment (b, c) likewise;   u = 1 - t, v = t;  feature 2, or 5 when t == 0, 6 (vertex 2) when t == 1
 *     edge 20: segment (c, a) likewise;   u = 0, v = 1 - t;  feature 3, or 6 when t == 0, 4 when t == 1
 *   (a dot product is (x x + y y) + z z);  dist = sqrt(best) 2^ex;  side = 1 when ap . (ab x ac) > 0 on the scaled operands, else 0;
 *   q = (w p0 + u p1) + v p2 per coordinate with w = (1 - u) - v, on the ORIGINAL vertices (not translated, not scaled).
 * (u, v) are the barycentrics of the closest point, q = (1 - u - v) p0 + u p1 + v p2; on an edge or vertex feature they are exactly the
 * 0 / t / 1 - t above.  feature 0 means the face term won -- the projection onto the plane lies in the CLOSED triangle -- so a point that
 * projects exactly onto an edge reports 0.  q is returned; callers need not recompute it.  side is the side of THIS triangle's plane
 * (1: the one that sees p0 p1 p2 counter-clockwise); on an edge or vertex feature it is NOT an inside / outside test of a surface.
 * A degenerate triangle has the distance of the segment or point it is (its face term is +inf).  Finite input never gives a NaN;
 * non-finite vertices give undefined results.  Scaling the point and the triangle by 2^k scales dist and q exactly and changes nothing
 * in (u, v, feature, side) over the band of cd_find_proximity (largest |coordinate| from about 2^-320 to 2^256 and beyond).
 *
 * cd_closest_points, flags = 0: for point k, of the triangles of this context with pt_tri's dist <= rmax, the one with the smallest
 * (dist, triangle ID, face index) in lexicographic order -- so a point equally far from two triangles (any point nearest to a shared
 * edge or vertex) has one defined answer.  face[k]: its index in cd_create's face list, 0xFFFFFFFF when no triangle is within rmax;
 * ids[k]: its ID; dist[k], closest[3 k ..], uv[2 k], uv[2 k + 1], feature[k], side[k]: pt_tri's values for it.  When nothing is within
 * rmax dist[k] = +inf and the other outputs are 0.  ids, dist, closest, uv, feature, side may each be NULL.
 * flags = CD_POINT_ANY (is anything within rmax?): face[k] = 0xFFFFFFFF when nothing is and SOME triangle with dist <= rmax otherwise.
 * WHETHER there is one is defined (exactly where the closest call finds one); WHICH one is returned is not (it depends on the tree and
 * may change from build to build).  ids, dist, closest, uv, feature and side must be NULL.
 * info (may be NULL): points that found a triangle, boxes tested, pt_tri evaluations -- numbers of this tree, not of the mesh.
 * Guarantee: the closest result depends on the mesh and the points only -- not on the Morton frame, CD_OPT_TRAVERSAL,
 * CD_OPT_CELL_TABLE, the build variant or the order of the points.  Points are walked in the order given, one lane each, neighbours in
 * one wave: spatially coherent points (a mesh's vertices in mesh order, a grid's rows) should be neighbours; the library does not sort them.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise, including after cd_update_vertices without a rebuild).
 * CD_ERR_ARG: a NULL context; NULL points or face with n > 0; flags other than 0 / CD_POINT_ANY; with CD_POINT_ANY an output other
 * than face; a non-finite coordinate, an rmax that is NaN or negative -- checked on the host before anything is launched, and nothing
 * is written then.  n = 0 returns CD_OK.  The call leaves cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH step and
 * every other query's buffers as they were; it keeps device buffers of its own (grown on demand; cd_destroy frees
 * them) and runs on the context's stream with one host synchronisation. */
typedef struct cd_point_info { uint64_t n_found, node_visits, tri_tests; } cd_point_info;
enum { CD_POINT_ANY = 1 };
int cd_closest_points(cd_ctx *ctx, const double *points, uint64_t n, int flags, uint32_t *face, uint32_t *ids, double *dist,
                      double *closest, double *uv, uint8_t *feature, uint8_t *side, cd_point_info *info);
/* pt_tri on explicit operands (host pointers; no context): points is n x 3 doubles (no radius), tri n x 9 (p0, p1, p2).  dist[k],
 * closest[3 k ..], uv[2 k], uv[2 k + 1], feature[k], side[k]: pt_tri's values; every output except dist may be NULL.  No argument is
 * checked for finiteness: the arithmetic decides.  The pin of the device function. */
int cd_pt_tri_points(const double *points, const double *tri, uint64_t n, double *dist, double *closest, double *uv,
                     uint8_t *feature, uint8_t *side);

/* ---- all-results point and ray queries: everything within a radius, every hit (not reference behaviour) ----
 * The complete sets behind cd_closest_points and cd_cast_rays: every triangle within a point's radius (vertex-face proximity for a
 * repulsion pass, radius selection) and every triangle a ray or segment crosses (entry and exit, crossing counts, ordered hits).
 * points is n x 4 doubles, exactly as cd_closest_points takes them (x, y, z, rmax with 0 <= rmax <= +inf); rays is n x 7 doubles,
 * exactly as cd_cast_rays takes them (origin, direction, tmax).
 *
 * cd_points_within: one row for every (point k, face f) of this context with pt_tri(p_k; f).dist <= rmax_k (closed).
 * cd_cast_rays_all: one row for every (ray k, face f) that ray_tri hits over [0, tmax_k].
 * Each (k, f) appears exactly once.  Row r: rows[2 r] = k, rows[2 r + 1] = f, the index in cd_create's face list.  The order of the
 * rows is free, as it is for cd_find_collisions; callers that want them grouped sort them.  out (may be NULL, and so may each of its
 * members), per row: ids[r] the face's ID; dist[r], closest[3 r ..], uv[2 r], uv[2 r + 1], feature[r], side[r]: pt_tri's values for
 * (k, f); t[r], uv[2 r], uv[2 r + 1], side[r]: ray_tri's.
 * *n_rows is the size of the set.  When it exceeds cap_rows the call returns CD_OVERFLOW with the true *n_rows; nothing is written at
 * or past cap_rows in any array, and the rows that are written are distinct rows of the true set.  rows may be NULL with cap_rows 0:
 * the count-only call.  n_tested (may be NULL): exact evaluations made -- a number of this tree, not of the mesh.
 * Guarantee: the set of rows and every value in a row depend on the mesh and the items only -- not on the Morton frame,
 * CD_OPT_TRAVERSAL, CD_OPT_CELL_TABLE, the build variant or the order of the items.  Consistency with the single-answer calls is by
 * definition: for item k the row with the smallest (dist, ID, face) -- for rays (t, ID, face) -- is bit for bit what cd_closest_points /
 * cd_cast_rays with flags = 0 returns for k, and the items with no row are exactly those calls' 0xFFFFFFFF items.
 * Items are walked in the order given, one lane each, neighbours in one wave: coherent items should be neighbours.  An item whose bound
 * meets every box (rmax = +inf) walks the whole tree in one lane: correct, bounded, and slow.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise, including after cd_update_vertices without a rebuild).
 * CD_ERR_ARG: a NULL context; NULL n_rows; n > 0xFFFFFFFF (the item index of a row is 32 bits; checked before the items are read); NULL
 * items with n > 0; NULL rows with cap_rows > 0; and what the single-answer call rejects in the items: a non-finite coordinate, an rmax
 * or tmax that is NaN or negative, an all-zero direction -- checked on the host before anything is launched, and nothing is written
 * then.  n = 0 returns CD_OK with *n_rows = 0.  The calls leave cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH
 * step and every other query's buffers as they were; they keep device buffers of their own (grown on demand, the candidate buffer
 * by running the pass again; cd_destroy frees them) and run on the context's stream. */
typedef struct cd_point_rows { uint32_t *ids; double *dist; double *closest; double *uv; uint8_t *feature; uint8_t *side; } cd_point_rows;
int cd_points_within(cd_ctx *ctx, const double *points, uint64_t n, uint32_t *rows, uint64_t cap_rows,
                     uint64_t *n_rows, uint64_t *n_tested, const cd_point_rows *out);
typedef struct cd_ray_rows { uint32_t *ids; double *t; double *uv; uint8_t *side; } cd_ray_rows;
int cd_cast_rays_all(cd_ctx *ctx, const double *rays, uint64_t n, uint32_t *rows, uint64_t cap_rows,
                     uint64_t *n_rows, uint64_t *n_tested, const cd_ray_rows *out);

/* ---- nearest triangle and separation distance between two meshes (not reference behaviour) ----
 * The threshold-free between-mesh question: how far is mesh a from mesh b, and where are they closest?  The per-pair functions are
 * tri_distance (the proximity section) and tri_witness (the witness section), a's triangle as the first argument, as in every
 * between call.  rmax is a search radius, 0 <= rmax <= +inf.
 *
 * flags = 0, per triangle: na rows, na the number of a's triangles.  Row i belongs to face i of a's face list from cd_create.  Of the
 * triangles B of b with tri_distance(A_i, B) <= rmax (closed) the winner is the one with the smallest (dist, ID of B, face index of B)
 * in lexicographic order.  faces[2 i] = i, faces[2 i + 1] = the winner's index in b's face list; ids[2 i], ids[2 i + 1]: the two IDs;
 * dist[i]: tri_distance(A_i, B), bit for bit.  When nothing is within rmax both faces are 0xFFFFFFFF, dist[i] = +inf and every other
 * output of the row is 0.  With rmax = +inf every row finds a triangle.
 * flags = CD_NEAREST_MIN, the separation distance: exactly ONE row.  Over all pairs with dist <= rmax the pair with the smallest
 * (dist, ID in a, face in a, ID in b, face in b); the "nothing" row above when no pair is within rmax.  By definition it is the
 * lexicographic minimum over the rows of the flags = 0 call.
 * ids and dist may be NULL.  w (may be NULL, and so may each of its members): points, bary and feature of a row are
 * tri_witness(A, B) of that row's pair -- its dist is dist[row] bit for bit, by tri_witness's own contract; a pair in contact is at 0
 * with features 7 / 7 and zeros; w->faces receives the same values as faces; a "nothing" row gets features 0 / 0 and zeros.
 * info (may be NULL): rows that found a triangle, boxes tested, tri_distance evaluations -- numbers of this run and this tree, not of
 * the meshes; with CD_NEAREST_MIN the last two may differ from run to run (the lanes share a shrinking bound), the result may not.
 * Guarantee: the result depends on the two meshes and rmax only -- not on either Morton frame, CD_OPT_TRAVERSAL, CD_OPT_CELL_TABLE,
 * the build variant or the run -- over the band of coordinate magnitudes of cd_find_proximity.  Both contexts are left as they were:
 * cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH step and every other query's buffers.  The call keeps device
 * buffers of its own in a (grown on demand; cd_destroy frees them) and runs on a's stream with one host synchronisation.
 * CD_ERR_ARG: a NULL context; a == b; contexts on different HIP devices; rmax NaN or negative; flags other than 0 / CD_NEAREST_MIN;
 * NULL faces -- checked on the host before anything is launched, and nothing is written then.  CD_ERR_ORDER unless both contexts have
 * a tree of their current vertices.  There is no CD_OVERFLOW: the row count is fixed. */
typedef struct cd_nearest_info { uint64_t n_found, node_visits, tri_tests; } cd_nearest_info;
enum { CD_NEAREST_MIN = 1 };
int cd_nearest_between(cd_ctx *a, cd_ctx *b, double rmax, int flags, uint32_t *faces, uint32_t *ids, double *dist,
                       const cd_witness_out *w, cd_nearest_info *info);

/* ---- nearest non-neighbouring triangle of the same mesh, and the mesh's clearance (not reference behaviour) ----
 * The threshold-free self question: how near does this mesh come to itself, and where?  A CCD dist or a step size for a garment whose
 * clearance is not known yet, a per-triangle self-clearance map, a "nothing of this mesh is near itself" test.  rmax is a search
 * radius, 0 <= rmax <= +inf.
 *
 * Admissible pairs: the unordered pairs (i, f) of distinct faces with no shared vertex index (cd_find_proximity's neighbour rule; equal
 * IDs do not exclude a pair).  The distance of a pair is tri_distance(A, B) with A the face with the smaller (ID, face index),
 * cd_find_proximity's rule: both rows that hold a pair hold the same bits, and they are cd_find_proximity's dists for that pair.
 *
 * flags = 0, per triangle: nt rows; row i belongs to face i of cd_create's face list.  Of the faces f admissible with i and with
 * distance <= rmax (closed) the winner is the one with the smallest (dist, ID of f, f).  faces[2 i] = i, faces[2 i + 1] = f;
 * ids[2 i], ids[2 i + 1]: the IDs of i and f; dist[i]: that distance.  When nothing is within rmax both faces are 0xFFFFFFFF,
 * dist[i] = +inf and every other output of the row is 0 (cd_nearest_between's "nothing" row).
 * flags = CD_NEAREST_MIN, the clearance of the mesh: exactly ONE row, the lexicographic minimum of the flags = 0 rows by
 * (dist, own ID, own face, partner ID, partner face), or the "nothing" row.
 * ids and dist may be NULL.  w (may be NULL, and so may each of its members): points, bary and feature of a row are
 * tri_witness(A, B) of the row's pair in the order that was PLAYED; w->faces[2 row], w->faces[2 row + 1] are the faces that played
 * A and B -- not (own, partner): cd_find_proximity_witness's convention.  The witness's dist is dist[row] bit for bit; a pair in
 * contact has features 7 / 7 and zeros; a "nothing" row has w->faces 0xFFFFFFFF, features 0 / 0 and zeros.
 * info (may be NULL): rows that found a partner, boxes tested, tri_distance evaluations (an excluded triangle is not one) -- numbers
 * of this run and this tree; with CD_NEAREST_MIN the last two may differ from run to run, the result may not.
 * Guarantee: the result depends on the mesh and rmax only -- not on the Morton frame, CD_OPT_TRAVERSAL, CD_OPT_CELL_TABLE, the build
 * variant or the run -- over the band of coordinate magnitudes of cd_find_proximity.  The context is left as it was: cd_stats, the
 * last pair list, the order hint, a captured CD_OPT_GRAPH step and every other query's buffers.  The call keeps device buffers of its
 * own (grown on demand; cd_destroy frees them) and runs on the context's stream with one host synchronisation.
 * CD_ERR_ARG: a NULL context; rmax NaN or negative; flags other than 0 / CD_NEAREST_MIN; NULL faces -- checked on the host before
 * anything is launched, and nothing is written then.  CD_ERR_ORDER unless the context has a tree of its current vertices.  There is
 * no CD_OVERFLOW: the row count is fixed. */
int cd_nearest_self(cd_ctx *ctx, double rmax, int flags, uint32_t *faces, uint32_t *ids, double *dist,
                    const cd_witness_out *w, cd_nearest_info *info);

/* ---- swept-point queries: moving points against the moving mesh (not reference behaviour) ----
 * The moving question for a point: a particle, a strand node, a grain with a radius, a garment vertex against a body that deforms in
 * the same step, the vertex-face half of a cloth's own CCD pass.  items is n x 7 doubles: p0, p1 (the point moves linearly from p0 to
 * p1 during the step) and the item's own dist, finite and > 0; all six coordinates finite.  The mesh moves linearly from the context's
 * vertices x0 (the tree's) to verts_end = x1, in cd_find_ccd's layout; x1 is uploaded by the call and never installed; NULL: the mesh
 * does not move (x1 = x0).  skip_vertex (may be NULL): n vertex indices, 0xFFFFFFFF for none; the triangles with that index among
 * their three are not tested for item k (the neighbour filter of a mesh's own vertices swept against the mesh), before the gate.
 *
 * pt_advance, the per-pair function (FP64, fixed operation order, no contraction; tests/sweep_ref.py restates it): every coordinate
 * moves as a + t (b - a), the difference, the product and the sum each rounded.  L = max_i |(b_i - a_i) - (p1 - p0)| (1 + 2^-20) over
 * the triangle's three vertices, |v| = sqrt((x x + y y) + z z); h = dist / 2.  At t = 0, on p0 and x0 themselves, r = pt_tri (the
 * closest-point section).  r.dist <= dist: reported at this t.  Else, with the evaluation on x1 done or L == 0: not reported.  Else,
 * after 1024 evaluations: reported UNRESOLVED at this t, with r.dist > dist.  Else t' = t + (r.dist - h) / L; t' >= 1: one evaluation
 * on p1 and x1 themselves, reported at toi = 1 when within dist; otherwise t = t' and again.  A reported pair returns toi, r of the
 * reporting evaluation (dist, u, v, feature, side and q, the closest point on the triangle as it stands at toi) and the evaluation count.
 * The gate decides which pairs are evaluated at all: the box of {p0, p1} and the box of the triangle's six points, each widened by dist
 * (lo - dist, hi + dist), overlap (closed).
 * Guarantee: with M the largest |coordinate| of the point and the triangle over both ends and delta = 2^-38 M, a
 * point that comes closer than h - delta to the exactly moving triangle at some t* is reported with toi <= t*, and stays at least
 * h - delta away before toi.
 *
 * cd_sweep_points_all: one row for every (item k, face f) that passes the filter and the gate and that pt_advance reports.  Row r:
 * rows[2 r] = k, rows[2 r + 1] = f, the index in cd_create's face list; each (k, f) once, in free order.  out (may be NULL, and so may
 * each member), per row: the face's ID, toi, and dist, closest, uv, feature, side of the reporting evaluation.  CD_OVERFLOW with the
 * true *n_rows when it exceeds cap_rows; nothing is written at or past cap_rows; cap_rows = 0 (rows may be NULL) counts only.  info (may
 * be NULL): candidates of the walk (a number of this tree), pairs through the gate, pt_tri evaluations, unresolved rows.
 * cd_sweep_points: per item the row of cd_sweep_points_all with the smallest (toi, ID, face index), bit for bit, by definition;
 * without one face[k] = 0xFFFFFFFF, toi[k] = +inf and zeros elsewhere.  face is required, the others may be NULL.  flags must be 0.
 * info (may be NULL): items with a row, records visited, pt_tri evaluations -- numbers of this tree and this run's item order.
 * The rows and every value in them depend on the mesh, x1 and the items only -- not on the Morton frame, CD_OPT_TRAVERSAL,
 * CD_OPT_CELL_TABLE, the build variant or the order of the items.  Items are walked in the order given, one lane each.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise).  CD_ERR_ARG: a NULL context; NULL n_rows / face; n >
 * 0xFFFFFFFF; NULL items with n > 0; NULL rows with cap_rows > 0; a non-finite coordinate; a dist that is not finite and > 0; flags
 * other than 0 -- checked on the host before anything is launched, and nothing is written then.  n = 0 returns CD_OK.  The calls
 * leave cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH step, cd_debug_swept's view of the last CCD pass and
 * every other query's buffers as they were; they keep device buffers of their own, swept records included (cd_destroy frees them).
 *
 * cd_pt_advance_points: pt_advance on explicit operands, host pointers, no context and no gate: items n x 7, tri n x 18 (a0 a1 a2 at
 * x0, then b0 b1 b2 at x1).  toi = +inf: not reported; the other outputs (each may be NULL) are those of the last evaluation made. */
typedef struct cd_sweep_rows { uint32_t *ids; double *toi; double *dist; double *closest; double *uv; uint8_t *feature; uint8_t *side; } cd_sweep_rows;
int cd_sweep_points_all(cd_ctx *ctx, const double *verts_end, const double *items, uint64_t n, const uint32_t *skip_vertex,
                        uint32_t *rows, uint64_t cap_rows, uint64_t *n_rows, const cd_sweep_rows *out, cd_ccd_info *info);
int cd_sweep_points(cd_ctx *ctx, const double *verts_end, const double *items, uint64_t n, const uint32_t *skip_vertex, int flags,
                    uint32_t *face, uint32_t *ids, double *toi, double *dist, double *closest, double *uv, uint8_t *feature,
                    uint8_t *side, cd_point_info *info);
int cd_pt_advance_points(const double *items, const double *tri, uint64_t n, double *toi, double *dist, double *closest, double *uv,
                         uint8_t *feature, uint8_t *side, uint32_t *evals);

/* ---- inside / outside and signed distance for points (not reference behaviour) ----
 * Is a point inside the closed surface this context's mesh forms?  The contained object that produces no colliding pair, a garment
 * vertex that has passed through the body, the sign of a distance field.  A point is three finite doubles; axis (0, 1 or 2) picks the
 * COLUMN, the line through the point parallel to that axis, along which the surface's crossings are counted.
 * column_tri(p, c; triangle v0 v1 v2), FP64 with a fixed operation order and no contraction, every difference, product and sum
 * rounded on its own (csrc/cd_math.h); a = (c + 1) % 3, b = (c + 2) % 3:
 *   gate:  p_a within [min, max] of the three v_a and p_b within those of v_b, closed, exact comparisons; else the face does not cover;
 *   edge l -> h:  la = l_a - p_a, lb = l_b - p_b, ha = h_a - p_a, hb = h_b - p_b, E = la hb - lb ha;
 *          E0 = E(v1 -> v2), E1 = E(v2 -> v0), E2 = E(v0 -> v1);
 *   the sign of an edge: that of E where E != 0; else that of l_b - h_b; else that of h_a - l_a (the input coordinates, compared
 *          exactly); else 0 -- the sign E would have for p moved by (eps, eps^2) in (a, b);
 *   cover: o = +1 when the three signs are +, -1 when they are -, else 0;
 *   height: z_i = v_i,c - p_c, S = (E0 + E1) + E2, zc = (E0 z0 + E1 z1) + E2 z2; S == 0: not counted; above when (zc > 0 and S > 0) or
 *          (zc < 0 and S < 0), else below (zc == 0, the point on the face, is below).  A NaN anywhere: not counted.
 * Swapping an edge's ends negates E exactly and reverses both tie comparisons, so the two faces on an edge see opposite signs: a point
 * exactly under an edge or a vertex is covered by the faces its moved copy is under and by no other -- one owner per crossing.  Where
 * every computed E has its true sign or is a true zero the counts are exactly the moved point's.  The arithmetic is not exact: for a
 * point within rounding of an edge's projection a sign can be wrong and a count off by one.
 *
 * cd_points_inside, per point k over the faces of this context: n_above[k] / n_below[k]: the faces counted above / below p;
 * w_above[k] / w_below[k]: the sums of their o.  On a closed, consistently oriented mesh w_above + w_below == 0 and w_above is the
 * winding number of p: +1 inside a body whose faces are counter-clockwise seen from outside, -1 inside an inverted one, 0 outside
 * and between a shell and an inverted shell inside it.  inside[k] = w_above[k] != 0; with CD_INSIDE_PARITY inside[k] = n_above[k] odd,
 * which needs no consistent orientation.  w_above[k] + w_below[k] != 0 tells the caller that the column passed through a hole or an
 * open mesh: the answer for k then means nothing, and another axis may avoid the hole.  inside is required; the four count arrays
 * may each be NULL.  info (may be NULL): points inside, boxes tested, column_tri evaluations -- numbers of this tree, not of the mesh.
 *
 * cd_signed_distance: cd_closest_points with rmax = +inf and cd_points_inside on the same points in one call, one host
 * synchronisation.  sdist[k] = -dist when inside[k], else dist; a dist of 0 stays +0.  face, ids, closest, uv, feature: bit for bit
 * cd_closest_points' values for k (|sdist[k]| its dist); inside: cd_points_inside's for this axis and these flags.  sdist is
 * required, the rest may be NULL.  info (may be NULL): points that found a triangle, and the boxes tested and exact evaluations of
 * both kernels together.
 *
 * Limits.  An open mesh (a cloth) has no inside.  A point ON the surface gets whichever side the arithmetic gives.  One lane walks
 * its point's whole column through the mesh, and neighbours in the array share a wave: points that are neighbours in space should be
 * neighbours in the array; the library does not sort them.
 * Guarantee: the result depends on the mesh, the points, the axis and the flags only -- not on the Morton frame, CD_OPT_TRAVERSAL,
 * CD_OPT_CELL_TABLE, the build variant or the order of the points.  Scaling mesh and points by 2^k changes no count while no nonzero
 * product leaves the normal FP64 range.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise, including after cd_update_vertices without a rebuild).
 * CD_ERR_ARG: a NULL context; NULL points, inside (cd_points_inside) or sdist (cd_signed_distance) with n > 0; an axis outside 0..2;
 * flags other than 0 / CD_INSIDE_PARITY; a non-finite coordinate -- checked on the host before anything is launched, and nothing is
 * written then.  n = 0 returns CD_OK.  The calls leave cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH step and
 * every other query's buffers as they were; they keep device buffers of their own (grown on demand; cd_destroy frees them) and run on
 * the context's stream with one host synchronisation. */
enum { CD_INSIDE_PARITY = 1 };
typedef struct cd_inside_info { uint64_t n_inside, node_visits, tri_tests; } cd_inside_info;
int cd_points_inside(cd_ctx *ctx, const double *points /* n x 3 */, uint64_t n, int axis, int flags, uint8_t *inside,
                     uint32_t *n_above, uint32_t *n_below, int32_t *w_above, int32_t *w_below, cd_inside_info *info);
int cd_signed_distance(cd_ctx *ctx, const double *points /* n x 3 */, uint64_t n, int axis, int flags, double *sdist, uint32_t *face,
                       uint32_t *ids, double *closest, double *uv, uint8_t *feature, uint8_t *inside, cd_point_info *info);
/* column_tri on explicit operands (host pointers; no context): points is n x 3 doubles, tri n x 9 (v0, v1, v2), axis 0..2.  cover[k]:
 * o (0 / +1 / -1, the gate included); above[k]: 1 when the face is counted above; E[3 k ..]: E0, E1, E2; zc[k], S[k].  A face with
 * cover != 0 and above == 0 is counted below unless S == 0 or zc is NaN.  E, zc and S are computed whatever the gate says.  Every
 * output except cover may be NULL.  No argument is checked for finiteness: the arithmetic decides.  The pin of the device function. */
int cd_column_tri_points(const double *points, const double *tri, uint64_t n, int axis, int8_t *cover, uint8_t *above, double *E,
                         double *zc, double *S);

/* ---- box queries: every triangle that meets an axis-aligned box (not reference behaviour) ----
 * Which triangles lie in this region?  One box a voxel of an occupancy grid, a brush or a trigger volume, the part of a garment in a
 * region, triangles per cell, the surface voxels of a distance field's narrow band.  A box is six doubles {x1, x2, y1, y2, z1, z2},
 * the layout of cd_root_box, and it is CLOSED: touching counts, and lo == hi on any axis is allowed (a slab, a line, a point).  This
 * is deliberately not the strict overlap of box.cuh: a triangle lying in a voxel's face belongs to both voxels.
 * box_tri(box; triangle p0 p1 p2) -> (hit, inside, code), FP64 with a fixed operation order and no contraction, every difference,
 * product and sum rounded on its own (csrc/cd_math.h):
 *   1 gate:   per axis a = x, y, z in that order, exact comparisons of the inputs: max(p0_a, p1_a, p2_a) < lo_a or min(...) > hi_a:
 *             miss, code 1 + a;
 *   2 inside: all three vertices in the closed box on all axes (exact comparisons): hit, inside = 1, code 0; nothing further is
 *             evaluated;
 *   2b vertex: any vertex in the closed box (exact comparisons): hit, inside = 0, code 0; nothing further is evaluated -- a box that
 *             touches a vertex, a point box on it included, cannot lose the face to the rounding of steps 3 and 4;
 *   3 edges:  c_a = 0.5 lo_a + 0.5 hi_a, h_a = 0.5 hi_a - 0.5 lo_a, v_i = p_i - c, f0 = p1 - p0, f1 = p2 - p1, f2 = p0 - p2; for edge
 *             k = 0, 1, 2 and box axis j = 0, 1, 2 in lexicographic (k, j) order, a = (j + 1) % 3, b = (j + 2) % 3:
 *             q_i = v_i[b] f_k[a] - v_i[a] f_k[b], r = h[a] |f_k[b]| + h[b] |f_k[a]|; min(q0, q1, q2) > r or max(q0, q1, q2) < -r:
 *             miss, code 4 + 3 k + j;
 *   4 plane:  n = f0 x f1 (each component x y - z w), d = (n_x v0_x + n_y v0_y) + n_z v0_z, r = (h_x |n_x| + h_y |n_y|) + h_z |n_z|;
 *             d > r or d < -r: miss, code 13; otherwise hit, inside = 0, code 0.
 * A miss reports the first separating test in this order.  A NaN separates nothing.  A degenerate triangle (a segment, a point) needs
 * no special case.  Scaling box and triangle by 2^k changes nothing while no nonzero product of three coordinate differences leaves
 * the normal FP64 range (ray_tri's band: |k| <= 300 for coordinates of order 1 .. 16); outside it the result follows the arithmetic.
 *
 * cd_boxes_overlap_all: one row for every (box k, face f) of this context that box_tri hits.  rows[2 r] = k, rows[2 r + 1] = f, the
 * index in cd_create's face list; out->ids[r]: the face's ID; out->inside[r]: box_tri's inside.  out and each array in it may be
 * NULL.  Everything else is cd_points_within's contract: the order of the rows is free and each (k, f) appears once; *n_rows is the
 * true number of rows, CD_OVERFLOW when it exceeds cap_rows, and nothing is written at or past cap_rows in any array; cap_rows = 0
 * counts only; n_tested (may be NULL): box_tri evaluations, a number of this tree.
 *
 * cd_boxes_count, by definition: count[k] is the number of rows item k has in cd_boxes_overlap_all, n_inside[k] (may be NULL) the
 * number of those with inside = 1.  With CD_BOX_ANY count[k] is 0 or 1, equal to (count > 0), the walk of a box stops at its first
 * hit, and n_inside must be NULL.  info (may be NULL): boxes with count > 0, boxes tested, box_tri evaluations -- numbers of this
 * tree.  One kernel with integer sums in registers: no candidate buffer, nothing that can overflow.  A subtree whose stored box lies
 * inside the query box is counted without being walked (every triangle in it takes rule 2), the whole tree included: a box around
 * the mesh costs one test.
 *
 * Limits.  The rows call walks a box that meets the whole mesh in one lane.  Neighbours in the array share a wave: boxes that are
 * neighbours in space should be neighbours in the array; the library does not sort them.  Oriented boxes and forms between two
 * meshes are not built.
 * Guarantee: the result depends on the mesh and the boxes only -- not on the Morton frame, CD_OPT_TRAVERSAL, CD_OPT_CELL_TABLE, the
 * build variant or the order of the boxes.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise, including after cd_update_vertices without a rebuild).
 * CD_ERR_ARG: a NULL context; NULL boxes with n > 0; n > 2^32 - 1; NULL n_rows, or NULL rows with cap_rows > 0 (cd_boxes_overlap_all);
 * NULL count with n > 0, flags other than 0 / CD_BOX_ANY, n_inside given with CD_BOX_ANY (cd_boxes_count); a bound that is not finite
 * or lo > hi on an axis -- checked on the host before anything is launched, and nothing is written then.  n = 0 returns CD_OK.  The
 * calls leave cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH step and every other query's buffers as they
 * were; they keep device buffers of their own (grown on demand; cd_destroy frees them) and run on the context's stream. */
enum { CD_BOX_ANY = 1 };
typedef struct cd_box_rows { uint32_t *ids; uint8_t *inside; } cd_box_rows;
typedef struct cd_box_info { uint64_t n_found, node_visits, tri_tests; } cd_box_info;
int cd_boxes_overlap_all(cd_ctx *ctx, const double *boxes /* n x 6 */, uint64_t n, uint32_t *rows, uint64_t cap_rows,
                         uint64_t *n_rows, uint64_t *n_tested, const cd_box_rows *out);
int cd_boxes_count(cd_ctx *ctx, const double *boxes /* n x 6 */, uint64_t n, int flags, uint32_t *count, uint32_t *n_inside,
                   cd_box_info *info);
/* box_tri on explicit operands (host pointers; no context): boxes is n x 6 doubles, tri n x 9 (p0, p1, p2).  hit[k], inside[k]: 0 / 1;
 * code[k]: 0 for a hit, else the first separating test (1 .. 13).  hit is required, the others may be NULL.  CD_ERR_ARG: NULL boxes,
 * tri or hit with n > 0; n = 0 returns CD_OK and writes nothing.  No argument is checked for finiteness: the arithmetic decides.  The
 * pin of the device function. */
int cd_box_tri_points(const double *boxes, const double *tri, uint64_t n, uint8_t *hit, uint8_t *inside, uint8_t *code);

/* ---- plane queries: where a plane cuts the mesh, and what lies on each side (not reference behaviour) ----
 * A floor or a wall (is anything under it, and how much), a clip plane, the cross-section of a garment for a debug view, the layers
 * of a slicer, splitting a mesh in two.  A plane is four doubles {nx, ny, nz, d}: the points with n . x = d.  n need not be a unit
 * vector; "below" is the side n points away from.
 * plane_tri(plane; triangle p0 p1 p2) -> (class, a, b, edge_a, edge_b, t_a, t_b, on), FP64 with a fixed operation order and no
 * contraction, every product, sum, difference and quotient rounded on its own (csrc/cd_math.h):
 *   vertex: s_i = ((nx p_i.x + ny p_i.y) + nz p_i.z) - d.  Vertex i is BELOW iff s_i < 0; s_i > 0, +-0 and a NaN are "not below".
 *   class:  CD_PLANE_BELOW: all three vertices below.  CD_PLANE_ABOVE: none below -- a face lying in the plane, or touching it from
 *           above, is ABOVE.  CD_PLANE_CUT: otherwise.
 *   points: a CUT face has exactly two boundary edges, of e = 0 (p0 -> p1), 1 (p1 -> p2), 2 (p2 -> p0), whose ends differ in "below".
 *           For such an edge L is its below vertex and U the other, whichever way the face runs through it.  s_U == 0: the point is
 *           U itself, t = 1.  Otherwise t = s_L / (s_L - s_U) and the point is L + t (U - L) per component (difference, product, sum).
 *           a is the point on the edge through which the boundary leaves "not below", b the point on the edge it comes back through.
 *   on:     bit i set iff s_i == 0.
 * A face that is not CUT has a = b = 0, edges 0, t = 0.  Consequences (proved in DESIGN.md section 24):
 *   - the point of a shared edge is the same bits in both faces: it depends on the edge's two vertices and the plane alone;
 *   - on a closed, consistently oriented mesh the multiset of a equals the multiset of b: the segments a -> b are closed loops with
 *     no epsilon anywhere, counter-clockwise seen from the tip of n for an outward mesh, and sum n . (a x b) / (2 |n|) is the
 *     enclosed area;
 *   - an edge lying in the plane is reported once, by the face below it;
 *   - a face below that touches the plane with one vertex is a row with a == b;
 *   - n_above + n_below + n_cut == the number of faces, always.
 * Scaling mesh and d by 2^k changes nothing but the scale of a and b while no nonzero intermediate (products n_a x_a and their sums)
 * leaves the normal FP64 range: ray_tri's band, |k| <= 300 for coordinates and |n| of order 1 .. 16.
 *
 * cd_planes_cut_all: one row for every (plane k, face f) of this context whose class is CD_PLANE_CUT.  rows[2 r] = k,
 * rows[2 r + 1] = f, the index in cd_create's face list; out->ids[r]: the face's ID; out->seg[6 r ..]: a then b; out->edge[2 r ..]:
 * edge_a, edge_b; out->t[2 r ..]: t_a, t_b; out->on[r].  out and each array in it may be NULL.  Everything else is
 * cd_boxes_overlap_all's contract: the order of the rows is free and each (k, f) appears once; *n_rows is the true number of rows,
 * CD_OVERFLOW when it exceeds cap_rows, and nothing is written at or past cap_rows in any array; cap_rows = 0 counts only; n_tested
 * (may be NULL): plane_tri evaluations, a number of this tree.
 *
 * cd_planes_count, by definition: n_cut[k] is the number of rows plane k has in cd_planes_cut_all; n_below[k] and n_above[k] (each
 * may be NULL) the faces of class BELOW and ABOVE.  info (may be NULL): planes with n_cut > 0, boxes tested, plane_tri evaluations
 * -- numbers of this tree.  One kernel with integer sums: no candidate buffer, nothing that can overflow.  A subtree whose stored
 * box lies on one side of the plane is counted without being walked, the whole tree included.
 *
 * One plane, many lanes.  A plane's work is cut into slabs of CD_PLANE_SLAB consecutive leaves of the tree, a lane each, so ONE plane
 * through a large mesh fills the device; no item of these calls is walked by a single lane.  The box filter of the walk is exact and
 * needs no pad: a subtree is skipped only when the rounded vertex formula at two corners of its box proves every vertex on one side.
 * Guarantee: the result depends on the mesh and the planes only -- not on the Morton frame, CD_OPT_TRAVERSAL, CD_OPT_CELL_TABLE, the
 * build variant, CD_PLANE_SLAB or the order of the planes.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise, including after cd_update_vertices without a rebuild).
 * CD_ERR_ARG: a NULL context; NULL planes with n > 0; n > 2^32 - 1, or n times the slabs of this tree above 2^36; NULL n_rows, or NULL
 * rows with cap_rows > 0 (cd_planes_cut_all); NULL n_cut with n > 0 (cd_planes_count); a plane with a member that is not finite or
 * with n = (0, 0, 0) -- checked on the host before anything is launched, and nothing is written then.  n = 0 returns CD_OK.  The calls
 * leave cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH step and every other query's buffers as they were;
 * they keep device buffers of their own (grown on demand; cd_destroy frees them) and run on the context's stream.
 * Not built: rows for the faces wholly below (a half-space selection is a count here or a box query), oriented boxes, frustums,
 * forms between two meshes. */
#ifndef CD_PLANE_SLAB
#define CD_PLANE_SLAB 256           /* leaves a lane; a power of two (tools/planes_time.py: DESIGN.md section 24) */
#endif
enum { CD_PLANE_ABOVE = 0, CD_PLANE_BELOW = 1, CD_PLANE_CUT = 2 };
typedef struct cd_plane_rows { uint32_t *ids; double *seg; uint8_t *edge; double *t; uint8_t *on; } cd_plane_rows;
typedef struct cd_plane_info { uint64_t n_found, node_visits, tri_tests; } cd_plane_info;
int cd_planes_cut_all(cd_ctx *ctx, const double *planes /* n x 4 */, uint64_t n, uint32_t *rows, uint64_t cap_rows,
                      uint64_t *n_rows, uint64_t *n_tested, const cd_plane_rows *out);
int cd_planes_count(cd_ctx *ctx, const double *planes /* n x 4 */, uint64_t n, uint32_t *n_cut, uint32_t *n_below,
                    uint32_t *n_above, cd_plane_info *info);
/* plane_tri on explicit operands (host pointers; no context): planes is n x 4 doubles, tri n x 9 (p0, p1, p2).  cls[k]: CD_PLANE_*;
 * seg[6 k ..]: a, b; edge[2 k ..]; t[2 k ..]; on[k].  cls is required, the others may be NULL.  CD_ERR_ARG: NULL planes, tri or cls
 * with n > 0; n = 0 returns CD_OK and writes nothing.  No argument is checked for finiteness: the arithmetic decides.  The pin of
 * the device function. */
int cd_plane_tri_points(const double *planes, const double *tri, uint64_t n, uint8_t *cls, double *seg, uint8_t *edge,
                        double *t, uint8_t *on);

/* ---- segment queries: every triangle within a radius of a segment, and the nearest (not reference behaviour) ----
 * The segment with a thickness -- the capsule: a strand or rod element against a body, the edges of one garment against another (the
 * edge-edge half of a repulsion pass, beside cd_points_within's vertex-face half), a bone or tool capsule against a mesh, a thick pick
 * ray of finite length.  segs is n x 7 doubles (ax, ay, az, bx, by, bz, r): the segment a + s (b - a), s in [0, 1], and a radius;
 * coordinates finite, 0 <= r <= +inf; a == b is allowed (a point).
 *
 * The per-pair predicate seg_tri(a, b; p0, p1, p2) -> (dist, s, u, v, feature, end, cross, side, qs, qt), FP64 with a fixed operation
 * order, no contraction, IEEE divide and sqrt:  s: the parameter of the closest point on the segment;  (u, v), feature: the closest
 * point on the triangle in pt_tri's coding (0 face, 1 / 2 / 3 edge 01 / 12 / 20, 4 / 5 / 6 vertex 0 / 1 / 2);  end: 1 when s == 0, 2 when
 * s == 1, else 0;  qs, qt: the two closest points.
 *   d = b - a per coordinate (one rounding).
 *   1. Crossing.  h = ray_tri(a, d, 1.0, p0, p1, p2), the call the contour makes for an edge.  On a hit: cross = 1, dist = 0, s = h.t,
 *      (u, v) = (h.u, h.v), feature = 0, side = h.side, qs = a + s d per coordinate (the product rounded, then the sum: the P of ray_tri's
 *      gate), qt = (w p0 + u p1) + v p2 with w = (1 - u) - v.  An all-zero d has det == 0 and misses by ray_tri's own arithmetic.
 *   2. Otherwise cross = 0, in pt_tri's frame translated to a: B = b - a, T_i = p_i - a; m = the largest |component| of B, T0, T1, T2;
 *      m == 0: pt_tri's all-coincident result (dist 0, s = u = v = 0, feature 4, end 1, side 0, qs = a, qt = p0); else m = f 2^ex with f
 *      in [0.5, 1), |ex| clamped at 1000, B and T_i times 2^-ex (exact), A = O the origin, and the minimum of 14 squared distances taken in
 *      this order, a later term replacing the running minimum only when STRICTLY smaller (an earlier term keeps a tie) -- the blocks are
 *      pt_tri's face and edge terms (above) and cd_find_proximity's edge-edge term:
 *        k = 0          face term of A against T                   s = 0               (u, v) = (fv, fw), feature 0
 *        k = 1, 2, 3    A against T's edges 01, 12, 20             s = 0               the edge's (u, v, feature) at its t, as pt_tri's table
 *        k = 4          face term of B against T                   s = 1
 *        k = 5, 6, 7    B against T's edges                        s = 1
 *        k = 8, 9, 10   T_(k-8) against the segment (A, B)         s = the clamped t   vertex k - 8: (u, v) = (0, 0), (1, 0), (0, 1)
 *        k = 11, 12, 13 the segment (A, B) against edge k - 11 at their interior critical point (+inf unless den > 0 and both parameters
 *                       lie in [0, 1])                             s = its s           the edge's (u, v, feature) at its t
 *      When d is all-zero ONLY terms 0..3 are taken: pt_tri(a)'s four terms in pt_tri's order and frame, so a segment with a == b is
 *      pt_tri(a) bit for bit -- dist, (u, v), feature, side, qt -- by construction.
 *      dist = sqrt(best) 2^ex;  side = 1 when (O - T0) . ((T1 - T0) x (T2 - T0)) > 0 on the scaled operands: pt_tri's side of endpoint a;
 *      qs = a for s == 0, b for s == 1, else a + s d;  qt = (w p0 + u p1) + v p2 on the ORIGINAL vertices.
 * The 14 terms are complete: without a crossing a closest pair involves a segment end (terms 0..7) or the triangle's boundary
 * (8..13); a pair in the interiors of both the segment and the face has the segment parallel to the plane there and slides, at the same
 * distance, to a segment end or to the boundary.  Band: ray_tri's (largest |coordinate| about 2^-300 .. 2^300), because the crossing
 * term is ray_tri; scaling segment and triangle by 2^k inside it scales dist, qs, qt exactly and changes nothing else.  Finite input
 * gives no NaN.  A triangle of no area (det == 0) is never crossed and gets the distance of the segment or point it is.
 * | |qs - qt| - dist | <= 2^-50 M on cross = 0 rows, M the pair's largest |coordinate|; on cross = 1 rows |qs - qt| <= 2^-46 M unless
 * the segment lies within rounding of the face's plane or the face is a sliver: there ray_tri's det is rounding noise, its gate admits
 * the hit, and the two points -- ray_tri's P and the point of its (u, v) -- can be as far apart as the triangle is large (conditions
 * on the inputs, as the witness's and the contour's bounds; measured: DESIGN.md section 25).
 *
 * cd_segments_within: one row for every (segment k, face f) of this context with seg_tri(a_k, b_k; f).dist <= r_k (closed).
 * rows[2 r] = k, rows[2 r + 1] = f, the index in cd_create's face list.  out (may be NULL, and so may each of its members), per row:
 * ids[r] the face's ID; dist[r], s[r], on_seg[3 r ..] (qs), on_tri[3 r ..] (qt), uv[2 r], uv[2 r + 1], feature[r], end[r], cross[r],
 * side[r]: seg_tri's values for (k, f).  Everything else is cd_points_within's contract, word for word: the order of the rows is free and
 * each (k, f) appears exactly once; *n_rows is the size of the set; when it exceeds cap_rows the call returns CD_OVERFLOW with the true
 * *n_rows, nothing is written at or past cap_rows in any array, and the rows that are written are distinct rows of the true set; rows
 * may be NULL with cap_rows 0: the count-only call; n_tested (may be NULL): seg_tri evaluations made -- a number of this tree.
 *
 * cd_segments_closest, flags = 0: for segment k, of the triangles with seg_tri's dist <= r_k (r is a search radius), the one with the
 * smallest (dist, triangle ID, face index).  face[k]: its index in the face list, 0xFFFFFFFF when nothing is within r; out (may be NULL,
 * and so may each member), per item: cd_segment_rows' values for it; when nothing is within r dist[k] = +inf and the other outputs are
 * 0.  By definition the smallest row of item k in cd_segments_within is this call's answer bit for bit, and the items with no row are
 * its 0xFFFFFFFF items.  flags = CD_SEGMENT_ANY: face[k] = 0xFFFFFFFF when nothing is within r and SOME triangle within r otherwise;
 * whether there is one is defined, which one is not; out must be NULL.  info (may be NULL): segments that found a triangle, boxes
 * tested, seg_tri evaluations -- numbers of this tree.
 *
 * Guarantee: the rows, the answers and every value in them depend on the mesh and the items only -- not on the Morton frame,
 * CD_OPT_TRAVERSAL, CD_OPT_CELL_TABLE, the build variant or the order of the items.  The box filter of both calls is the ray queries'
 * slab test over s in [0, 1] against the box inflated by the bound plus the point queries' pad; it only filters (the proof: DESIGN.md
 * section 25).  Items are walked in the order given, one lane each, neighbours in one wave: coherent items should be neighbours.  An
 * item of cd_segments_within whose bound meets every box (r = +inf) walks the whole tree in one lane: correct, bounded, and slow.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise, including after cd_update_vertices without a rebuild).
 * CD_ERR_ARG: a NULL context; n > 0xFFFFFFFF (checked before the items are read); NULL segs with n > 0; NULL n_rows, or NULL rows with
 * cap_rows > 0 (cd_segments_within); NULL face with n > 0, flags other than 0 / CD_SEGMENT_ANY, out given with CD_SEGMENT_ANY
 * (cd_segments_closest); a non-finite coordinate, an r that is NaN or negative -- checked on the host before anything is launched, and
 * nothing is written then.  n = 0 returns CD_OK.  The calls leave cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH
 * step and every other query's buffers as they were; they keep device buffers of their own (grown on demand, the candidate buffer by
 * running the pass again; cd_destroy frees them) and run on the context's stream.
 * Not built: capsules against capsules, forms between two meshes.  The moving question is cd_sweep_segments_all's (below). */
enum { CD_SEGMENT_ANY = 1 };
typedef struct cd_segment_rows { uint32_t *ids; double *dist; double *s; double *on_seg; double *on_tri; double *uv; uint8_t *feature; uint8_t *end; uint8_t *cross; uint8_t *side; } cd_segment_rows;
typedef struct cd_segment_info { uint64_t n_found, node_visits, tri_tests; } cd_segment_info;
int cd_segments_within(cd_ctx *ctx, const double *segs /* n x 7 */, uint64_t n, uint32_t *rows, uint64_t cap_rows,
                       uint64_t *n_rows, uint64_t *n_tested, const cd_segment_rows *out);
int cd_segments_closest(cd_ctx *ctx, const double *segs /* n x 7 */, uint64_t n, int flags, uint32_t *face,
                        const cd_segment_rows *out, cd_segment_info *info);
/* seg_tri on explicit operands (host pointers; no context): segs is n x 6 doubles (a, b; no radius), tri n x 9 (p0, p1, p2).  dist[k],
 * s[k], on_seg[3 k ..], on_tri[3 k ..], uv[2 k ..], feature[k], end[k], cross[k], side[k]: seg_tri's values; every output except dist
 * may be NULL.  CD_ERR_ARG: NULL segs, tri or dist with n > 0; n = 0 returns CD_OK and writes nothing.  No argument is checked for
 * finiteness: the arithmetic decides.  The pin of the device function. */
int cd_seg_tri_points(const double *segs, const double *tri, uint64_t n, double *dist, double *s, double *on_seg, double *on_tri,
                      double *uv, uint8_t *feature, uint8_t *end, uint8_t *cross, uint8_t *side);

/* ---- swept-segment queries: moving segments against the moving mesh (not reference behaviour) ----
 * The moving question for a segment: a strand or rod element, a bone or tool capsule, the edges of a garment against a body that
 * deforms in the same step, the edge-edge half of a cloth's own CCD pass.  items is n x 13 doubles: a0, b0, a1, b1 (end a of the
 * segment moves linearly from a0 to a1 during the step, end b from b0 to b1) and the item's own dist, finite and > 0; all twelve
 * coordinates finite.  A segment of zero length at both ends of the step (a0 == b0, a1 == b1) is a moving point.  The mesh moves
 * linearly from the context's vertices x0 (the tree's) to verts_end = x1, as for cd_sweep_points_all; NULL: the mesh does not move.
 * skip_vertices (may be NULL): n x 2 vertex indices, 0xFFFFFFFF for none; the triangles with either index among their three are not
 * tested for item k, before the gate -- what an edge of the mesh itself passes (its two ends).
 *
 * seg_advance, the per-pair function (FP64, fixed operation order, no contraction; tests/swept_segment_ref.py restates it), is
 * pt_advance (above) with seg_tri in place of pt_tri: every coordinate of the five points moves as x + t (y - x), the difference,
 * the product and the sum each rounded; the evaluation at t = 0 is on the start positions themselves and the one at t = 1 on the end
 * positions themselves.  L = max over the ends j in {a, b} and the vertices i of |(x1_i - x0_i) - (j1 - j0)| (1 + 2^-20), six norms,
 * |v| = sqrt((x x + y y) + z z); h = dist / 2.  r = seg_tri at t.  r.dist <= dist: reported at this t (a crossing, cross = 1 and
 * dist = 0, like any other evaluation).  Else, with the evaluation on the end positions done or L == 0: not reported.  Else, after
 * 1024 evaluations: reported UNRESOLVED at this t, with r.dist > dist.  Else t' = t + (r.dist - h) / L; t' >= 1: one evaluation on the
 * end positions, reported at toi = 1 when within dist; otherwise t = t' and again.  A reported pair returns toi, the whole of seg_tri's
 * result of the reporting evaluation (dist, s, qs, qt, u, v, feature, end, cross, side; qs and qt on the segment and the triangle as
 * they stand at toi) and the evaluation count.
 * The gate decides which pairs are evaluated at all: the box of {a0, b0, a1, b1} and the box of the triangle's six points, each widened
 * by dist (lo - dist, hi + dist), overlap (closed).
 * By construction an item with a0 == b0 and a1 == b1 is pt_advance of (a0, a1, dist) bit for bit and passes pt_gate's gate: its rows
 * are cd_sweep_points_all's.  With nothing moving there is one evaluation a pair and the rows are cd_segments_within's at r = dist.
 * Guarantee: with M the largest |coordinate| of the segment and the triangle over both ends and
 * delta = 2^-38 M, (1) a segment that comes closer than h - delta to the exactly moving triangle at some t* is reported with
 * toi <= t*, and stays at least h - delta away before toi; (2) a reported, resolved pair is within dist + delta at toi -- except a
 * cross = 1 report of a segment within rounding of the face's plane or through a sliver, where ray_tri's hit is noise: such a report
 * is early, never late.
 *
 * cd_sweep_segments_all: cd_sweep_points_all's contract word for word.  One row for every (item k, face f) that passes the filter and
 * the gate and that seg_advance reports.  Row r: rows[2 r] = k, rows[2 r + 1] = f, the index in cd_create's face list; each (k, f)
 * once, in free order.  out (may be NULL, and so may each member), per row: the face's ID, toi, and seg_tri's values of the reporting
 * evaluation: dist[r], s[r], on_seg[3 r ..] (qs), on_tri[3 r ..] (qt), uv[2 r ..], feature[r], end[r], cross[r], side[r].
 * CD_OVERFLOW with the true *n_rows when it exceeds cap_rows; nothing is written at or past cap_rows; cap_rows = 0 (rows may be NULL)
 * counts only.  info (may be NULL): candidates of the walk (a number of this tree), pairs through the gate, seg_tri evaluations,
 * unresolved rows.
 * cd_sweep_segments: per item the row of cd_sweep_segments_all with the smallest (toi, ID, face index), bit for bit, by definition;
 * without one face[k] = 0xFFFFFFFF, toi[k] = +inf and zeros elsewhere.  face is required; out and its members may be NULL.  flags
 * must be 0.  info (may be NULL): items with a row, records visited, seg_tri evaluations of the walk -- numbers of this tree and this
 * run's item order.
 * The rows and every value in them depend on the mesh, x1 and the items only -- not on the Morton frame, CD_OPT_TRAVERSAL,
 * CD_OPT_CELL_TABLE, the build variant or the order of the items.  Items are walked in the order given, one lane each.
 * Needs a tree built from the current vertices (CD_ERR_ORDER otherwise, including after cd_update_vertices without a rebuild).
 * CD_ERR_ARG: a NULL context; NULL n_rows / face; n > 0xFFFFFFFF; NULL items with n > 0; NULL rows with cap_rows > 0; a non-finite
 * coordinate; a dist that is not finite and > 0; flags other than 0 -- checked on the host before anything is launched, and nothing
 * is written then.  n = 0 returns CD_OK.  The calls leave cd_stats, the last pair list, the order hint, a captured CD_OPT_GRAPH step,
 * cd_debug_swept's view of the last CCD pass and every other query's results as they were; they refit the swept-point queries' swept
 * records for themselves (as those calls do on every call) and keep device buffers of their own (cd_destroy frees them).
 * Not built: a slab or capsule filter tighter than the four-point box, an ANY form, a form between two meshes.
 *
 * cd_seg_advance_points: seg_advance on explicit operands, host pointers, no context and no gate: items n x 13, tri n x 18 (the three
 * vertices at x0, then at x1).  toi = +inf: not reported; the other outputs (each may be NULL) are those of the last evaluation made.
 * The pin of the device function. */
typedef struct cd_sweep_segment_rows { uint32_t *ids; double *toi; double *dist; double *s; double *on_seg; double *on_tri; double *uv; uint8_t *feature; uint8_t *end; uint8_t *cross; uint8_t *side; } cd_sweep_segment_rows;
int cd_sweep_segments_all(cd_ctx *ctx, const double *verts_end, const double *items /* n x 13 */, uint64_t n,
                          const uint32_t *skip_vertices /* n x 2 */, uint32_t *rows, uint64_t cap_rows, uint64_t *n_rows,
                          const cd_sweep_segment_rows *out, cd_ccd_info *info);
int cd_sweep_segments(cd_ctx *ctx, const double *verts_end, const double *items /* n x 13 */, uint64_t n,
                      const uint32_t *skip_vertices /* n x 2 */, int flags, uint32_t *face, const cd_sweep_segment_rows *out,
                      cd_point_info *info);
int cd_seg_advance_points(const double *items /* n x 13 */, const double *tri /* n x 18 */, uint64_t n, double *toi, double *dist,
                          double *s, double *on_seg, double *on_tri, double *uv, uint8_t *feature, uint8_t *end, uint8_t *cross,
                          uint8_t *side, uint32_t *evals);

/* Library / build identification: "mi355cd <version> gfx950". */
const char *cd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355CD_H */
