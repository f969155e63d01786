// mi355cd.hip -- C-ABI implementation of include/mi355cd.h (libmi355cd.so), gfx950 only.
// Build: hipcc -O3 -ffp-contract=off --offload-arch=gfx950 -shared -fPIC (see ../Makefile).
#include "../../include/mi355cd.h"
#include "cd_math.h"
#include "cd_sort.h"
#include "cd_bvh.h"
#include "cd_build.h"
#include "cd_traverse.h"
#include "cd_post.h"
#include "cd_proximity.h"
#include "cd_ccd.h"
#include "cd_between.h"
#include "cd_witness.h"
#include "cd_contour.h"
#include "cd_rays.h"
#include "cd_points.h"
#include "cd_nearest.h"
#include "cd_within.h"
#include "cd_sweep.h"
#include "cd_inside.h"
#include "cd_boxes.h"
#include "cd_planes.h"
#include "cd_segments.h"
#include "cd_sweep_segments.h"
#include "cd_columns.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

using namespace cd;

namespace {

#define HIPCHK(expr)                                                   \
    do {                                                               \
        hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) return -(int)e_;                         \
    } while (0)

enum Stage { ST_CREATED = 0, ST_SORTED = 1, ST_BUILT = 2, ST_REFIT = 3 };

enum Ev { EV_MORTON0, EV_MORTON1, EV_SORT1, EV_HIER0, EV_HIER1, EV_REFIT0, EV_REFIT1, EV_TRAV0, EV_TRAV1, EV_DESC1, EV_DEEP0, EV_DEEP1, EV_CHK0, EV_CHK1, EV_BLK0, EV_BLK1, EV_COUNT };

}  // namespace

// Everything one traversal pass writes: counters, candidates, pairs (+ the Report in front of them), deferred items.
// The context has two sets: [0] for its own leaves as queries (and for every single-pass entry point), [1] for the
// external queries of the multi-GPU step, so that both passes can be enqueued back to back and read with ONE host
// synchronisation (cd_multi.h).
struct TravBuf {
    TravState *d_state = nullptr; bool state_owned = false;                // [0]: inside the context's scratch block (zeroed by the fused memset)
    uint32_t *d_pairs = nullptr; uint64_t pairs_cap = 0;                   // d_pairs points sizeof(Report) bytes into its allocation: [Report][pairs]
    char *h_report = nullptr;                                              // pinned: Report + SPEC_PAIRS pairs, target of the read-back
    uint32_t synced_reports = 0;                                           // reports into h_report that ended in a stream synchronise (polled completion waits for POLL_WARM of them)
    uint64_t direct_id = 0; uint32_t synced_direct = 0;                    // the same for the caller's pinned pair buffer last written directly (its serial number: pinned_pairs_id)
    uint2 *d_defer = nullptr; uint32_t defer_cap = 0;
    Candidates *d_cand = nullptr; uint64_t cand_cap = 0;
    int32_t *d_deep = nullptr; uint64_t deep_items = 0;
    // the report of the pass being enqueued, decided BEFORE its kernels are (run_traversal, prepare_report): the exact kernel posts the first pairs into pinned host memory itself
    uint32_t *post_dst = nullptr; uint64_t post_n = 0;                     // where to (the caller's pinned buffer, or the staging area behind the report), how many at most
    bool prepared = false; unsigned long long prep_seq = 0; uint32_t *prep_area = nullptr; bool posted = false;   // the polled completion's sequence number and the scan's area of that report; the pass's k_exact did post
};

// ---- the buffers of the queries behind the tree (proximity, CCD, between-mesh, rays, closest points) --------------------------------
// Every record allocates a group of buffers as a whole: the group's capacity (for the state words: the mirror's pointer) is set only
// after every allocation in it has succeeded, and a group that failed is freed again -- a later call finds it absent, never half there.
template <typename T> void dev_alloc(hipError_t &e, T *&p, size_t bytes)      // e carries the first error: nothing is tried after it
{
    if (e == hipSuccess && (e = hipMalloc(reinterpret_cast<void **>(&p), bytes)) != hipSuccess) p = nullptr;
}
template <typename T> void dev_free(T *&p) { hipFree(p); p = nullptr; }

// a query's device counters and their pinned mirror
template <typename State>
struct StateWords {
    State *d = nullptr, *h = nullptr;
    int ensure()
    {
        if (h) return CD_OK;
        hipError_t e = hipSuccess;
        State *mirror = nullptr;
        dev_alloc(e, d, sizeof(State));
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&mirror), sizeof(State), hipHostMallocDefault);
        if (e != hipSuccess) { dev_free(d); return -(int)e; }
        h = mirror;
        return CD_OK;
    }
    void release() { dev_free(d); if (h) hipHostFree(h); h = nullptr; }
};

// What the witness form of a pair query (cd_find_*_witness, cd_witness.h) adds to its PairBuf, allocated on the first such call: per
// reported pair the two leaf positions the exact stage notes, and the witness kernel's outputs
struct WitnessBuf {
    uint2 *d_leaf = nullptr; uint32_t *d_faces = nullptr; double *d_points = nullptr, *d_bary = nullptr; uint8_t *d_feat = nullptr; uint64_t cap = 0;
    void release() { dev_free(d_leaf); dev_free(d_faces); dev_free(d_points); dev_free(d_bary); dev_free(d_feat); cap = 0; }
    int ensure(uint64_t cap_pairs)
    {
        const uint64_t want = cap_pairs > 0 ? cap_pairs : 1;
        if (want <= cap) return CD_OK;
        release();
        hipError_t e = hipSuccess;
        dev_alloc(e, d_leaf, sizeof(uint2) * want);
        dev_alloc(e, d_faces, sizeof(uint32_t) * 2 * want);
        dev_alloc(e, d_points, sizeof(double) * 6 * want);
        dev_alloc(e, d_bary, sizeof(double) * 4 * want);
        dev_alloc(e, d_feat, sizeof(uint8_t) * 2 * want);
        if (e != hipSuccess) { release(); return -(int)e; }
        cap = want;
        return CD_OK;
    }
};

// What the contour form of a contact query (cd_find_collisions_contour, cd_find_collisions_between_contour, cd_contour.h) adds to its
// PairBuf, allocated on the first such call that asks for an output: the leaf positions of the reported pairs and the contour kernel's outputs
struct ContourBuf {
    uint2 *d_leaf = nullptr; uint32_t *d_faces = nullptr; uint8_t *d_code = nullptr; double *d_param = nullptr, *d_points = nullptr; uint64_t cap = 0;
    void release() { dev_free(d_leaf); dev_free(d_faces); dev_free(d_code); dev_free(d_param); dev_free(d_points); cap = 0; }
    int ensure(uint64_t cap_pairs)
    {
        const uint64_t want = cap_pairs > 0 ? cap_pairs : 1;
        if (want <= cap) return CD_OK;
        release();
        hipError_t e = hipSuccess;
        dev_alloc(e, d_leaf, sizeof(uint2) * want);
        dev_alloc(e, d_faces, sizeof(uint32_t) * 2 * want);
        dev_alloc(e, d_code, sizeof(uint8_t) * 3 * want);
        dev_alloc(e, d_param, sizeof(double) * 6 * want);
        dev_alloc(e, d_points, sizeof(double) * 6 * want);
        if (e != hipSuccess) { release(); return -(int)e; }
        cap = want;
        return CD_OK;
    }
};

// What a pair query (self-proximity, self-CCD, between two meshes, the self contour) owns: counters, NSHARD shards of candidates, the result arrays
template <typename State>
struct PairBuf {
    static constexpr bool HAS_TOI = std::is_same<State, CcdState>::value;   // (proximity reports no times; between-mesh always has the array)
    StateWords<State> state;
    uint2 *d_cand = nullptr; uint64_t shard_cap = 0;                        // candidates a shard
    uint32_t *d_pairs = nullptr; double *d_toi = nullptr, *d_dists = nullptr; uint64_t pairs_cap = 0;
    WitnessBuf wit;
    ContourBuf con;

    int alloc_cand(uint64_t per)
    {
        hipError_t e = hipSuccess;
        dev_alloc(e, d_cand, sizeof(uint2) * per * NSHARD);
        shard_cap = e == hipSuccess ? per : 0;
        return e == hipSuccess ? CD_OK : -(int)e;
    }
    void release_results() { dev_free(d_pairs); dev_free(d_toi); dev_free(d_dists); pairs_cap = 0; }
    void release() { state.release(); dev_free(d_cand); shard_cap = 0; release_results(); wit.release(); con.release(); }
    // nt: the triangles whose candidates the shards take (16 a triangle to start with; grown on overflow)
    int ensure(uint32_t nt, uint64_t cap_pairs)
    {
        int rc = state.ensure();
        if (!rc && !shard_cap) rc = alloc_cand(std::max<uint64_t>(4096, (16ull * nt + NSHARD - 1) / NSHARD));
        const uint64_t want = cap_pairs > 0 ? cap_pairs : 1;
        if (rc || want <= pairs_cap) return rc;
        release_results();
        hipError_t e = hipSuccess;
        dev_alloc(e, d_pairs, sizeof(uint32_t) * 2 * want);
        if (HAS_TOI) dev_alloc(e, d_toi, sizeof(double) * want);
        dev_alloc(e, d_dists, sizeof(double) * want);
        if (e != hipSuccess) { release_results(); return -(int)e; }
        pairs_cap = want;
        return CD_OK;
    }
    // after the synchronisation: true = a shard overflowed and the buffer has been grown (enqueue again); false = done, or rc says why not
    bool overflowed(int &rc)
    {
        uint64_t mx = 0;
        for (int i = 0; i < NSHARD; ++i) mx = std::max<uint64_t>(mx, state.h->shard[i * PROX_SHARD_STRIDE]);
        rc = CD_OK;
        if (mx <= shard_cap) return false;
        dev_free(d_cand);
        rc = alloc_cand(mx + mx / 4 + 1024);
        return rc == CD_OK;
    }
    int results(uint32_t *pairs, double *toi, double *dists, uint64_t cap_pairs, uint64_t *n_pairs) const
    {
        const uint64_t np = state.h->n_pairs, take = std::min(np, cap_pairs);
        if (take) {
            HIPCHK(hipMemcpy(pairs, d_pairs, sizeof(uint32_t) * 2 * take, hipMemcpyDeviceToHost));
            if (toi) HIPCHK(hipMemcpy(toi, d_toi, sizeof(double) * take, hipMemcpyDeviceToHost));
            if (dists) HIPCHK(hipMemcpy(dists, d_dists, sizeof(double) * take, hipMemcpyDeviceToHost));
        }
        if (n_pairs) *n_pairs = np;
        return np > cap_pairs ? CD_OVERFLOW : CD_OK;
    }
    void fill_info(cd_ccd_info *info) const                                 // (CcdState only)
    {
        if (!info) return;
        uint64_t cand = 0;
        for (int i = 0; i < NSHARD; ++i) cand += state.h->shard[i * PROX_SHARD_STRIDE];
        info->n_candidates = cand; info->n_tested = state.h->n_tested; info->n_evals = state.h->n_evals; info->n_unresolved = state.h->n_unresolved;
    }
};

// The swept tree of a CCD pass (cd_ccd.h) over `cap` leaves at most, and what cd_debug_swept reports of the last pass through it (host
// words only: nothing is enqueued for them)
struct SweptBuf {
    NodeRec32 *d_recs = nullptr; int32_t *d_up = nullptr; uint32_t *d_arrive = nullptr; uint64_t cap = 0;
    struct Seen { bool ran = false; uint32_t n = 0, m_bits = 0; double dist = 0.0; } seen;
    void release() { dev_free(d_recs); dev_free(d_up); dev_free(d_arrive); cap = 0; }
    int ensure(uint32_t n)
    {
        if (n <= cap) return CD_OK;
        release();
        hipError_t e = hipSuccess;
        dev_alloc(e, d_recs, sizeof(NodeRec32) * (size_t)n);
        dev_alloc(e, d_up, sizeof(int32_t) * 2 * (size_t)n);
        dev_alloc(e, d_arrive, sizeof(uint32_t) * (size_t)n);
        if (e != hipSuccess) { release(); return -(int)e; }
        cap = n;
        return CD_OK;
    }
};

// one device array of `cap` items, grown to the largest count seen (the old contents are not kept)
template <typename T>
struct DevArray {
    T *d = nullptr; uint64_t cap = 0;
    void release() { dev_free(d); cap = 0; }
    int ensure(uint64_t n, uint64_t elems_per_item)
    {
        if (n <= cap) return CD_OK;
        release();
        hipError_t e = hipSuccess;
        dev_alloc(e, d, sizeof(T) * elems_per_item * n);
        if (e != hipSuccess) return -(int)e;
        cap = n;
        return CD_OK;
    }
};

// What a per-item query (rays, closest points) owns: counters and ONE block of the items' inputs and results, whose columns are the
// query's list in cd_columns.h (Cols: it gives ensure() the bytes an item and cols() the pointers)
template <typename State>
struct ItemBuf {
    StateWords<State> state;
    DevArray<char> block;
    void release() { state.release(); block.release(); }
    template <class Cols, class... A> int ensure(uint64_t n, A... a) { const int rc = state.ensure(); return rc ? rc : block.ensure(n, column_bytes<Cols>(a...)); }
    template <class Cols, class... A> Cols cols(A... a) const { return carve<Cols>(block.d, block.cap, a...); }
    // what every call enqueues in front of its kernels (the items up, the counters zeroed) and behind them (the counters back)
    int upload(hipStream_t s, double *d_items, const double *items, uint64_t doubles, uint64_t n)
    {
        HIPCHK(hipMemcpyAsync(d_items, items, sizeof(double) * doubles * n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(state.d, 0, sizeof(State), s));
        return CD_OK;
    }
    int launched(hipStream_t s)
    {
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(state.h, state.d, sizeof(State), hipMemcpyDeviceToHost, s));
        return CD_OK;
    }
};

// What an all-results item query (cd_points_within, cd_cast_rays_all, cd_within.h) owns: a pair query's record -- counters, candidate
// shards, the rows (d_pairs: item, face) and their dist / t (d_dists) -- the items, and ONE block of the rows' other values, whose
// columns are the query's row list in cd_columns.h
struct ItemRowsBuf {
    PairBuf<ProxState> q;
    DevArray<double> items; DevArray<char> vals;
    void release() { q.release(); items.release(); vals.release(); }
    template <class Cols> int ensure(uint64_t n, uint64_t doubles_per_item, uint64_t cap_rows)
    {
        int rc = q.shard_cap ? CD_OK : q.alloc_cand(WITHIN_SHARD_FIRST);     // (before q.ensure, which would size the shards by a triangle count)
        if (!rc) rc = q.ensure(0, cap_rows);
        if (!rc) rc = items.ensure(n, doubles_per_item);
        return rc ? rc : vals.ensure(std::max<uint64_t>(cap_rows, 1), column_bytes<Cols>());
    }
    template <class Cols> Cols cols() const { return carve<Cols>(vals.d, vals.cap); }
};

// What the swept-point queries (cd_sweep_points_all, cd_sweep_points, cd_sweep.h) own: an all-results item query's record for the rows,
// the CCD counters their swept refit and exact stage write (M; evaluations, unresolved rows), swept records of their own (swept[0] and
// swept[1] stay the last CCD pass's), x1, the items' skip_vertex, and the first-contact call's counters and block
struct SweepBuf {
    ItemRowsBuf rows;
    StateWords<CcdState> cst;
    SweptBuf swept;
    DevArray<double> x1;
    DevArray<uint32_t> skip;
    ItemBuf<PointState> first;
    void release() { rows.release(); cst.release(); swept.release(); x1.release(); skip.release(); first.release(); }
};

// What the swept-segment queries (cd_sweep_segments_all, cd_sweep_segments, cd_sweep_segments.h) own besides what they share with the
// swept-point queries (SweepBuf's cst, swept and x1): the rows call's record, the items' skip_vertices (2 an item) and the
// first-contact call's counters and block
struct SweepSegBuf {
    ItemRowsBuf rows;
    DevArray<uint32_t> skip;
    ItemBuf<PointState> first;
    void release() { rows.release(); skip.release(); first.release(); }
};

struct cd_multi;
struct cd_ctx {
    uint32_t nv = 0, nt = 0;
    cd_multi *attached_multi = nullptr;     // the multi-GPU step object built on this context, if any (cd_multi.h): it holds a pointer to the context and buffers inside it
    int stage = ST_CREATED;
    int frame_mode = CD_FRAME_REFERENCE;
    uint32_t vbase = 0;
    int trav_variant = 3;                   // CD_OPT_TRAVERSAL: 0 = lane-private FP64 (A), 1 = fp32 descent from the root + exact kernel (B), 3 = half traversal (D)
    uint32_t queries_per_wave = 64; 
    uint32_t dbg_no_shared_path = 0;        // CD_DBG_NO_SHARED_PATH: k_descend without the shared root path (A/B)
    uint32_t dbg_diag = 0;                  // CD_DBG_DIAG: the DIAG instance of the descent kernel runs, which also fills the diagnostic counters (cd_debug_counters)
    uint32_t dbg_lds_pad = 0;               // CD_DBG_LDS_PAD: extra dynamic LDS bytes per traversal workgroup (occupancy experiments)
    double frame_host[FRAME_WORDS] = {0.004501, -0.476622, -0.381965, 3.08, 0.76, 2.36, 0.0, 0.0};   // morton.h:45,51,57; [6]: the bits of the key layout word (cd_math.h; 0 = the reference's interleave)
    hipStream_t stream = nullptr;
    hipEvent_t ev[EV_COUNT] = {};
    // inputs
    double *d_verts = nullptr; uint32_t *d_vidx = nullptr; uint32_t *d_ids = nullptr;
    // sort
    uint64_t *d_keys[2] = {nullptr, nullptr}; uint32_t *d_perm[2] = {nullptr, nullptr};
    uint32_t *d_counts = nullptr; uint32_t ntiles = 0;
    uint32_t *d_chunk_tot = nullptr;        // d_counts summed over chunks of OS_CHUNK tiles (sorts of more than OS_CHUNK_MIN_TILES tiles: k_tile_chunks)
    // The cell form of the hybrid sort's global stage (cd_sort.h, k_cell_scatter): keys per cell | a cursor per cell, 2 x CELLS words.  Both are zero between steps: a step in
    // the cell form clears them for the next (ZeroPlan), the classic form does not touch them, a step that did not clean up after itself leaves cell_clean false (one memset).
    uint32_t *d_cell = nullptr; bool cell_clean = false;
    bool cell_form = false;                 // the form the NEXT hybrid sort's global stage takes: chosen by choose_cell_form when a step's flags are judged, from the statistic that step's report carried
    bool cell_form_used = false;            // ... and the one the last sort took (CD_DBG_GET_SORT_CELLS)
    uint32_t dbg_sort_cells = 0;            // CD_DBG_SORT_CELLS: 0 the form the statistic asks for, 1 always the classic form (two onesweep passes), 2 always the cell form (A/B, tests)
    uint32_t cell_stat = 0;                 // the last judged step's statistic: cell changes among every wave of k_morton's 64 consecutive triangles, summed (CD_DBG_GET_CELL_STAT)
    // onesweep state, part of one scratch block (layout: cd_create): [8][256] u32 histograms | 8 u32 tickets (padded) | [8][ntiles][256] u64 granules
    void *d_os = nullptr; size_t os_bytes = 0 /* whole block */, zero_bytes = 0 /* its front part: all a fused call with the hybrid sort needs zeroed */, sort_hi_bytes = 0 /* of that, the sort's own */;
    unsigned long long *d_os_look_lo = nullptr;   // granules of the digit passes 0..5 (behind the front part); d_os_look: passes 6 and 7
    uint32_t *d_os_hist = nullptr; uint32_t *d_os_ticket = nullptr; unsigned long long *d_os_look = nullptr;
    double *d_frame = nullptr, *d_partial = nullptr;
    // tree
    unsigned long long *d_top_pub = nullptr; uint32_t top_seq = 0;          // k_cross_fused: the upper levels of the fp32 tree as its first workgroup publishes them, and the launch counter its flag word carries
    LeafTri *d_leaf = nullptr; NodeMeta *d_meta = nullptr; int32_t *d_parent = nullptr; double *d_seg = nullptr; float *d_seg32 = nullptr; uint32_t nbp2 = 1; int32_t *d_cross = nullptr; uint32_t cross_cap = 0;   // segment tree over leaf boxes: nbp2*512 heap nodes
    double *d_boxes = nullptr; uint32_t *d_bounded = nullptr; NodeRec32 *d_recs32 = nullptr; LeafBox32 *d_qbox = nullptr;
    unsigned long long *d_leaf_side = nullptr;   // fused build: one bit a leaf -- its box is in the left half of recs[j] (else the right half of recs[j - 1]); what k_cross_fused reads instead of qbox[]
    uint32_t dbg_big_offsets = 0;           // CD_DBG_BIG_OFFSETS: k_descend_half's 64-bit-address instance whatever n is (tests)
    uint32_t dbg_store_qbox = 0;            // CD_DBG_STORE_QBOX: the fused build always stores qbox[] (A/B, tests)
    // the cell table of the current vertices (cd_bvh.h AmbTable; amb_refresh): keys == nullptr while every coordinate is an fp32 value
    AmbTable amb = {nullptr, 0u, 0u};
    unsigned long long *d_amb_keys = nullptr, *d_amb_vals = nullptr; uint64_t amb_cap = 0; uint32_t *d_amb_flag = nullptr;
    bool cell_table_opt = true;             // CD_OPT_CELL_TABLE
    uint8_t *d_vamb = nullptr, *vamb = nullptr;   // per vertex: which of its three coordinates lie in ambiguous cells (vamb: d_vamb, or nullptr while there is no table)
    int32_t *d_root = nullptr;              // name (split) of the root record, one word inside d_small
    int32_t *d_split_of = nullptr;          // fused build: split of every internal node (child links of the records)
    uint32_t stamp_mask = 15;               // CD_OPT_KERNEL_STAMPS: with stage timing off, which time stamps a fused call still takes (1 block build, 2 descent, 4 exact, 8 pipeline start): ~5 us of idle GPU each
    uint32_t dbg_sort_windows = 0;          // CD_DBG_SORT_WINDOWS: 0 the form the size asks for, 1 always the large window form of k_local_sort, 2 always the small one (A/B, tests)
    bool left_frame = false; uint32_t steps_in_mode1 = 0;    // the sort went from its first form to its second because keys lay beyond bit 59 (not for a long run); sorts since then
    bool local_small_ok = true, local_small_active = false;   // the small window form has not met a run too long for it; the sort in flight used it
    uint32_t dbg_split_cross = 0;           // CD_DBG_SPLIT_CROSS: the fused build runs k_cross_meta + k_cross_records instead of k_cross_fused (A/B, tests)
    uint32_t dbg_no_fused_build = 0;        // CD_DBG_STAGEWISE_BUILD: fused entry points run k_hierarchy + the meta-reading refit (A/B)
    uint32_t *d_small = nullptr;            // 16 x u32 scratch counters (parent_wrong, check outputs)
    // traversal
    TravBuf tb[2];
    int exact_blocks = 1024;
    // pair-list post-processing (cd_sorted_pairs / cd_collision_triangles): sort buffers sized on demand
    uint64_t *pp_keys[2] = {nullptr, nullptr}; uint32_t *pp_vals[2] = {nullptr, nullptr}; uint32_t *pp_flags = nullptr;
    void *pp_os = nullptr; size_t pp_os_bytes = 0; uint32_t pp_cap = 0;
    uint64_t last_pairs_on_device = 0;      // pairs of the last traversal that are resident in d_pairs
    // What the enqueuers of a step leave behind ON THE HOST for whoever comes next.  A replayed graph runs no enqueuer, so graph_step puts this record (and stats.sort_passes) back as
    // its capture left it: a flag an enqueuer sets for later readers belongs HERE, or a replay differs from the stream path.  Written while enqueueing too, and deliberately outside:
    // order_ready and local_small_ok are part of the graph's KEY (a change captures again; local_small_active follows local_small_ok and CD_DBG_SORT_WINDOWS, both in the key),
    // order_pending is set and taken inside one enqueue_refit, top_seq and report_seq are counters a kernel compares against (never set back), last_pairs_on_device is
    // written by graph_step itself.
    struct StepLeft {
        bool leaves_filled = false;         // the sort's fix-up hop already wrote leaf[], parent = -1, bounded = 0
        bool leaf_records_filled = false;   // leaf[] holds the sorted triangles (leaves_filled: and parent[] / bounded[] are reset)
        bool hierarchy_valid = false;       // meta[] / parent[] hold the tree of the current keys (fused calls build the records without them)
        bool internal_boxes_valid = false;  // the FP64 boxes of the internal nodes were written by the last refit (fused calls skip them)
        bool last_tree_fused = false;       // the last fused call built hierarchy + refit in one pass (ms_hierarchy is then part of ms_refit)
        bool events_ride = false;           // the last pass recorded EV_TRAV0 / EV_DESC1 / EV_TRAV1 through its kernels' dispatch packets
        bool scratch_clean = false;         // the kernels of the last fused step left the scratch block zeroed (ZeroPlan, cd_build.h): the next one needs no memset at all
        bool qbox_valid = false;            // d_qbox holds THIS tree's query boxes (the fused build stores them only when somebody is known to read them: qbox_wanted / ensure_qbox)
    } left;
    // host mirrors
    cd_stats stats = {};
    uint32_t sort_flags[10] = {};           // [0..7] look-back time-out words of the last sort, [8] half-key fix-up overflow, [9] no flag: the cell statistic (k_morton), which travels with them; refreshed by read_state()
    bool stage_events = true;               // CD_OPT_STAGE_TIMING
    uint32_t dbg_report_copies = 0;        // CD_DBG_REPORT_COPIES: the report kernel copies the first pairs to the host (32 workgroups) instead of the exact kernel posting them (A/B)
    bool order_hint_large = false;          // CD_OPT_ORDER_HINT 2: also for trees of more than 1 M leaves (sorted chunk by chunk; measured slower there)
    bool order_hint = true;                 // CD_OPT_ORDER_HINT: the half traversal takes its groups of 64 leaves longest-first, by the previous step's times (cd_bvh.h, build_half_order)
    bool order_ready = false;               // d_order holds THIS tree's order hint (its fused build has made it)
    uint32_t *d_cost = nullptr, *d_order = nullptr;   // per group of 64 leaves: the score k_build_block gives it (max of its triangles' time classes); the order made from the scores
    bool order_pending = false;             // k_build_block has scored the groups: the k_cross_fused behind it sorts them
    uint8_t *d_tri_cost = nullptr;          // per triangle (original index): the time class its wave left in the last half traversal
    bool prezeroed = false;                 // fused path: the scratch block was zeroed by one memset at pipeline start
    hipEvent_t tree_done_event = nullptr;   // set by the multi-GPU step: taken (and cleared) by the launch that completes the tree, if it can carry it
    bool quiet_pass = false;                // launch_pass records no events (a pass on another stream, beside the one whose times are reported)
    int sort_mode = 0;                      // 0 hybrid on key bits 44..59 (every in-frame Morton key is below 2^60), 1 hybrid on bits 48..63 (2 global passes + in-LDS sort of the windows + fix-up), 2 half-key (4 passes + fix-up),
                                            // 2 full (8 passes); forced by CD_OPT_SORT_FULL, or escalated after an overflow on this context
    // CD_OPT_GRAPH: the steady-state fused step captured once as a hipGraph and replayed (graph_step); the key is everything a replay bakes in
    bool graph_opt = false;
    // CD_OPT_POLL: the step's end is read off the report's sequence word in pinned host memory instead of waiting for the stream (wait_report)
    bool poll_opt = true;
    unsigned long long report_seq = 0;      // last sequence number handed to a k_report
    uint32_t polled_steps = 0, poll_fallbacks = 0;
    // why a polled wait ran into its 20 ms budget (two such fall-backs in 360 000 stressed steps went unexplained): at the time-out the stream was still BUSY (the step itself was
    // late: queued behind other work, or the device stalled) / the stream had DRAINED and the word arrived with the synchronise (late in flight) / the word was not there even after the
    // stream had drained (LOST: the one that would be a bug of the protocol); and the longest polled wait that did end in the word, in microseconds
    uint32_t poll_fb_busy = 0, poll_fb_late_word = 0, poll_fb_lost = 0, poll_max_wait_us = 0;
    // CD_DBG_POLL_SCAN (tools/poll_stress.py, tests): the pair area the report kernel writes is filled with 0xff before every step and scanned the moment the
    // sequence word is seen -- a pair that is still 0xff then was overtaken by the word (poll_stale counts such steps: CD_DBG_GET_POLL_STALE; _FALLBACKS: the fall-backs to the stream)
    bool dbg_poll_check = false;
    uint32_t poll_stale = 0;
    hipGraph_t graph = nullptr; hipGraphExec_t graph_exec = nullptr;
    struct GraphKey { uint64_t cap, spec_n; int sort_mode, variant, frame_mode; uint32_t nt, exact_blocks, dbg; const void *p_pairs, *p_cand, *p_defer, *p_report; uint64_t cand_cap; uint32_t defer_cap, pad; } graph_key = {};   // (no padding bytes: compared with memcmp)
    struct GraphPost { StepLeft left; uint32_t sort_passes; } graph_post = {};   // what the captured step's enqueuers left on the host: a replay runs none of them
    uint64_t graph_replays = 0, graph_captures = 0;
    bool all_verts_referenced = false;      // every vertex belongs to a triangle (checked at cd_create; the topology never changes afterwards)
    int wall_clock_khz = 0;                 // hipDeviceAttributeWallClockRate: ticks of s_memrealtime per millisecond
    double root_box_host[6] = {};           // AABB of the whole tree, fetched together with other read-backs
    bool root_box_valid = false;
    // self-proximity (cd_find_proximity, cd_proximity.h): buffers of its own -- nothing the collision path keeps is touched
    PairBuf<ProxState> prox;
    // the self contour (cd_find_collisions_contour, cd_contour.h): buffers of its own, allocated on first use
    PairBuf<ProxState> cont;
    // continuous collision queries (cd_find_ccd, cd_ccd.h): buffers of their own, allocated on first use
    PairBuf<CcdState> ccd;
    DevArray<double> ccd_x1;                // the end positions, nv vertices
    // queries between two meshes (cd_find_*_between, cd_between.h) with this context as a: buffers of their own, allocated on first use and
    // grown to the other context's sizes (x1 of b, b's swept tree)
    PairBuf<CcdState> bw;
    DevArray<double> bw_x1a, bw_x1b;
    // the swept trees of the CCD passes: [0] this mesh's own (cd_find_ccd / cd_self_ccd), [1] b's, of cd_find_ccd_between with this context as a
    SweptBuf swept[2];
    int device = 0;                         // the HIP device ordinal current at cd_create (the between queries need both contexts on one device)
    // The per-item queries' buffers, each query's own, allocated on first use and grown to the largest count seen.  What a block or a
    // rows' vals holds, column by column, is the list in cd_columns.h named here.
    // ray queries (cd_cast_rays, cd_rays.h).  rays.block: RayCols
    ItemBuf<RayState> rays;
    // closest-point queries (cd_closest_points, cd_points.h).  points.block: PointCols
    ItemBuf<PointState> points;
    // nearest triangle / separation distance against another mesh (cd_nearest_between, cd_nearest.h) with this context as a: na + 1
    // rows (the last one: CD_NEAREST_MIN's).  nearest.block: NearestCols(self = false)
    ItemBuf<NearestState> nearest;
    // the same against the mesh itself (cd_nearest_self): nt + 1 rows of its own.  nearest_self.block: NearestCols(self = true)
    ItemBuf<NearestState> nearest_self;
    // all-results item queries (cd_points_within, cd_cast_rays_all, cd_within.h).
    // within.items: points [4 n], within.vals: WithinRowCols;   rays_all.items: rays [7 n], rays_all.vals: RayRowCols
    ItemRowsBuf within, rays_all;
    // swept-point queries (cd_sweep_points_all, cd_sweep_points, cd_sweep.h).
    // sweep.rows.items: items [7 n], sweep.rows.vals: SweepRowCols;   sweep.first.block: SweepFirstCols
    SweepBuf sweep;
    // inside / outside and signed distance (cd_points_inside, cd_signed_distance, cd_inside.h).  inside.block: InsideCols;
    // sdist.block: PointCols with inside for side; sdist.state: the closest-point kernel's counters, sdist_in: k_points_inside's
    ItemBuf<PointState> inside, sdist;
    StateWords<PointState> sdist_in;
    // box queries (cd_boxes_overlap_all, cd_boxes_count, cd_boxes.h).
    // boxes_all.items: boxes [6 n], boxes_all.vals: BoxRowCols;   boxes_count.block: BoxCountCols
    ItemRowsBuf boxes_all;
    ItemBuf<PointState> boxes_count;
    // plane queries (cd_planes_cut_all, cd_planes_count, cd_planes.h).
    // planes_all.items: planes [4 n], planes_all.vals: PlaneRowCols;   planes_count.block: PlaneCountCols
    ItemRowsBuf planes_all;
    ItemBuf<PointState> planes_count;
    // segment queries (cd_segments_within, cd_segments_closest, cd_segments.h).
    // segments_all.items: segments [7 n], segments_all.vals: SegmentRowCols;   segments.block: SegmentCols
    ItemRowsBuf segments_all;
    ItemBuf<PointState> segments;
    // swept-segment queries (cd_sweep_segments_all, cd_sweep_segments, cd_sweep_segments.h); the swept records, their counters and x1 are `sweep`'s.
    // sweep_segments.rows.items: items [13 n], sweep_segments.rows.vals: SweepSegmentRowCols;   sweep_segments.first.block: SweepSegmentCols
    SweepSegBuf sweep_segments;
};

namespace {

// k_cross_fused's published levels above the blocks (24 bytes a node, heap nodes [1, nbp2)) and, behind them, the flag word
// (a tree of more than TOP_IN_BLOCK blocks: from k_top_publish / k_top_publish_upper)
size_t top_pub_nodes(const cd_ctx *c) { return std::max<size_t>(TOP_IN_BLOCK, c->nbp2); }
size_t top_pub_bytes(const cd_ctx *c) { return sizeof(unsigned long long) * 3 * top_pub_nodes(c) + 64; }
uint32_t *top_flag_of(cd_ctx *c) { return reinterpret_cast<uint32_t *>(c->d_top_pub + 3 * top_pub_nodes(c)); }

void free_all(cd_ctx *c)
{
    hipFree(c->d_verts); hipFree(c->d_vidx); hipFree(c->d_ids);
    for (int i = 0; i < 2; ++i) { hipFree(c->d_keys[i]); hipFree(c->d_perm[i]); }
    hipFree(c->d_counts); hipFree(c->d_chunk_tot); hipFree(c->d_cell); hipFree(c->d_os); hipFree(c->d_frame); hipFree(c->d_partial);
    hipFree(c->d_top_pub); hipFree(c->d_leaf); hipFree(c->d_meta); hipFree(c->d_parent); hipFree(c->d_seg); hipFree(c->d_seg32); hipFree(c->d_cross); hipFree(c->d_boxes);
    hipFree(c->d_bounded); hipFree(c->d_recs32); hipFree(c->d_qbox); hipFree(c->d_leaf_side); hipFree(c->d_split_of); hipFree(c->d_cost); hipFree(c->d_order); hipFree(c->d_tri_cost);
    hipFree(c->d_amb_keys); hipFree(c->d_amb_flag); hipFree(c->d_vamb);
    for (TravBuf &tb : c->tb) {
        if (tb.d_pairs) hipFree(reinterpret_cast<char *>(tb.d_pairs) - sizeof(Report));
        if (tb.h_report) hipHostFree(tb.h_report);
        hipFree(tb.d_defer); hipFree(tb.d_deep); hipFree(tb.d_cand);
        if (tb.state_owned) hipFree(tb.d_state);
    }
    for (int i = 0; i < 2; ++i) { hipFree(c->pp_keys[i]); hipFree(c->pp_vals[i]); }
    hipFree(c->pp_flags); hipFree(c->pp_os);
    c->prox.release(); c->cont.release(); c->ccd.release(); c->bw.release(); c->ccd_x1.release(); c->bw_x1a.release(); c->bw_x1b.release();
    for (SweptBuf &sw : c->swept) sw.release();
    c->rays.release(); c->points.release(); c->nearest.release(); c->nearest_self.release(); c->within.release(); c->rays_all.release(); c->sweep.release();
    c->inside.release(); c->sdist.release(); c->sdist_in.release(); c->boxes_all.release(); c->boxes_count.release(); c->planes_all.release(); c->planes_count.release();
    c->segments_all.release(); c->segments.release(); c->sweep_segments.release();
    if (c->graph_exec) hipGraphExecDestroy(c->graph_exec);
    if (c->graph) hipGraphDestroy(c->graph);
    for (int i = 0; i < EV_COUNT; ++i) if (c->ev[i]) hipEventDestroy(c->ev[i]);
    if (c->stream) hipStreamDestroy(c->stream);
}

inline uint32_t cdiv(uint64_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }
inline uint32_t strided_grid(uint64_t n, uint32_t threads) { return std::min(cdiv(n, threads), 4096u); }   // the grid-stride kernels on explicit operands
inline uint32_t shard_blocks(uint32_t n) { return std::max(1u, std::min(64u, cdiv(n, 4096))); }             // exact stage of the pair queries: workgroups per shard
inline bool have_device() { int ndev = 0; return hipGetDeviceCount(&ndev) == hipSuccess && ndev != 0; }

// The device buffers of ONE call on explicit operands (no context, null stream): freed when the call returns.  e is the first HIP
// error; every operation after it does nothing and hands out nullptr, so the caller launches only while e == hipSuccess.
struct OneShot {
    hipError_t e = hipSuccess;
    void *owned[12] = {}; int n_owned = 0;
    OneShot() = default; OneShot(const OneShot &) = delete;
    ~OneShot() { for (int i = 0; i < n_owned; ++i) hipFree(owned[i]); }
    template <typename T> T *out(uint64_t count)                             // an output of `count` elements
    {
        void *p = nullptr;
        if (e == hipSuccess && n_owned == 12) e = hipErrorOutOfMemory;
        if (e == hipSuccess && (e = hipMalloc(&p, sizeof(T) * count)) == hipSuccess) owned[n_owned++] = p;
        return e == hipSuccess ? static_cast<T *>(p) : nullptr;
    }
    template <typename T> T *in(const T *host, uint64_t count)              // a host array, uploaded
    {
        T *p = out<T>(count);
        if (e == hipSuccess) e = hipMemcpy(p, host, sizeof(T) * count, hipMemcpyHostToDevice);
        return p;
    }
    template <typename T> void back(T *host, const T *dev, uint64_t count)  // an output copied back, if the caller asked for it
    {
        if (host && e == hipSuccess) e = hipMemcpy(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost);
    }
    int rc() const { return e == hipSuccess ? CD_OK : -(int)e; }
};

// An optional output of a per-item query on the context's stream.  wanted: the launch argument of its column -- the kernel writes it
// only if the caller asked; fetch: `elems` elements for each of n items copied back into the caller's array, if the caller asked
template <typename H, typename T> T *wanted(const H *host, T *dev) { return host ? dev : nullptr; }
template <typename T> int fetch(hipStream_t s, T *host, const T *dev, uint64_t elems, uint64_t n)
{
    if (host) HIPCHK(hipMemcpyAsync(host, dev, sizeof(T) * elems * n, hipMemcpyDeviceToHost, s));
    return CD_OK;
}
// after the synchronisation: the counters every per-item query reports (what it found, boxes visited, triangles tested), if asked for
template <class Info, class State> void item_info(Info *info, uint64_t found, const State *h)
{
    if (info) *info = Info{found, h->node_visits, h->tri_tests};
}

// pair buffers handed out by cd_alloc_host_pairs: pinned host memory the report kernel writes STRAIGHT into (no staging copy on the host)
// (id: a buffer's serial number -- an address the allocator hands out again is a NEW buffer, with pages the device has never written)
struct PinnedPairs { std::mutex mu; struct Buf { const uint32_t *p; uint64_t cap, id; }; std::vector<Buf> v; uint64_t next_id = 1; };
PinnedPairs &pinned_pairs() { static PinnedPairs p; return p; }
// 0: not a buffer of cd_alloc_host_pairs (or too small for `cap`); else the buffer's serial number
uint64_t pinned_pairs_id(const uint32_t *pairs, uint64_t cap)
{
    if (!pairs) return 0;
    PinnedPairs &pp = pinned_pairs();
    std::lock_guard<std::mutex> lock(pp.mu);
    for (const auto &e : pp.v) if (e.p == pairs && cap <= e.cap) return e.id;
    return 0;
}
constexpr uint64_t SPEC_PAIRS = 1u << 15;     // pairs that come back together with the counters, zero-copy (256 KB)

// morton.h:70-89 / :7-29 on explicit inputs (cd_morton3d_points, cd_expand64_values): the device functions k_morton uses
__global__ void k_morton_points(const double *__restrict__ xyz, uint64_t n, const double *__restrict__ frame /* FRAME_WORDS */, uint64_t *__restrict__ keys)
{
    const unsigned long long layout = (unsigned long long)__double_as_longlong(frame[6]);
    const KeyLayout kl = key_layout(layout, frame, frame + 3);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        keys[i] = layout ? morton3d_layout(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], kl) : morton3d(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], frame, frame + 3);
}
__global__ void k_expand_values(const uint64_t *__restrict__ v, uint64_t n, uint64_t *__restrict__ out)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = expand64(v[i]);
}

// box.cuh:24-32 / :40-43 and tri_contact.cuh:19-78 on explicit operands (cd_box_pairs, cd_tri_contact_points): the device functions
// the refit, the descent's FP64 leaf test and k_exact use
__global__ void k_box_pairs(const double *__restrict__ a, const double *__restrict__ b, uint64_t n, uint8_t *__restrict__ overlap,
                            double *__restrict__ merged)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const double *pa = a + 6 * i, *pb = b + 6 * i;
        const Box x{pa[0], pa[1], pa[2], pa[3], pa[4], pa[5]}, y{pb[0], pb[1], pb[2], pb[3], pb[4], pb[5]};
        if (overlap) overlap[i] = box_overlap(x, y) ? 1 : 0;
        if (merged) {
            const Box m = box_merge(x, y);
            double *o = merged + 6 * i;
            o[0] = m.x1; o[1] = m.x2; o[2] = m.y1; o[3] = m.y2; o[4] = m.z1; o[5] = m.z2;
        }
    }
}
__global__ void k_tri_contact_points(const double *__restrict__ t, uint64_t n, uint8_t *__restrict__ out)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const double *p = t + 18 * i;
        // (the form k_exact runs: hardware max / min, tri_contact itself where a projection is a NaN -- cd_math.h; the reference-compiled verdicts of tests/golden pin THIS)
        out[i] = tri_contact_fast(d3{p[0], p[1], p[2]}, d3{p[3], p[4], p[5]}, d3{p[6], p[7], p[8]},
                                  d3{p[9], p[10], p[11]}, d3{p[12], p[13], p[14]}, d3{p[15], p[16], p[17]}) ? 1 : 0;
    }
}

// ---- the cell table of the vertices (cd_bvh.h): which fp32 cells hold two distinct doubles of the same axis
__global__ void k_amb_scan(const double *__restrict__ v, uint64_t n3, uint32_t *__restrict__ flag)
{
    bool any = false;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n3; i += (uint64_t)gridDim.x * blockDim.x) { const double x = v[i]; any |= (double)(float)x != x; }
    if (__builtin_amdgcn_ballot_w64(any) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
// Slot h: keys[h] = the cell's key (| AMB_BIT once two distinct doubles were seen in it), vals[h] = the first double that claimed it
// (as an ordered integer; 0 = not yet written -- no double maps to 0).  A value that finds its cell's slot holding ANOTHER double marks
// the cell; one that finds its own double does nothing.  The pass is idempotent and order-independent: whatever the interleaving,
// a cell ends up marked iff two distinct doubles of the mesh lie in it.
__global__ void k_amb_insert(const double *__restrict__ v, uint64_t n3, unsigned long long *keys, unsigned long long *vals, uint32_t shift, uint32_t mask)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n3; i += (uint64_t)gridDim.x * blockDim.x) {
        double x = v[i];
        if (x == 0.0) x = 0.0;                                             // -0.0 and +0.0 are the same value
        const unsigned long long key = amb_key((int)(i % 3), amb_cell(x));
        uint32_t h = amb_hash(key, shift);
        // A mesh has far fewer distinct coordinates than vertices along its regular directions (a grid's columns share their x):
        // look before touching the slot with an atomic -- a thousand threads on one word retire one after the other.
        for (uint32_t probe = 0; probe <= mask; ++probe) {                 // (the table holds every key at a load below 2 / 3: this ends)
            unsigned long long old = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~AMB_BIT;
            if (old == 0ull) old = atomicCAS(&keys[h], 0ull, key) & ~AMB_BIT;
            if (old == 0ull || old == key) break;
            h = (h + 1u) & mask;
        }
        const unsigned long long o = f64_ordered(x);                       // (never 0: f64_ordered(-NaN with all bits set) aside, outside the contract)
        unsigned long long w = __hip_atomic_load(&vals[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == 0ull) w = atomicCAS(&vals[h], 0ull, o);
        if (w != 0ull && w != o && !(__hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & AMB_BIT)) atomicOr(&keys[h], AMB_BIT);
    }
}
// vamb[v]: bit a = the cell of vertex v's coordinate a is ambiguous (what the leaf encoding of the builds reads instead of six probes)
__global__ void k_amb_vertex(const double *__restrict__ verts, uint32_t nv, AmbTable t, uint8_t *__restrict__ vamb)
{
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += gridDim.x * blockDim.x) {
        const double x = verts[3 * (size_t)v], y = verts[3 * (size_t)v + 1], z = verts[3 * (size_t)v + 2];
        vamb[v] = (uint8_t)((amb_lookup(t, 0, x) ? 1u : 0u) | (amb_lookup(t, 1, y) ? 2u : 0u) | (amb_lookup(t, 2, z) ? 4u : 0u));
    }
}

constexpr int BOUNDS_BLOCKS = 1024;
constexpr uint32_t SORT_RETRY_STEPS = 64;          // sorts after which a context whose mesh had left the Morton frame tries the first sort form again
void graph_drop(cd_ctx *c);

int ensure_pairs(cd_ctx *c, TravBuf &tb, uint64_t cap)
{
    if (cap <= tb.pairs_cap) return 0;
    if (tb.d_pairs) hipFree(reinterpret_cast<char *>(tb.d_pairs) - sizeof(Report));
    tb.d_pairs = nullptr; tb.pairs_cap = 0;
    if (&tb == &c->tb[0]) c->last_pairs_on_device = 0;                 // the resident pair list went with the old buffer
    char *block = nullptr;
    HIPCHK(hipMalloc(&block, sizeof(Report) + sizeof(uint32_t) * 2 * cap + 16));      // +16: k_report moves pairs as 16-byte quads
    tb.d_pairs = reinterpret_cast<uint32_t *>(block + sizeof(Report));
    tb.pairs_cap = cap;
    return 0;
}

// (an event that was never recorded -- stage events off -- makes hipEventElapsedTime fail: that is "no measurement",
//  not an error of the call in progress, so the sticky last-error is cleared)
float elapsed(cd_ctx *c, int a, int b)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev[a], c->ev[b]) != hipSuccess) { (void)hipGetLastError(); return 0.f; }
    return ms;
}

// Per-stage events cost a few microseconds of idle GPU each (two per stage boundary).  With CD_OPT_STAGE_TIMING 0
// only the events the roofline needs are recorded: pipeline start, descent start / end, pipeline end.
inline hipError_t evrec(cd_ctx *c, int idx)
{
    if (!c->stage_events && !(idx == EV_MORTON0 || idx == EV_TRAV0 || idx == EV_DESC1 || idx == EV_TRAV1 || idx == EV_DEEP0 || idx == EV_DEEP1)) return hipSuccess;
    if (!c->stage_events && idx == EV_MORTON0 && !(c->stamp_mask & 8u)) return hipSuccess;
    return hipEventRecord(c->ev[idx], c->stream);
}

struct Prezeroed {                          // scope of a fused call: stage memsets are replaced by the one in enqueue_morton_sort
    cd_ctx *c;
    explicit Prezeroed(cd_ctx *c_) : c(c_) { c->prezeroed = true; }
    ~Prezeroed() { c->prezeroed = false; }
};

// ---- stage enqueuers (no host synchronisation inside) -------------------------------------------
static bool fused_build_next(const cd_ctx *c);
// links_too: the fix-up hop also resets the parent links / arrival counters (k_hierarchy and the stage-wise refit need them;
// the fused build does not)
// frame_ready: the caller has already run the bounds kernels of this step (the multi-GPU step needs the box of all triangles first)
int enqueue_morton_sort(cd_ctx *c, bool links_too = true, bool frame_ready = false)
{
    const uint32_t n = c->nt;
    hipStream_t s = c->stream;
    c->order_ready = false;                                                 // (the order hint belongs to a sorted order: this sort's fused build makes the next)
    HIPCHK(evrec(c, EV_MORTON0));
    // auto frame: per-block centroid bounds here (frame_ready: they are still there from this step's first sort); k_morton
    // folds them into the frame itself
    const bool auto_frame = c->frame_mode == CD_FRAME_AUTO;
    if (auto_frame && !frame_ready) k_centroid_bounds<false><<<BOUNDS_BLOCKS, 256, 0, s>>>(c->d_verts, c->d_vidx, n, c->d_partial);
    // fused pipeline: the sort scratch, the small counters and the traversal state are one block, zeroed once here
    // (the hybrid forms use the digit passes 6 and 7 only: their granules sit in the front part of the block, with the counters)
    // ... unless the previous fused step's own kernels have left the sort scratch zeroed and this step's kernels zero
    // the rest (k_local_sort: the small counters, k_build_block: the traversal counters; ZeroPlan, cd_build.h)
    const bool self_cleaning = c->prezeroed && c->sort_mode <= 1 && fused_build_next(c);
    const bool skip_memset = self_cleaning && c->left.scratch_clean;
    c->left.scratch_clean = false;
    if (!skip_memset) HIPCHK(hipMemsetAsync(c->d_os, 0, c->sort_mode <= 1 ? (c->prezeroed ? c->zero_bytes : c->sort_hi_bytes) : c->os_bytes, s));
    // Three forms of the same stable 64-bit sort (cd_sort.h): hybrid = the top 16 bits ordered globally (2 passes, or one launch that places
    // every key by its cell of those bits: `cells` below) + an in-LDS sort of run-aligned windows + the fix-up hop; half-key = 4 global passes on the high 32 bits + the fix-up hop;
    // full = 8 global passes.  The keys start in the buffer that leaves the sorted data in buffer 0.
    const int mode = c->sort_mode;
    const bool hybrid = mode <= 1;
    const int down = mode == 0 ? 4 : 0;         // mode 0: the two global digits are key bits 44..51 and 52..59 -- 16 bits that all vary,
                                                // where bits 48..63 of a 60-bit Morton key hold 12: runs 16 x shorter, windows of even size
    const int first_digit = hybrid ? 6 : (mode == 2 ? 4 : 0);
    int cur = mode == 3 ? 0 : 1;
    // The hybrid forms' global stage, classic (two onesweep passes) or by cells (one launch, no rendezvous: cd_sort.h); same result either way.  The cell arrays are
    // zero unless a step in the cell form went without its clean-up (no fused build behind it, or a raised flag).
    const bool cells = hybrid && c->cell_form;
    c->cell_form_used = cells;
    if (cells && !(skip_memset && c->cell_clean)) HIPCHK(hipMemsetAsync(c->d_cell, 0, sizeof(uint32_t) * 2 * CELLS, s));
    if (cells) { c->cell_clean = false; cur = 0; }                           // (one hop instead of two: the keys start in buffer 0, the window sort finds them in buffer 1 as always)
    const int cell_shift = hybrid ? 48 - down : -1;
    uint32_t *cell_hist = cells ? c->d_cell : nullptr, *cell_stat = c->d_os_ticket + 17;
    const uint32_t mblocks = c->ntiles < 2048u ? c->ntiles : 2048u;         // a workgroup per sort tile (4096 keys)
    unsigned long long host_layout = 0ull; std::memcpy(&host_layout, &c->frame_host[6], sizeof host_layout);
    const double *mframe = auto_frame ? nullptr : c->d_frame;               // (auto: the kernel folds the partial bounds itself and WRITES d_frame)
    const double *mpart = auto_frame ? c->d_partial : nullptr;
    if (auto_frame || host_layout != 0ull)
        k_morton<true><<<mblocks, MORTON_THREADS, 0, s>>>(c->d_verts, c->d_vidx, n, mframe, c->d_keys[cur], c->d_os_hist, first_digit, down, c->d_os_ticket + 16,
                                                          mpart, (uint32_t)BOUNDS_BLOCKS, c->d_frame, nullptr, c->d_counts, cell_shift, cell_hist, cell_stat + 1);
    else
        k_morton<false><<<mblocks, MORTON_THREADS, 0, s>>>(c->d_verts, c->d_vidx, n, mframe, c->d_keys[cur], c->d_os_hist, first_digit, down, c->d_os_ticket + 16,
                                                           mpart, (uint32_t)BOUNDS_BLOCKS, c->d_frame, nullptr, c->d_counts, cell_shift, cell_hist, cell_stat + 1);
    HIPCHK(evrec(c, EV_MORTON1));
    // onesweep: one pass over the data per digit; the digit histograms came with the keys
    // (more than 512 tiles: the first pass adds up chunk totals of the per-tile counts instead of every earlier tile's row -- cd_sort.h)
    const bool chunked = !cells && c->ntiles > (uint32_t)OS_CHUNK_MIN_TILES;
    if (cells) {
        k_cell_scatter<<<c->ntiles, OS_THREADS, 0, s>>>(c->d_keys[cur], c->d_keys[cur ^ 1], c->d_perm[cur ^ 1], n, cell_shift, c->d_os_hist + 7 * RADIX, HIST_COPIES,
                                                        c->d_cell, c->d_cell + CELLS, cell_stat);
    }
    if (chunked) k_tile_chunks<<<cdiv(c->ntiles, (uint32_t)OS_CHUNK), RADIX, 0, s>>>(c->d_counts, c->ntiles, c->d_chunk_tot);
    for (int pass = first_digit; pass < 8 && !cells; ++pass) {
        k_os_pass<<<c->ntiles, OS_THREADS, 0, s>>>(c->d_keys[cur], c->d_perm[cur], c->d_keys[cur ^ 1], c->d_perm[cur ^ 1], n, pass * RADIX_BITS - down,
                                                    c->d_os_hist + pass * RADIX,
                                                    (pass >= 6 ? c->d_os_look + (size_t)(pass - 6) * c->ntiles * RADIX : c->d_os_look_lo + (size_t)pass * c->ntiles * RADIX),
                                                    c->d_os_ticket + pass, pass == first_digit, HIST_COPIES, pass == first_digit ? c->d_counts : nullptr,
                                                    pass == first_digit && chunked ? c->d_chunk_tot : nullptr, pass == first_digit && hybrid ? cell_stat : nullptr);
        cur ^= 1;
    }
    c->left.leaves_filled = false; c->left.leaf_records_filled = false;
    if (hybrid) {                               // data is in buffer 1 again; windows go 1 -> 0, fix-up hop and leaf fill in the kernel's epilogue
        const LeafFill fill{c->d_vidx, c->d_ids, n, c->d_leaf, links_too ? c->d_parent : nullptr, links_too ? c->d_bounded : nullptr};
        // one workgroup per CU is all this kernel's LDS allows: the windows are n / 256 keys when that is less than their nominal
        // 4096 (1 M keys: 256 windows of 3907 instead of 245 of 4096 -- every CU busy, fewer windows over 4096 keys), not below 1024
        // (round 5) the SMALL form by default: windows of 2048 keys in workgroups of 512 threads and 48 KB, two of which share a CU (cd_sort.h) -- faster at every
        // size measured (100 k: 18.3 -> 14.4 us, 1 M cloth: 30.9 -> 27.8, 8 M: 269 -> 199); a run too long for it (3072 keys) is answered by the large form
        // (windows of 4096, runs up to 6144, one 1024-thread workgroup a CU) before the sort escalates to more global passes (judge_sort_flags)
        const bool small = c->dbg_sort_windows == 2 || (c->dbg_sort_windows == 0 && c->local_small_ok);
        c->local_small_active = small;
        if (small) {
            // (windows of n / 512 keys when that is less than the nominal 2048 -- two workgroups on every CU --, not below 512)
            const uint32_t per_half_cu = cdiv(n, 512u), win = per_half_cu >= (uint32_t)LocalSmall::W ? (uint32_t)LocalSmall::W : (per_half_cu < 512u ? 512u : per_half_cu);
            k_local_sort<LeafFill, LocalSmall><<<cdiv(n, win), LocalSmall::THREADS, 0, s>>>(c->d_keys[1], c->d_perm[1], c->d_keys[0], c->d_perm[0], n, 48 - down, c->d_os_ticket + 16, fill,
                                                                                            self_cleaning ? c->d_small : nullptr, self_cleaning ? 128u : 0u, win);
        } else {
            const uint32_t per_cu = cdiv(n, 256u), win = per_cu >= (uint32_t)LOCAL_W ? (uint32_t)LOCAL_W : (per_cu < 1024u ? 1024u : per_cu);
            k_local_sort<LeafFill, LocalLarge><<<cdiv(n, win), LocalLarge::THREADS, 0, s>>>(c->d_keys[1], c->d_perm[1], c->d_keys[0], c->d_perm[0], n, 48 - down, c->d_os_ticket + 16, fill,
                                                                                            self_cleaning ? c->d_small : nullptr, self_cleaning ? 128u : 0u, win);
        }
        c->left.leaves_filled = links_too;
        c->left.leaf_records_filled = true;
    } else if (mode != 3) {
        k_sort_fixup_fill<<<cdiv(n, 256), 256, 0, s>>>(c->d_keys[1], c->d_perm[1], c->d_keys[0], c->d_perm[0], n, c->d_os_ticket + 16,
                                                       c->d_vidx, c->d_ids, c->d_leaf, links_too ? c->d_parent : nullptr, links_too ? c->d_bounded : nullptr);
        c->left.leaves_filled = links_too;           // by the fix-up hop; enqueue_hierarchy runs k_fill_leaves otherwise
        c->left.leaf_records_filled = true;
    }
    c->stats.sort_passes = hybrid ? 2 : (mode == 2 ? 4 : 8);       // (8-bit digits ordered globally: two in either form of the hybrid sort's global stage)
    HIPCHK(evrec(c, EV_SORT1));
    HIPCHK(hipGetLastError());
    return 0;
}

int enqueue_hierarchy(cd_ctx *c, bool poison_boxes)
{
    const uint32_t n = c->nt;
    hipStream_t s = c->stream;
    HIPCHK(evrec(c, EV_HIER0));
    if (!c->prezeroed) HIPCHK(hipMemsetAsync(c->d_small, 0, 16 * sizeof(uint32_t), s));
    // (a repeated cd_build_hierarchy needs the parent links reset again: the flag is good for one use)
    if (!c->left.leaves_filled || poison_boxes)
        k_fill_leaves<<<cdiv(n, 256), 256, 0, s>>>(c->d_perm[0], c->d_vidx, c->d_ids, n, c->d_leaf, c->d_parent, c->d_bounded, poison_boxes ? c->d_boxes : nullptr);
    c->left.leaves_filled = false;
    if (n > 1)
        k_hierarchy<<<cdiv(n - 1, 256), 256, 0, s>>>(c->d_keys[0], (int)n, c->d_meta, c->d_parent, c->d_small);
    c->left.hierarchy_valid = true;
    HIPCHK(evrec(c, EV_HIER1));
    HIPCHK(hipGetLastError());
    return 0;
}

// fused: k_build_block (cd_build.h) builds hierarchy, fp32 boxes and records of its 512-leaf block itself, k_cross_meta /
// k_cross_records those of the cross nodes: no k_hierarchy before it, meta[] / parent[] / internal FP64 boxes are not written.
// Does anybody the build knows of read qbox[] after it?  The half traversal takes its query boxes out of the records and k_cross_fused its leaf pieces too (cd_build.h);
// the from-the-root descent (variant 1, and variant 0's tree comes from the stage-wise build anyway), k_cross_records, k_exact's FP64 path on a mesh with a cell table
// and the multi-GPU step's packers / external pass do read it.  Everybody else asks ensure_qbox() when the time comes.
static bool qbox_wanted(const cd_ctx *c)
{
    return c->trav_variant != 3 || c->dbg_split_cross || c->dbg_store_qbox || c->amb.keys != nullptr || c->amb.mask != 0u || c->attached_multi != nullptr;
}
int ensure_qbox(cd_ctx *c)
{
    if (c->left.qbox_valid) return 0;
    k_fill_qbox<<<cdiv(c->nt, 256), 256, 0, c->stream>>>(c->d_verts, c->d_leaf, (int)c->nt, c->d_qbox, c->amb, (const uint8_t *)c->vamb);
    HIPCHK(hipGetLastError());
    c->left.qbox_valid = true;
    return 0;
}
int enqueue_refit(cd_ctx *c, bool write_internal, bool fused = false)
{
    const uint32_t n = c->nt;
    hipStream_t s = c->stream;
    HIPCHK(evrec(c, EV_REFIT0));
    const int nblocks = (int)cdiv(n, REFIT_BLK);
    // the cross-node list (nodes whose range leaves their 512-leaf block) and its length, d_small[16]
    int32_t *cross_list = c->d_cross;
    uint32_t *cross_count = c->d_small + 16;
    if (!c->prezeroed) HIPCHK(hipMemsetAsync(cross_count, 0, 64 * sizeof(uint32_t), s));
    if (fused) {
        if (!c->left.leaf_records_filled)                 // (the 8-pass sort does not fill the leaves; enqueue_hierarchy would have)
            k_fill_leaves<<<cdiv(n, 256), 256, 0, s>>>(c->d_perm[0], c->d_vidx, c->d_ids, n, c->d_leaf, c->d_parent, c->d_bounded, nullptr);
        c->left.leaves_filled = false; c->left.leaf_records_filled = true;
        c->left.hierarchy_valid = false;
        // (its time stamps ride on its own dispatch packet: this is the largest kernel of the step, bench.py prices it)
        const bool stamp = (c->stamp_mask & 1u) != 0;
        const bool self_cleaning = c->prezeroed && c->sort_mode <= 1;
        ZeroPlan zp{nullptr, 0u, nullptr, 0u, nullptr, 0u, top_flag_of(c)};
        if (self_cleaning) {
            const size_t gran = sizeof(unsigned long long) * (size_t)c->ntiles * RADIX;
            zp = ZeroPlan{c->d_os_hist, (uint32_t)HIST_COPIES * 8u * RADIX + 8u /* histograms + tickets; the flags behind them stay */,
                          c->cell_form_used ? reinterpret_cast<uint4 *>(c->d_cell) : reinterpret_cast<uint4 *>(c->d_os_look),      // (the cell form wrote no granule: its cell arrays instead)
                          c->cell_form_used ? (uint32_t)(sizeof(uint32_t) * 2 * CELLS / sizeof(uint4)) : (uint32_t)(2 * gran / sizeof(uint4)),
                          reinterpret_cast<uint32_t *>(c->tb[0].d_state), (uint32_t)(sizeof(TravState) / sizeof(uint32_t)), top_flag_of(c)};
        }
        const int seg_min = (c->nbp2 > 1 && !c->dbg_split_cross) ? SEG32_MIN_LEVEL : SEG_MIN_LEVEL;
        // the half traversal's order hint (cd_bvh.h): this kernel scores the groups of 64 leaves, 8 workgroups of k_cross_fused sort them -- for trees that kernel serves
        // (trees of more than TOP_IN_BLOCK blocks -- more than 1 M leaves -- only with CD_OPT_ORDER_HINT 2: their descent runs many rounds of waves, the tail the hint packs is a
        //  tenth of it and the locality it gives up costs more -- 4 M cloth 173 -> 176 us, 8 M 454 -> 471 us with the hint)
        const bool hint = c->order_hint && c->trav_variant >= 3 && n > 64u && c->nbp2 > 1 && !c->dbg_split_cross && (c->nbp2 <= (uint32_t)TOP_IN_BLOCK || c->order_hint_large);
        const uint32_t *hp = hint ? c->d_perm[0] : nullptr; const uint8_t *ht = hint ? c->d_tri_cost : nullptr; uint32_t *hc = hint ? c->d_cost : nullptr;
        const int store_q = qbox_wanted(c) ? 1 : 0;
        c->left.qbox_valid = store_q != 0;
        if (stamp)
            hipExtLaunchKernelGGL(k_build_block, dim3(nblocks), dim3(REFIT_BLK), 0u, s, c->ev[EV_BLK0], c->ev[EV_BLK1], 0u,
                                  (const double *)c->d_verts, (const LeafTri *)c->d_leaf, (int)n, (const uint64_t *)c->d_keys[0], c->d_split_of,
                                  c->d_boxes, c->d_recs32, c->d_qbox, c->d_root, c->d_seg, c->d_seg32, (int)c->nbp2,
                                  cross_list, cross_count, c->cross_cap, zp, seg_min, c->amb, (const uint8_t *)c->vamb, hp, ht, hc, c->d_leaf_side, store_q);
        else                                        // (no time stamps: a plain launch, which a stream capture can record -- graph_step)
            k_build_block<<<nblocks, REFIT_BLK, 0, s>>>(c->d_verts, c->d_leaf, (int)n, c->d_keys[0], c->d_split_of, c->d_boxes, c->d_recs32, c->d_qbox, c->d_root,
                                                        c->d_seg, c->d_seg32, (int)c->nbp2, cross_list, cross_count, c->cross_cap, zp, seg_min, c->amb, (const uint8_t *)c->vamb,
                                                        hp, ht, hc, c->d_leaf_side, store_q);
        c->order_pending = hint;
        c->left.scratch_clean = self_cleaning;       // (judge_sort_flags takes it back when the sort has raised a flag)
        if (self_cleaning && c->cell_form_used) c->cell_clean = true;
    } else {
        c->left.qbox_valid = true;
        k_refit_seg_local<<<nblocks, REFIT_BLK, 0, s>>>(c->d_verts, c->d_leaf, (int)n, c->d_meta, c->d_boxes, c->d_bounded,
                                                       c->d_recs32, c->d_qbox, c->d_root, write_internal ? 1 : 0, c->d_seg, (int)c->nbp2,
                                                       cross_list, cross_count, c->cross_cap, c->amb, (const uint8_t *)c->vamb);
    }
    // fused build, a tree of 2 blocks or more: the cross nodes' ranges, splits, links and records in ONE launch (k_cross_fused, cd_build.h)
    if (fused && n > 1 && c->nbp2 > 1 && !c->dbg_split_cross) {
        const uint32_t xb = (uint32_t)nblocks < 8u ? 8u : ((uint32_t)nblocks > 1790u ? 1790u : (uint32_t)nblocks);   // 16 nodes per workgroup and round, ~13 per block; with the two workgroups below at most what the chip holds at once (7 workgroups per CU)
        // (the multi-GPU step's "tree is there" event rides on this kernel's dispatch packet: recorded on its own it is a barrier
        //  packet between the tree and the traversal, ~6 us of idle GPU)
        hipEvent_t done = c->tree_done_event; c->tree_done_event = nullptr;
        const uint32_t ogroups = (n + 63u) / 64u;
        const uint32_t nord = c->order_pending ? 8u * (((ogroups + 7u) / 8u + (uint32_t)ORDER_MAX_ITEMS - 1u) / (uint32_t)ORDER_MAX_ITEMS) : 0u;   // a workgroup per XCD list and chunk of it
        c->order_pending = false;
        const bool large = c->nbp2 > (uint32_t)TOP_IN_BLOCK;                // the upper levels come from launches of their own (below)
        const uint32_t xlds = std::max((uint32_t)(large ? 64u : sizeof(float) * 6 * (c->nbp2 >= 4 ? c->nbp2 / 4 : 1)) /* (used by the publishing workgroup only) */,
                                       nord ? (uint32_t)sizeof(OrderLds<256>) : 0u /* (the order hint's workgroups) */);
        uint32_t *top_flag = top_flag_of(c);
        if (++c->top_seq == 0u) ++c->top_seq;                               // (never 0: what k_build_block leaves in the flag word)
        if (large) {
            const int nspans = (int)(c->nbp2 / (uint32_t)TOP_IN_BLOCK);
            k_top_publish<<<nspans, 256, 0, s>>>(c->d_seg32, (int)c->nbp2, nblocks, c->d_top_pub);
            k_top_publish_upper<<<1, 256, 0, s>>>(c->d_top_pub, nspans, top_flag, c->top_seq);
        }
        if (done)
            hipExtLaunchKernelGGL(k_cross_fused, dim3(nord + xb + 2u /* [the order hint's 8,] then: the first workgroup publishes the upper levels, the last folds the FP64 box of all leaves */), dim3(256), xlds, s, nullptr, done, 0u,
                                  (const uint64_t *)c->d_keys[0], (int)n, (const double *)c->d_seg, (const float *)c->d_seg32, (int)c->nbp2, nblocks, (const unsigned long long *)c->d_leaf_side, c->d_boxes,
                                  c->d_recs32, (const int32_t *)c->d_split_of, c->d_root, (const int32_t *)c->d_cross, (const uint32_t *)cross_count, c->cross_cap,
                                  c->d_top_pub, top_flag, c->top_seq, nord, ogroups, (const uint32_t *)c->d_cost, c->d_order);
        else
            k_cross_fused<<<nord + xb + 2u, 256, xlds, s>>>(c->d_keys[0], (int)n, c->d_seg, c->d_seg32, (int)c->nbp2, nblocks, c->d_leaf_side, c->d_boxes,
                                                            c->d_recs32, c->d_split_of, c->d_root, c->d_cross, cross_count, c->cross_cap, c->d_top_pub, top_flag, c->top_seq,
                                                            nord, ogroups, c->d_cost, c->d_order);
        if (nord) c->order_ready = true;
        c->left.internal_boxes_valid = write_internal;
        HIPCHK(evrec(c, EV_REFIT1));
        HIPCHK(hipGetLastError());
        return 0;
    }
    // the levels above the blocks: a launch of their own -- unless the fused build's k_cross_meta can take them along (block 0)
    const bool top_in_meta = fused && n > 1 && c->nbp2 <= (uint32_t)TOP_IN_BLOCK;
    if (!top_in_meta) {
        if (fused && n > 1) {                    // a large tree: a workgroup per 2048 blocks, then the heap's upper part the same way
            int nb = (int)c->nbp2, live = nblocks;
            while (nb > 1) {
                const int span = nb < TOP_IN_BLOCK ? nb : TOP_IN_BLOCK;
                k_top_levels<<<nb / span, 256, 0, s>>>(c->d_seg, nb, live);
                nb /= span; live = (live + span - 1) / span;
            }
        } else k_refit_seg_top<<<1, 1024, 0, s>>>(c->d_seg, (int)c->nbp2, nblocks);
    }
    // about 13 cross nodes per 512-leaf block: ~one node per wave, every load chain in flight at once
    // one wave per cross node, about 13 of them per 512-leaf block: two workgroups (8 waves) per block -> 1-2 nodes per wave
    // (measured: 1024 / 2048 / 4096 / 8192 workgroups at 1 M triangles -> 120 / 113 / 111 / 112 us for the whole stage with the FP64
    //  kernels; k_cross_records alone with 2 .. 16 workgroups per block: no difference, 76 us for the stage)
    const uint32_t xblocks = 2u * nblocks < 256u ? 256u : (2u * nblocks > 16384u ? 16384u : 2u * (uint32_t)nblocks);
    if (fused && n > 1) {
        k_cross_meta<<<xblocks, 256, 0, s>>>(c->d_keys[0], (int)n, c->d_meta, c->d_split_of, c->d_cross, cross_count, c->cross_cap,
                                             top_in_meta ? c->d_seg : nullptr, (int)c->nbp2, nblocks);
        k_cross_records<<<xblocks, 256, 0, s>>>((int)n, c->d_meta, c->d_seg, c->d_seg32, (int)c->nbp2, c->d_qbox, c->d_boxes, c->d_recs32,
                                                c->d_split_of, c->d_root, c->d_cross, cross_count, c->cross_cap, c->amb);
    } else if (n > 1)
        k_refit_seg_cross<<<xblocks, 256, 0, s>>>((int)n, c->d_meta, c->d_seg, (int)c->nbp2, c->d_boxes, c->d_bounded, c->d_recs32,
                                                  c->d_root, write_internal ? 1 : 0, c->d_cross, cross_count, c->cross_cap, c->amb);
    c->left.internal_boxes_valid = write_internal;
    HIPCHK(evrec(c, EV_REFIT1));
    HIPCHK(hipGetLastError());
    return 0;
}

// Hierarchy + refit of a fused call: one pass that builds the records straight from the sorted keys (no k_hierarchy, no
// meta[] / parent[]), unless the traversal in use walks the reference-shaped tree (variant 0) or the A/B switch says so.
static bool fused_build_next(const cd_ctx *c) { return !(c->trav_variant == 0 || c->dbg_no_fused_build); }
int enqueue_tree(cd_ctx *c)
{
    c->left.last_tree_fused = false;
    if (!fused_build_next(c)) {
        int rc = enqueue_hierarchy(c, false);
        if (!rc) rc = enqueue_refit(c, c->trav_variant == 0, false);
        return rc;
    }
    c->left.last_tree_fused = true;
    return enqueue_refit(c, false, true);
}

// Launch one traversal pass (shallow: all queries from the root; deep: the deferred (query, subtree) items).
template <bool EXTERNAL, bool DEEP>
void launch_pass(cd_ctx *c, TravBuf &tb, const QuerySrc &src, uint32_t items, uint64_t cap_pairs)
{
    const int n = (int)c->nt;
    hipStream_t s = c->stream;
    const uint32_t vb = EXTERNAL ? c->vbase : 0u;
    if (c->trav_variant == 0) {
        k_traverse<EXTERNAL, DEEP><<<cdiv(items, TRAV_THREADS), TRAV_THREADS, 0, s>>>(src, items, n, c->d_meta, c->d_boxes, c->d_leaf, c->d_verts, tb.d_pairs, cap_pairs, tb.d_state,
                                                                                       DEEP ? nullptr : tb.d_defer, DEEP ? 0u : tb.defer_cap, DEEP ? tb.d_deep : nullptr, vb);
    } else {
        // variant 3 (half traversal) applies to self-collision queries; external queries are not leaves of this tree
        // and take the full descent of variant 1.  The deep pass of a half traversal continues (query, subtree) items
        // with the full descent, but its candidates keep the half traversal's meaning (`half`).
        const bool half_mode = c->trav_variant >= 3 && !EXTERNAL && (DEEP || items == (uint32_t)n);     // (k_descend_half derives its grid mapping from n: its queries are ALL the leaves)
        const uint32_t qpw = (DEEP || c->trav_variant >= 3) ? 64u : c->queries_per_wave;
        const uint64_t shard_cap = tb.cand_cap / NSHARD;
        const dim3 grid(cdiv(items, qpw * DESC_WAVES));
        const size_t pad = DEEP ? 0 : c->dbg_lds_pad;
        // Timing of the two kernels: with stage events on, hipEventRecord before / between / after (each record is a
        // barrier packet and ~6 us of idle GPU); off, the events ride on the kernels' own dispatch packets
        // (hipExtLaunchKernelGGL start / stop events): same timestamps, no gaps.
        const bool ride = !DEEP && !c->stage_events && !c->quiet_pass;
        hipEvent_t e0 = (ride && (c->stamp_mask & 2u)) ? c->ev[EV_TRAV0] : nullptr, e1 = (ride && (c->stamp_mask & 2u)) ? c->ev[EV_DESC1] : nullptr;
        hipEvent_t e2 = (ride && (c->stamp_mask & 4u)) ? c->ev[EV_TRAV1] : nullptr;
        const uint32_t qarg = qpw | (c->dbg_no_shared_path ? 0x40000000u : 0u);
        uint2 *dl = DEEP ? nullptr : tb.d_defer; const uint32_t dcap = DEEP ? 0u : tb.defer_cap; int32_t *deep = DEEP ? tb.d_deep : nullptr;
        const uint32_t half = half_mode ? 1u : 0u;
        const bool plain = !e0 && !e1 && !e2;          // no time stamp rides on these launches: plain launches (a stream capture can record them)
        if (half_mode && !DEEP) {
            const dim3 hgrid(cdiv(items, 64u)), hblock(HALF_THREADS);
            const uint32_t *h_order = (c->order_hint && c->order_ready) ? c->d_order : nullptr;      // (the order hint: cd_bvh.h, build_half_order)
            const bool h_rec = c->order_hint && (c->nbp2 <= (uint32_t)TOP_IN_BLOCK || c->order_hint_large);      // (the waves leave their times only where a build will read them)
            const uint32_t *h_perm = h_rec ? c->d_perm[0] : nullptr; uint8_t *h_tri = h_rec ? c->d_tri_cost : nullptr;
#define LAUNCH_HALF_(DIAG, TIES, BIG)                                                                                                           \
            do { if (plain) k_descend_half<DIAG, TIES, BIG><<<hgrid, hblock, pad, s>>>(src, n, c->d_recs32, tb.d_state, tb.d_cand, (unsigned long long)shard_cap, dl, dcap, h_order, h_perm, h_tri); \
                 else hipExtLaunchKernelGGL((k_descend_half<DIAG, TIES, BIG>), hgrid, hblock, (uint32_t)pad, s, e0, e1, 0u, src, n, (const NodeRec32 *)c->d_recs32, \
                                            tb.d_state, tb.d_cand, (unsigned long long)shard_cap, dl, dcap, h_order, h_perm, h_tri); } while (0)
            const bool ties = c->amb.keys != nullptr || c->amb.mask != 0u;                      // (a graph capture bakes the instance in: amb_refresh drops the graph when the table comes or goes)
            const bool big = n > HALF_SMALL_N || c->dbg_big_offsets;                            // (CD_DBG_BIG_OFFSETS: the tests run the 64-bit instance on trees of any size)
#define LAUNCH_HALF(DIAG, TIES) do { if (big) LAUNCH_HALF_(DIAG, TIES, true); else LAUNCH_HALF_(DIAG, TIES, false); } while (0)
            if (c->dbg_diag) { if (ties) LAUNCH_HALF(true, true); else LAUNCH_HALF(true, false); }
            else { if (ties) LAUNCH_HALF(false, true); else LAUNCH_HALF(false, false); }
#undef LAUNCH_HALF
#undef LAUNCH_HALF_
        }
        else if (qpw == 64)
            hipExtLaunchKernelGGL((k_descend<EXTERNAL, DEEP, false>), grid, dim3(DESC_THREADS), (uint32_t)pad, s, e0, e1, 0u,
                                  src, items, n, qarg, (const NodeRec32 *)c->d_recs32, (const double *)c->d_boxes, tb.d_state, tb.d_cand, (unsigned long long)shard_cap, dl, dcap, deep, vb, half);
        else
            hipExtLaunchKernelGGL((k_descend<EXTERNAL, DEEP, true>), grid, dim3(DESC_THREADS), (uint32_t)pad, s, e0, e1, 0u,
                                  src, items, n, qarg, (const NodeRec32 *)c->d_recs32, (const double *)c->d_boxes, tb.d_state, tb.d_cand, (unsigned long long)shard_cap, dl, dcap, deep, vb, half);
        if (!DEEP && !ride && !c->quiet_pass) evrec(c, EV_DESC1);
        uint32_t *post = DEEP ? nullptr : tb.post_dst; const unsigned long long post_n = DEEP ? 0ull : (unsigned long long)tb.post_n;
        if (!DEEP) { tb.posted = post != nullptr; tb.post_dst = nullptr; tb.post_n = 0; }     // (asked for by run_traversal for THIS pass only)
        if (plain)
            k_exact<EXTERNAL><<<c->exact_blocks, EXACT_THREADS, 0, s>>>(src, n, c->d_leaf, c->d_boxes, c->d_verts, vb, tb.d_cand, (unsigned long long)shard_cap, tb.d_pairs,
                                                                        (unsigned long long)cap_pairs, tb.d_state, half, post, post_n);
        else
            hipExtLaunchKernelGGL((k_exact<EXTERNAL>), dim3(c->exact_blocks), dim3(EXACT_THREADS), 0u, s, nullptr, e2, 0u,
                                  src, n, (const LeafTri *)c->d_leaf, (const double *)c->d_boxes, (const double *)c->d_verts, vb, (const Candidates *)tb.d_cand,
                                  (unsigned long long)shard_cap, tb.d_pairs, (unsigned long long)cap_pairs, tb.d_state, half, post, post_n);
        c->left.events_ride = ride;
    }
}

struct HostCounters { uint64_t n_pairs, pairs_tested, node_visits, max_shard_candidates; uint32_t n_deferred; uint64_t wave_steps, candidates, clk_start_inv, clk_end; };

// One host round trip and NO copy: k_report writes counters, the sort's time-out flags, the root box and the first
// spec_n pairs straight into pinned host memory.  enqueue_report queues the kernel; parse_report reads the record
// after the caller has synchronised the stream (the multi-GPU step queues two passes and synchronises once).
int ensure_report(TravBuf &tb)
{
    if (!tb.h_report) {
        // (coherent = fine-grained host memory: what the polled completion's system-scope release / acquire pair is defined on)
        HIPCHK(hipHostMalloc(&tb.h_report, sizeof(Report) + sizeof(uint32_t) * 2 * SPEC_PAIRS, hipHostMallocCoherent));
        std::memset(tb.h_report, 0, sizeof(Report));                       // (Report::seq: pinned memory is recycled by the allocator -- no stale sequence number)
    }
    return 0;
}
// direct: the first spec_n pairs go straight into the CALLER's buffer (pinned host memory from cd_alloc_host_pairs) instead of the staging area behind the record
int enqueue_report(cd_ctx *c, TravBuf &tb, bool want_pairs, uint64_t &spec_n, uint32_t *direct = nullptr, unsigned long long seq = 0)
{
    { const int rc = ensure_report(tb); if (rc) return rc; }
    if (!want_pairs) spec_n = 0; else if (spec_n > SPEC_PAIRS) spec_n = SPEC_PAIRS;
    // (the pair list is allocated with an even capacity + slack, so the quad copy may read one pair past `take`; a pinned buffer of
    //  cd_alloc_host_pairs has the same slack)
    constexpr int REPORT_BLOCKS = 32;
    // (the pass's exact kernel has posted the pairs itself: the report is the 256-byte record, one workgroup)
    const uint64_t copy_n = tb.posted ? 0 : spec_n;
    tb.posted = false;
    k_report<<<copy_n ? REPORT_BLOCKS : 1, REPORT_THREADS, 0, c->stream>>>(tb.d_state, c->d_os_ticket + 8, c->d_boxes, reinterpret_cast<Report *>(tb.h_report),
                                                              tb.d_pairs, direct ? direct : reinterpret_cast<uint32_t *>(tb.h_report + sizeof(Report)), (unsigned long long)copy_n, seq);
    return 0;
}
// Polled completion of a step (CD_OPT_POLL): spin on the sequence word k_report stores last.  Nothing that follows may need the
// stream's events (the caller checks: no stage events, no time stamps).  A step that takes longer than the spin budget, or never
// reports (a faulted kernel), ends in the ordinary stream synchronise, which also returns the error.  Every 64th polled step
// synchronises the stream as well, so that the runtime retires what it keeps per launch.
// Why the host may trust what it reads after seeing the word: DESIGN.md section 6 (system-scope release / acquire on fine-grained host memory,
// the HSA memory model's own guarantee -- the one the runtime's completion signal rests on too).  The first POLL_WARM reports into a report
// area (and into a caller's pinned buffer, told apart by serial number, not address) still end in a stream synchronise: not part of that
// argument, but free, and it makes the first steps of a context go through the path that also returns a launch's errors.
constexpr uint32_t POLL_WARM = 2;
// May this report be waited for by polling?  Also notes which pinned pair buffer the report goes to (a new one starts cold).
bool poll_this_report(const cd_ctx *c, TravBuf &tb, uint64_t direct_id)
{
    if (direct_id && direct_id != tb.direct_id) { tb.direct_id = direct_id; tb.synced_direct = 0; }     // (a step into an ordinary buffer in between does not make the pinned one cold again)
    return c->poll_opt && !c->stage_events && c->stamp_mask == 0 && tb.synced_reports >= POLL_WARM && (!direct_id || tb.synced_direct >= POLL_WARM);
}
int wait_report(cd_ctx *c, TravBuf &tb, unsigned long long seq)
{
    if (seq != 0ull) {
        const volatile unsigned long long *p = &reinterpret_cast<const volatile Report *>(tb.h_report)->seq;
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t it = 1; *p != seq; ++it) {
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
            if ((it & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        }
        if (*p == seq) {
            std::atomic_thread_fence(std::memory_order_acquire);
            if ((c->polled_steps & 15u) == 0) {                               // (a clock read every 16th step: what the longest ordinary wait is)
                const auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
                if ((uint64_t)us > c->poll_max_wait_us) c->poll_max_wait_us = (uint32_t)us;
            }
            if ((++c->polled_steps & 63u) == 0) HIPCHK(hipStreamSynchronize(c->stream));
            return 0;
        }
        ++c->poll_fallbacks;
        const hipError_t q = hipStreamQuery(c->stream);                       // busy: the step is late; drained: the word is
        (void)hipGetLastError();
        HIPCHK(hipStreamSynchronize(c->stream));
        if (q == hipErrorNotReady) ++c->poll_fb_busy;
        else if (*p == seq) ++c->poll_fb_late_word;
        else ++c->poll_fb_lost;
        return 0;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
void parse_report(cd_ctx *c, TravBuf &tb, HostCounters &h, uint32_t *spec_pairs, uint64_t spec_n)
{
    const Report &r = *reinterpret_cast<const Report *>(tb.h_report);
    h = HostCounters{r.n_pairs, r.pairs_tested, r.node_visits, r.max_shard_candidates, r.n_deferred, r.wave_steps, r.candidates, r.clk_start_inv, r.clk_end};
    std::memcpy(c->sort_flags, r.sort_flags, sizeof c->sort_flags);
    std::memcpy(c->root_box_host, r.root_box, sizeof(double) * 6);
    if (spec_n && spec_pairs) {
        const uint64_t take = r.n_pairs < spec_n ? r.n_pairs : spec_n;
        std::memcpy(spec_pairs, tb.h_report + sizeof(Report), sizeof(uint32_t) * 2 * take);
    }
}
// What read_state needs decided before it enqueues the report -- is the step's end polled (its sequence number), is the pair area poisoned for the scan -- decided here, so that
// run_traversal can do it BEFORE the pass's kernels are enqueued: with `post` the pass's exact kernel stores the first pairs into the pinned area itself (k_exact), and a poison
// written after that would be written over the pairs.
int prepare_report(cd_ctx *c, TravBuf &tb, uint32_t *spec_pairs, uint64_t spec_n, uint64_t direct_id, bool post)
{
    if (ensure_report(tb)) return CD_ERR_ARG;
    const bool direct = direct_id != 0;
    if (spec_n > SPEC_PAIRS) spec_n = SPEC_PAIRS;
    tb.prep_seq = poll_this_report(c, tb, direct_id) ? ++c->report_seq : 0ull;
    tb.prep_area = nullptr;
    uint32_t *dst = direct ? spec_pairs : reinterpret_cast<uint32_t *>(tb.h_report + sizeof(Report));
    if (c->dbg_poll_check && tb.prep_seq && spec_pairs && spec_n) {
        tb.prep_area = dst;
        std::memset(dst, 0xff, sizeof(uint32_t) * 2 * spec_n);
    }
    tb.post_dst = (post && spec_pairs && spec_n) ? dst : nullptr;
    tb.post_n = tb.post_dst ? spec_n : 0;
    tb.prepared = true;
    return 0;
}
int read_state(cd_ctx *c, TravBuf &tb, HostCounters &h, uint32_t *spec_pairs = nullptr, uint64_t spec_n = 0, uint64_t direct_id = 0)
{
    if (ensure_report(tb)) return CD_ERR_ARG;
    const bool direct = direct_id != 0;
    if (!tb.prepared) prepare_report(c, tb, spec_pairs, spec_n, direct_id, false);
    const unsigned long long seq = tb.prep_seq;
    uint32_t *area = tb.prep_area;
    tb.prepared = false; tb.post_dst = nullptr; tb.post_n = 0;
    int rc = enqueue_report(c, tb, spec_pairs != nullptr, spec_n, direct ? spec_pairs : nullptr, seq);
    if (rc) return rc;
    const uint32_t fb0 = c->poll_fallbacks;
    if ((rc = wait_report(c, tb, seq))) return rc;
    if (seq == 0ull) { ++tb.synced_reports; if (direct) ++tb.synced_direct; }
    if (area && c->poll_fallbacks == fb0) {
        const Report &r = *reinterpret_cast<const Report *>(tb.h_report);
        const uint64_t take = r.n_pairs < spec_n ? r.n_pairs : spec_n;
        bool stale = false;
        for (uint64_t i = 0; i < 2 * take; ++i) stale |= reinterpret_cast<volatile uint32_t *>(area)[i] == 0xffffffffu;
        if (stale) ++c->poll_stale;
    }
    parse_report(c, tb, h, direct ? nullptr : spec_pairs, spec_n);          // (direct: the pairs are already where the caller wants them)
    return 0;
}

// Did a shard of the candidate buffer overflow in the pass `h` reports?  (Nothing is written past a shard; the step is redone.)
bool shards_overflowed(const TravBuf &tb, const HostCounters &h) { return h.max_shard_candidates > tb.cand_cap / NSHARD; }
int grow_candidates(cd_ctx *c, TravBuf &tb, uint64_t max_shard);
int grow_shards(cd_ctx *c, TravBuf &tb, const HostCounters &h) { return grow_candidates(c, tb, h.max_shard_candidates); }
int grow_candidates(cd_ctx *c, TravBuf &tb, uint64_t max_shard)
{
    hipFree(tb.d_cand); tb.d_cand = nullptr; tb.cand_cap = 0;
    const uint64_t want = ((max_shard + max_shard / 4 + 1024 + 3) & ~3ull) * NSHARD;          // (a shard: a multiple of 4 slots -- FatPair entries are counted from its end, cd_traverse.h)
    HIPCHK(hipMalloc(&tb.d_cand, sizeof(Candidates) * want));
    tb.cand_cap = want;
    return 0;
}

// Traversal (local leaves or external queries).  Blocks: reads the counters, runs the deep pass when needed.
int run_traversal(cd_ctx *c, TravBuf &tb, const void *d_ext, uint64_t nq_ext, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs)
{
    const uint32_t n = c->nt;
    hipStream_t s = c->stream;
    const bool external = d_ext != nullptr;
    const uint32_t nq = external ? (uint32_t)nq_ext : n;
    int rc = ensure_pairs(c, tb, cap_pairs > 0 ? cap_pairs : 1);
    if (rc) return rc;
    const int per_pass = c->trav_variant == 0 ? 1 : 2;             // descent + exact kernel
    if (c->trav_variant == 0 && !(c->left.internal_boxes_valid && c->left.hierarchy_valid)) {   // variant 0 walks meta[] and the FP64 boxes of the internal nodes
        if (!c->left.hierarchy_valid && (rc = enqueue_hierarchy(c, false))) return rc;
        if ((rc = enqueue_refit(c, true, false))) return rc;
    }
    // (the from-the-root descent reads its query boxes from qbox[], k_exact the leaf boxes of candidates that are not certain -- external queries against a tree whose
    //  build did not store them: filled here, once per tree)
    if (c->trav_variant != 0 && (external || c->trav_variant < 3) && (rc = ensure_qbox(c))) return rc;
    uint32_t launches = 0;
    float deep_ms = 0.f;
    HostCounters h = {};
    uint64_t spec_valid = 0;
    bool done = false;
    c->stats.stack_overflows = 0;
    for (int attempt = 0; attempt < 8 && !done; ++attempt) {
        launches = 0; deep_ms = 0.f;
        QuerySrc src{c->d_leaf, c->d_boxes, c->d_qbox, c->d_root, d_ext, nullptr, c->d_os_ticket + 8};
        const bool will_ride = !c->stage_events && (c->trav_variant == 1 || c->trav_variant >= 3) && nq > 0;   // see launch_pass: events on the dispatch packets
        c->left.events_ride = false;
        if (!will_ride) HIPCHK(evrec(c, EV_TRAV0));
        if (!(c->prezeroed && attempt == 0 && &tb == &c->tb[0])) HIPCHK(hipMemsetAsync(tb.d_state, 0, sizeof(TravState), s));
        const uint64_t spec_n = pairs ? (cap_pairs < SPEC_PAIRS ? cap_pairs : SPEC_PAIRS) : 0;
        // (the exact kernel posts the first pairs itself when it is the one that appends them: every traversal but variant 0's)
        if ((rc = prepare_report(c, tb, pairs, spec_n, pinned_pairs_id(pairs, cap_pairs), c->trav_variant != 0 && nq > 0 && !c->dbg_report_copies))) return rc;
        if (nq > 0) {
            if (external) launch_pass<true, false>(c, tb, src, nq, cap_pairs); else launch_pass<false, false>(c, tb, src, nq, cap_pairs);
            launches += per_pass;
        }
        if (!c->left.events_ride) HIPCHK(evrec(c, EV_TRAV1));      // device time of the kernels only: recorded before the read-back
        if ((rc = read_state(c, tb, h, pairs, spec_n, pinned_pairs_id(pairs, cap_pairs)))) return rc;
        spec_valid = spec_n;
        if (shards_overflowed(tb, h)) { if ((rc = grow_shards(c, tb, h))) return rc; continue; }
        if (h.n_deferred > tb.defer_cap) {               // the deferred list was too small: grow it and redo (pairs restart at 0)
            hipFree(tb.d_defer); tb.d_defer = nullptr; tb.defer_cap = 0;
            HIPCHK(hipMalloc(&tb.d_defer, sizeof(uint2) * (size_t)h.n_deferred));
            tb.defer_cap = h.n_deferred;
            continue;
        }
        if (h.n_deferred > 0) {                          // deep pass over the deferred (query, subtree) items
            const uint32_t nd = h.n_deferred;
            const uint64_t deep_lanes = (uint64_t)cdiv(nd, 64) * 64 + 256;
            if (deep_lanes > tb.deep_items) {
                hipFree(tb.d_deep); tb.d_deep = nullptr; tb.deep_items = 0;
                HIPCHK(hipMalloc(&tb.d_deep, sizeof(int32_t) * (size_t)DEEP_STACK * deep_lanes));
                tb.deep_items = deep_lanes;
            }
            if (c->trav_variant != 0 && (rc = ensure_qbox(c))) return rc;      // (the deep pass continues with the from-the-root descent)
            HIPCHK(evrec(c, EV_DEEP0));
            HIPCHK(hipMemsetAsync(&tb.d_state->n_deferred, 0, sizeof(uint32_t), s));
            // candidate shards restart from 0: the shallow pass's candidates have all been consumed by k_exact
            for (int i = 0; i < NSHARD; ++i) { /* one memset per shard would be 64 calls: clear them with a 2-D memset */ }
            HIPCHK(hipMemset2DAsync(&tb.d_state->shard[0].n_candidates, sizeof(CtrShard), 0, sizeof(unsigned long long), NSHARD, s));
            src.list = tb.d_defer;
            if (external) launch_pass<true, true>(c, tb, src, nd, cap_pairs); else launch_pass<false, true>(c, tb, src, nd, cap_pairs);
            launches += per_pass;
            HIPCHK(evrec(c, EV_DEEP1));
            if ((rc = read_state(c, tb, h))) return rc;
            if (h.n_deferred != 0) return CD_ERR_ARG;    // tree deeper than DEEP_STACK: cannot happen (height <= 96)
            if (shards_overflowed(tb, h)) { if ((rc = grow_shards(c, tb, h))) return rc; continue; }
            c->stats.stack_overflows = nd;
            deep_ms = elapsed(c, EV_DEEP0, EV_DEEP1);            // (always recorded: a deep pass is device time of this traversal)
        }
        done = true;
    }
    if (!done) return CD_ERR_ARG;
    HIPCHK(hipGetLastError());
    const uint64_t found = h.n_pairs;
    const uint64_t ncopy = found < cap_pairs ? found : cap_pairs;
    // the first spec_valid pairs came back with the counters -- unless a deep pass appended more afterwards
    const uint64_t have = (c->stats.stack_overflows == 0) ? spec_valid : 0;
    if (pairs && ncopy > have) {
        HIPCHK(hipMemcpyAsync(pairs + 2 * have, tb.d_pairs + 2 * have, sizeof(uint32_t) * 2 * (ncopy - have), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    // (a time stamp that was not taken in this call must not be read: the event holds an earlier call's)
    const bool have_d = !c->left.events_ride || (c->stamp_mask & 2u), have_x = !c->left.events_ride || (c->stamp_mask & 4u);
    c->stats.ms_traverse = (have_d && have_x) ? elapsed(c, EV_TRAV0, EV_TRAV1) + deep_ms : 0.f;
    c->stats.ms_descend = (c->trav_variant != 0 && nq > 0 && have_d) ? elapsed(c, EV_TRAV0, EV_DESC1) : 0.f;
    c->stats.ms_exact = (c->trav_variant != 0 && nq > 0 && have_d && have_x) ? elapsed(c, EV_DESC1, EV_TRAV1) : 0.f;
    c->stats.traverse_launches = launches;
    c->stats.n_pairs = found; c->stats.pairs_tested = h.pairs_tested; c->stats.node_visits = h.node_visits;
    c->stats.wave_steps = h.wave_steps; c->stats.candidates = h.candidates;
    // the descent kernel's own clock (k_descend_half): first wave start -> last wave end, in ticks of the device's constant wall clock
    c->stats.ms_descend_clock = (h.clk_end && h.clk_start_inv && c->wall_clock_khz > 0 && c->stats.stack_overflows == 0)
                                    ? (float)((double)(h.clk_end - ~h.clk_start_inv) / (double)c->wall_clock_khz) : 0.f;
    c->last_pairs_on_device = found <= cap_pairs ? found : cap_pairs;
    if (n_pairs) *n_pairs = found;
    return found > cap_pairs ? CD_OVERFLOW : CD_OK;
}


// ---- pair-list post-processing -----------------------------------------------------------------------
int pp_reserve(cd_ctx *c, uint32_t m)
{
    if (m <= c->pp_cap) return 0;
    for (int i = 0; i < 2; ++i) { hipFree(c->pp_keys[i]); hipFree(c->pp_vals[i]); c->pp_keys[i] = nullptr; c->pp_vals[i] = nullptr; }
    hipFree(c->pp_flags); hipFree(c->pp_os); c->pp_flags = nullptr; c->pp_os = nullptr; c->pp_cap = 0;
    const uint32_t cap = m + m / 4 + 4096;
    const uint32_t ntiles = cdiv(cap, SORT_TILE);
    for (int i = 0; i < 2; ++i) { HIPCHK(hipMalloc(&c->pp_keys[i], sizeof(uint64_t) * cap)); HIPCHK(hipMalloc(&c->pp_vals[i], sizeof(uint32_t) * cap)); }
    HIPCHK(hipMalloc(&c->pp_flags, sizeof(uint32_t) * cap));
    c->pp_os_bytes = sizeof(uint32_t) * 8 * RADIX + 64 + sizeof(unsigned long long) * 8 * (size_t)ntiles * RADIX;
    HIPCHK(hipMalloc(&c->pp_os, c->pp_os_bytes));
    c->pp_cap = cap;
    return 0;
}

// Ascending radix sort of pp_keys[0][0..m) (onesweep, cd_sort.h); result back in pp_keys[0].
int pp_sort(cd_ctx *c, uint32_t m)
{
    hipStream_t s = c->stream;
    const uint32_t ntiles = cdiv(m, SORT_TILE);
    uint32_t *hist = reinterpret_cast<uint32_t *>(c->pp_os);
    uint32_t *ticket = hist + 8 * RADIX;
    unsigned long long *look = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(c->pp_os) + sizeof(uint32_t) * 8 * RADIX + 64);
    HIPCHK(hipMemsetAsync(c->pp_os, 0, sizeof(uint32_t) * 8 * RADIX + 64 + sizeof(unsigned long long) * 8 * (size_t)ntiles * RADIX, s));
    k_os_hist<<<cdiv(m, SORT_THREADS * 8) < 1024u ? cdiv(m, SORT_THREADS * 8) : 1024u, SORT_THREADS, 0, s>>>(c->pp_keys[0], m, hist);
    int cur = 0;
    for (int pass = 0; pass < 8; ++pass) {
        k_os_pass<<<ntiles, OS_THREADS, 0, s>>>(c->pp_keys[cur], c->pp_vals[cur], c->pp_keys[cur ^ 1], c->pp_vals[cur ^ 1], m, pass * RADIX_BITS,
                                                hist + pass * RADIX, look + (size_t)pass * ntiles * RADIX, ticket + pass, pass == 0, 1, nullptr, nullptr, nullptr);
        cur ^= 1;
    }
    return 0;
}

int judge_sort_flags(cd_ctx *c);
// ---- CD_OPT_GRAPH: the steady-state fused step as ONE hipGraph launch ------------------------------------------------
// Eligible: no stage events, no time stamps, hybrid sort, fused build, half traversal, and a previous step has left the
// scratch clean (so the captured sequence holds kernels only: no memset).  The capture records exactly what the stream path
// enqueues -- k_morton, 2 x k_os_pass or k_cell_scatter, k_local_sort, k_build_block, k_cross_fused, k_descend_half, k_exact, k_report -- with
// the arguments of this call baked in; any change of those (capacity, buffers grown, options) captures again.  Whatever the
// report says that the stream path would answer with a retry -- a sort flag, a candidate shard that overflowed, a deferred
// subtree -- is handed to the stream path (handled = false, or run_traversal on the tree that is there).
void graph_drop(cd_ctx *c)
{
    if (c->graph_exec) { hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
    if (c->graph) { hipGraphDestroy(c->graph); c->graph = nullptr; }
}
// The cell table follows the VERTICES: rebuilt by cd_create / cd_update_vertices (after their copy), never inside a step.  Every
// coordinate an fp32 value -- the reference's loader produces those (load_obj.h:38) -- : one streaming pass, no table.
int amb_refresh(cd_ctx *c)
{
    hipStream_t s = c->stream;
    const uint64_t n3 = 3ull * c->nv;
    if (!c->d_amb_flag) HIPCHK(hipMalloc(&c->d_amb_flag, sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(c->d_amb_flag, 0, sizeof(uint32_t), s));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n3 + 255) / 256, 4096);
    k_amb_scan<<<blocks, 256, 0, s>>>(c->d_verts, n3, c->d_amb_flag);
    uint32_t inexact = 0;
    HIPCHK(hipMemcpyAsync(&inexact, c->d_amb_flag, sizeof inexact, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const AmbTable before = c->amb;
    if (!inexact) { c->amb = AmbTable{nullptr, 0u, 0u}; c->vamb = nullptr; }
    else if (!c->cell_table_opt) { c->amb = AmbTable{nullptr, 0u, 1u}; c->vamb = nullptr; }      // every inexact coordinate counts as ambiguous: plain outward rounding
    else {
        uint64_t cap = 1024; uint32_t lg = 10;
        while (cap < n3 + n3 / 2) { cap <<= 1; ++lg; }                      // load below 2 / 3
        if (cap > (1ull << 32)) return CD_ERR_ARG;
        if (cap != c->amb_cap) {
            hipFree(c->d_amb_keys); c->d_amb_keys = c->d_amb_vals = nullptr; c->amb_cap = 0;
            HIPCHK(hipMalloc(&c->d_amb_keys, sizeof(unsigned long long) * 2 * cap));       // keys | vals, one allocation, one memset
            c->d_amb_vals = c->d_amb_keys + cap;
            c->amb_cap = cap;
        }
        HIPCHK(hipMemsetAsync(c->d_amb_keys, 0, sizeof(unsigned long long) * 2 * cap, s));
        const uint32_t shift = 64u - lg, mask = (uint32_t)(cap - 1);
        k_amb_insert<<<blocks, 256, 0, s>>>(c->d_verts, n3, c->d_amb_keys, c->d_amb_vals, shift, mask);
        c->amb = AmbTable{c->d_amb_keys, shift, mask};
        if (!c->d_vamb) HIPCHK(hipMalloc(&c->d_vamb, c->nv));
        k_amb_vertex<<<(uint32_t)std::min<uint64_t>((c->nv + 255ull) / 256, 4096), 256, 0, s>>>(c->d_verts, c->nv, c->amb, c->d_vamb);
        c->vamb = c->d_vamb;
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
    }
    if (before.keys != c->amb.keys || before.shift != c->amb.shift || before.mask != c->amb.mask) graph_drop(c);       // (a captured step has the table baked into its launches)
    return CD_OK;
}
bool graph_eligible(const cd_ctx *c)
{
    return c->graph_opt && !c->stage_events && c->stamp_mask == 0 && c->sort_mode <= 1 && fused_build_next(c) && c->trav_variant == 3 &&
           c->left.scratch_clean && (!c->cell_form || c->cell_clean) /* (no memset in a captured step) */ && !c->dbg_diag && !c->dbg_lds_pad && c->nt > 1 && c->tree_done_event == nullptr;
}
int graph_step(cd_ctx *c, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs, bool &handled)
{
    handled = false;
    TravBuf &tb = c->tb[0];
    hipStream_t s = c->stream;
    int rc = ensure_pairs(c, tb, cap_pairs > 0 ? cap_pairs : 1);
    if (!rc) rc = ensure_report(tb);
    if (rc) return rc;
    uint64_t spec_n = pairs ? (cap_pairs < SPEC_PAIRS ? cap_pairs : SPEC_PAIRS) : 0;
    const bool direct = pinned_pairs_id(pairs, cap_pairs) != 0;
    const cd_ctx::GraphKey key{cap_pairs, spec_n, c->sort_mode, c->trav_variant, c->frame_mode, c->nt, (uint32_t)c->exact_blocks, c->dbg_no_shared_path | (c->dbg_split_cross << 1) | (c->order_hint ? 4u : 0u) | (c->order_ready ? 8u : 0u) | (c->local_small_ok ? 16u : 0u) | (c->dbg_sort_windows << 5) | (qbox_wanted(c) ? 128u : 0u) | (c->cell_form ? 256u : 0u) /* (whether the descent's launch reads the order hint is baked in) */,
                               tb.d_pairs, tb.d_cand, tb.d_defer, direct ? (const void *)pairs : (const void *)tb.h_report, tb.cand_cap, tb.defer_cap, 0u};
    static_assert(sizeof(cd_ctx::GraphKey) == 2 * 8 + 6 * 4 + 4 * 8 + 8 + 2 * 4, "GraphKey has no padding");
    if (!c->graph_exec || std::memcmp(&key, &c->graph_key, sizeof key) != 0) {
        graph_drop(c);
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        c->prezeroed = true;
        rc = enqueue_morton_sort(c, false);
        if (!rc) rc = enqueue_tree(c);
        if (!rc) {
            QuerySrc src{c->d_leaf, c->d_boxes, c->d_qbox, c->d_root, nullptr, nullptr, c->d_os_ticket + 8};
            launch_pass<false, false>(c, tb, src, c->nt, cap_pairs);
            rc = enqueue_report(c, tb, pairs != nullptr, spec_n, direct ? pairs : nullptr);
        }
        c->prezeroed = false;
        hipGraph_t g = nullptr;
        const hipError_t ee = hipStreamEndCapture(s, &g);
        if (rc || ee != hipSuccess || !g) { if (g) hipGraphDestroy(g); (void)hipGetLastError(); c->left.scratch_clean = false; return CD_OK; }   // (not handled: the stream path runs, with its memset)
        c->graph = g;
        if (hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0) != hipSuccess) { graph_drop(c); (void)hipGetLastError(); c->left.scratch_clean = false; return CD_OK; }
        std::memset(&c->graph_key, 0, sizeof c->graph_key);
        c->graph_key = key;
        c->graph_post = {c->left, c->stats.sort_passes};
        ++c->graph_captures;
    }
    // what the enqueue functions leave behind on the host side, as the capture left it
    c->left = c->graph_post.left; c->stats.sort_passes = c->graph_post.sort_passes;
    c->cell_form_used = c->cell_form;                                       // (the form is part of the key: the captured step's)
    HIPCHK(hipGraphLaunch(c->graph_exec, s));
    HIPCHK(hipStreamSynchronize(s));
    ++c->graph_replays;
    HostCounters h = {};
    parse_report(c, tb, h, direct ? nullptr : pairs, spec_n);
    c->stage = ST_REFIT; c->root_box_valid = true;
    { const int js = judge_sort_flags(c); if (js != CD_OK) return CD_OK; }                 // (not handled: the stream path redoes the step in the sort's next form)
    if (shards_overflowed(tb, h) || h.n_deferred > 0) {             // the tree is fine: the traversal again, with the stream path's retries / deep pass
        handled = true;
        c->left.scratch_clean = false;
        return run_traversal(c, tb, nullptr, 0, pairs, cap_pairs, n_pairs);
    }
    handled = true;
    const uint64_t found = h.n_pairs, ncopy = found < cap_pairs ? found : cap_pairs;
    if (pairs && ncopy > spec_n) {
        HIPCHK(hipMemcpyAsync(pairs + 2 * spec_n, tb.d_pairs + 2 * spec_n, sizeof(uint32_t) * 2 * (ncopy - spec_n), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    c->stats.ms_morton = c->stats.ms_sort = c->stats.ms_hierarchy = c->stats.ms_refit = c->stats.ms_traverse = c->stats.ms_descend = c->stats.ms_exact = 0.f;
    c->stats.ms_pipeline = c->stats.ms_build_block = 0.f;
    c->stats.traverse_launches = 0; c->stats.stack_overflows = 0;       // (0: this call launched no kernel of its own -- one graph launch)
    c->stats.n_pairs = found; c->stats.pairs_tested = h.pairs_tested; c->stats.node_visits = h.node_visits;
    c->stats.wave_steps = h.wave_steps; c->stats.candidates = h.candidates;
    c->stats.ms_descend_clock = (h.clk_end && h.clk_start_inv && c->wall_clock_khz > 0) ? (float)((double)(h.clk_end - ~h.clk_start_inv) / (double)c->wall_clock_khz) : 0.f;
    c->last_pairs_on_device = ncopy;
    if (n_pairs) *n_pairs = found;
    return found > cap_pairs ? CD_OVERFLOW : CD_OK;
}

}  // namespace

void multi_detach_from(cd_ctx *c);          // cd_multi.h

extern "C" {

const char *cd_version(void) { return "mi355cd 0.1 gfx950"; }

int cd_create(cd_ctx **out, const double *verts_xyz, uint32_t nv, const uint32_t *vidx3, const uint32_t *ids, uint32_t nt)
{
    if (!out || !verts_xyz || !vidx3 || nv == 0 || nt == 0) return CD_ERR_ARG;
    *out = nullptr;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    for (uint64_t k = 0; k < 3ull * nt; ++k) if (vidx3[k] >= nv) return CD_ERR_INDEX;
    bool all_ref = true;                                // is every vertex used by some triangle?  (then the box of the triangles is the box of the vertices: cd_multi.h)
    { std::vector<uint8_t> used(nv, 0);
      for (uint64_t k = 0; k < 3ull * nt; ++k) used[vidx3[k]] = 1;
      for (uint32_t v = 0; v < nv && all_ref; ++v) all_ref = used[v] != 0; }
    cd_ctx *c = new (std::nothrow) cd_ctx();
    if (!c) return CD_ERR_ARG;
    c->nv = nv; c->nt = nt;
    c->all_verts_referenced = all_ref;
    c->ntiles = cdiv(nt, SORT_TILE);
    { int dev = 0, khz = 0; if (hipGetDevice(&dev) == hipSuccess) { c->device = dev; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess) c->wall_clock_khz = khz; } (void)hipGetLastError(); }
    const size_t n = nt;
#define ALLOC(p, bytes) do { hipError_t e_ = hipMalloc((void **)&(p), (bytes)); if (e_ != hipSuccess) { free_all(c); delete c; return -(int)e_; } } while (0)
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return -(int)e; }
    for (int i = 0; i < EV_COUNT; ++i) { e = hipEventCreate(&c->ev[i]); if (e != hipSuccess) { free_all(c); delete c; return -(int)e; } }
    ALLOC(c->d_verts, sizeof(double) * 3 * (size_t)nv);
    ALLOC(c->d_vidx, sizeof(uint32_t) * 3 * n);
    if (ids) ALLOC(c->d_ids, sizeof(uint32_t) * n);
    for (int i = 0; i < 2; ++i) { ALLOC(c->d_keys[i], sizeof(uint64_t) * n); ALLOC(c->d_perm[i], sizeof(uint32_t) * n); }
    ALLOC(c->d_counts, sizeof(uint32_t) * RADIX * c->ntiles);
    ALLOC(c->d_chunk_tot, sizeof(uint32_t) * RADIX * cdiv(c->ntiles, (uint32_t)OS_CHUNK));
    ALLOC(c->d_cell, sizeof(uint32_t) * 2 * CELLS);
    { hipError_t e_ = hipMemset(c->d_cell, 0, sizeof(uint32_t) * 2 * CELLS); if (e_ != hipSuccess) { free_all(c); delete c; return -(int)e_; } }
    c->cell_clean = true;
    // one scratch block so that the fused pipeline zeroes everything with ONE memset, and as little as the sort form needs:
    //   [onesweep: histograms | tickets, flags | look-back granules of passes 6, 7] [small counters: 128 words] [TravState]   <- hybrid sort: this much
    //   [look-back granules of passes 0..5]                                                                                  <- the other forms: all of it
    const size_t gran = sizeof(unsigned long long) * (size_t)c->ntiles * RADIX;           // one pass
    const size_t look_off = sizeof(uint32_t) * HIST_COPIES * 8 * RADIX + 128;              // hist (HIST_COPIES partial tables) | 8 tickets, 8 time-out flags, fix-up flag, the cell statistic's two words (cd_sort.h cell_stat_turn), pad
    c->sort_hi_bytes = look_off + 2 * gran;
    const size_t small_off = (c->sort_hi_bytes + 127) & ~(size_t)127, state_off = small_off + 512;
    c->zero_bytes = state_off + sizeof(TravState);
    const size_t lo_off = (c->zero_bytes + 127) & ~(size_t)127;
    c->os_bytes = lo_off + 6 * gran;
    ALLOC(c->d_os, c->os_bytes);
    c->d_small = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(c->d_os) + small_off);
    c->tb[0].d_state = reinterpret_cast<TravState *>(reinterpret_cast<char *>(c->d_os) + state_off);
    c->d_root = reinterpret_cast<int32_t *>(c->d_small + 96);
    c->d_os_hist = reinterpret_cast<uint32_t *>(c->d_os);
    c->d_os_ticket = c->d_os_hist + HIST_COPIES * 8 * RADIX;
    c->d_os_look = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(c->d_os) + look_off);
    c->d_os_look_lo = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(c->d_os) + lo_off);
    ALLOC(c->d_frame, sizeof(double) * FRAME_WORDS);
    ALLOC(c->d_partial, sizeof(double) * BOUNDS_STRIDE * BOUNDS_BLOCKS);
    ALLOC(c->d_leaf, sizeof(LeafTri) * n);
    // a failed sort may leave slots unwritten for one (discarded) run: keep their vertex ids in range
    { hipError_t e_ = hipMemset(c->d_leaf, 0, sizeof(LeafTri) * n); if (e_ != hipSuccess) { free_all(c); delete c; return -(int)e_; } }
    ALLOC(c->d_meta, sizeof(NodeMeta) * n);
    ALLOC(c->d_parent, sizeof(int32_t) * 2 * n);
    { uint32_t nb = cdiv(nt, REFIT_BLK); c->nbp2 = 1; while (c->nbp2 < nb) c->nbp2 <<= 1; }
    if (c->nbp2 / (uint32_t)TOP_IN_BLOCK > (uint32_t)TOP_MAX_SPANS) { free_all(c); delete c; return CD_ERR_ARG; }   // k_top_publish_upper folds the span roots in LDS sized for 2^30 leaves (cd_build.h)
    ALLOC(c->d_seg, sizeof(double) * 6 * (size_t)c->nbp2 * REFIT_BLK);
    ALLOC(c->d_top_pub, top_pub_bytes(c));
    if (hipMemset(c->d_top_pub, 0, top_pub_bytes(c)) != hipSuccess) { free_all(c); delete c; return -(int)hipGetLastError(); }
    ALLOC(c->d_seg32, sizeof(float) * 6 * ((size_t)c->nbp2 << (REFIT_LOG - SEG32_MIN_LEVEL + 1)));   // fused build: levels SEG32_MIN_LEVEL .. 9 of the blocks' fp32 trees
    c->cross_cap = nt;                                  // every internal node could be one (it never is: about 2 %)
    ALLOC(c->d_cross, sizeof(int32_t) * (size_t)c->cross_cap);
    ALLOC(c->d_boxes, sizeof(double) * 6 * 2 * n);
    ALLOC(c->d_bounded, sizeof(uint32_t) * n);
    ALLOC(c->d_recs32, sizeof(NodeRec32) * n);
    ALLOC(c->d_qbox, sizeof(LeafBox32) * n);
    ALLOC(c->d_leaf_side, sizeof(unsigned long long) * ((n + 63) / 64 + 1));
    ALLOC(c->d_split_of, sizeof(int32_t) * n);
    { const size_t groups = ((size_t)n + 63) / 64;
      ALLOC(c->d_cost, sizeof(uint32_t) * groups); ALLOC(c->d_order, sizeof(uint32_t) * groups); ALLOC(c->d_tri_cost, n);
      if (hipMemset(c->d_cost, 0, sizeof(uint32_t) * groups) != hipSuccess || hipMemset(c->d_tri_cost, 0, n) != hipSuccess) { free_all(c); delete c; return CD_ERR_ARG; } }   // (no times yet: the first hint is half_vblock's own order)
    c->tb[0].cand_cap = ((4 * n > (1u << 20) ? 4 * n : (1u << 20)) + 4 * NSHARD - 1) / (4 * NSHARD) * (4 * NSHARD);    // (a shard: a multiple of 4 slots, cd_traverse.h: FatPair)
    ALLOC(c->tb[0].d_cand, sizeof(Candidates) * c->tb[0].cand_cap);
    c->tb[0].defer_cap = 1u << 16;
    ALLOC(c->tb[0].d_defer, sizeof(uint2) * c->tb[0].defer_cap);
#undef ALLOC
    // main.cu:86-88 H2D
    bool ok = hipMemcpy(c->d_verts, verts_xyz, sizeof(double) * 3 * (size_t)nv, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(c->d_vidx, vidx3, sizeof(uint32_t) * 3 * n, hipMemcpyHostToDevice) == hipSuccess &&
              (!ids || hipMemcpy(c->d_ids, ids, sizeof(uint32_t) * n, hipMemcpyHostToDevice) == hipSuccess) &&
              hipMemcpy(c->d_frame, c->frame_host, sizeof(double) * FRAME_WORDS, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { free_all(c); delete c; return -(int)hipGetLastError(); }
    { const int rc = amb_refresh(c); if (rc) { free_all(c); delete c; return rc; } }
    *out = c;
    return CD_OK;
}

void cd_destroy(cd_ctx *c)
{
    if (!c) return;
    multi_detach_from(c);                   // a cd_multi still attached keeps no pointer into a freed context (its next step returns CD_ERR_ORDER)
    hipStreamSynchronize(c->stream);
    free_all(c);
    delete c;
}

int cd_update_vertices(cd_ctx *c, const double *verts_xyz)
{
    if (!c || !verts_xyz) return CD_ERR_ARG;
    HIPCHK(hipStreamSynchronize(c->stream));                                // (nothing of an earlier call may still read the old vertices or the old cell table)
    HIPCHK(hipMemcpy(c->d_verts, verts_xyz, sizeof(double) * 3 * (size_t)c->nv, hipMemcpyHostToDevice));
    c->stage = ST_CREATED;
    c->root_box_valid = false;
    return amb_refresh(c);
}

static int install_frame(cd_ctx *c, int mode, const double off[3], const double span[3], unsigned long long layout)
{
    if (off) for (int a = 0; a < 3; ++a) { c->frame_host[a] = off[a]; c->frame_host[3 + a] = span[a]; }
    std::memcpy(&c->frame_host[6], &layout, sizeof layout); c->frame_host[7] = 0.0;
    c->frame_mode = mode;
    HIPCHK(hipStreamSynchronize(c->stream));                                // (nothing of an earlier call may still read the old frame)
    HIPCHK(hipMemcpy(c->d_frame, c->frame_host, sizeof(double) * FRAME_WORDS, hipMemcpyHostToDevice));
    c->stage = ST_CREATED;
    graph_drop(c);                                                          // (a captured step has k_morton's instance baked in: <true> for a layout word, <false> without)
    return CD_OK;
}
int cd_set_morton_frame(cd_ctx *c, int mode, const double offset[3], const double span[3])
{
    if (!c) return CD_ERR_ARG;
    if (mode == CD_FRAME_REFERENCE) {
        const double ref[6] = {0.004501, -0.476622, -0.381965, 3.08, 0.76, 2.36};
        return install_frame(c, mode, ref, ref + 3, 0ull);
    }
    if (mode == CD_FRAME_CUSTOM) {
        if (!offset || !span) return CD_ERR_ARG;
        return install_frame(c, mode, offset, span, 0ull);                  // morton.h:70-89's interleave in the caller's frame
    }
    if (mode != CD_FRAME_AUTO) return CD_ERR_ARG;
    return install_frame(c, mode, nullptr, nullptr, 0ull);                  // (the step computes the frame and writes it to d_frame)
}
// A frame WITH its key layout (cd_math.h), as cd_get_morton_frame returned it -- from this context after a step in CD_FRAME_AUTO (a frame computed
// once and kept: the AUTO pass over the triangles, ~11 us at 1 M, leaves the step), or from another one (all ranks of a job in one frame).
int cd_set_morton_frame_layout(cd_ctx *c, const double offset[3], const double span[3], uint64_t layout)
{
    if (!c || !offset || !span || !layout_ok(layout)) return CD_ERR_ARG;
    for (int a = 0; a < 3; ++a) if (!(span[a] > 0.0)) return CD_ERR_ARG;
    return install_frame(c, CD_FRAME_CUSTOM, offset, span, layout);
}
// The frame the last sort used: offset, span and key layout (0: the reference's interleave).
int cd_get_morton_frame(cd_ctx *c, double offset[3], double span[3], uint64_t *layout)
{
    if (!c) return CD_ERR_ARG;
    if (c->stage < ST_SORTED) return CD_ERR_ORDER;
    double f[FRAME_WORDS];
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(f, c->d_frame, sizeof f, hipMemcpyDeviceToHost));
    for (int a = 0; a < 3; ++a) { if (offset) offset[a] = f[a]; if (span) span[a] = f[3 + a]; }
    if (layout) std::memcpy(layout, &f[6], sizeof *layout);
    return CD_OK;
}

// the onesweep look-back spins are bounded; a timeout sets one of the words d_os_ticket[8..15]
constexpr int SORT_REDO = 77;                   // internal: this form of the sort could not finish, redo with the one the flags ask for
constexpr int SORT_REDO_MAX = 4;                // redos one call can need: small windows -> large windows -> half-key -> full is three (judge_sort_flags); one to spare
// The mean number of cell changes among 64 consecutive triangles (k_morton's statistic, cd_sort.h cell_count) up to which the global stage goes by cells, in sixteenths.
// Measured (profiles/r20_experiments/cell_sort.log): the 1 M / 4 M cloth lie at 5.7 / 3.4 and gain, a cloth of 250 k at 10.3 and one of 40 k at 22.9 lose (few keys a cell),
// a triangle soup lies at 64 and takes twice as long; at CELL_LOOP_CAP = 8 distinct cells a wave the kernels' loop no longer covers the wave.
constexpr uint32_t CELL_FORM_MAX_MEAN_16 = 8u * 16u;
static void choose_cell_form(cd_ctx *c, bool stat_known)
{
    const uint64_t waves = ((uint64_t)c->nt + 63u) / 64u;
    const bool coherent = stat_known && c->cell_stat != 0u && (uint64_t)c->cell_stat * 16u <= (uint64_t)CELL_FORM_MAX_MEAN_16 * waves;
    const bool next = c->dbg_sort_cells == 2 || (c->dbg_sort_cells == 0 && coherent);
    c->cell_form = next;
}
namespace { int judge_sort_flags(cd_ctx *c)
{
    for (int i = 0; i < 9; ++i) if (c->sort_flags[i]) { c->left.scratch_clean = false; c->cell_clean = false; }     // the flag words are cleared by the memset only
    for (int i = 0; i < 8; ++i) if (c->sort_flags[i]) return CD_ERR_SORT;
    const uint32_t f = c->sort_flags[8];
    // The form of the NEXT sort's global stage (cd_sort.h): by cells where this step's keys came in coherent order -- k_morton's statistic, which travels with the flags --,
    // classic after a raised flag (the redo, and a context's first step: nothing is known yet).  Either form gives the same keys and permutation.
    c->cell_stat = c->sort_flags[9];
    choose_cell_form(c, !f);
    if (!f) return CD_OK;
    // The flags say WHY (cd_sort.h): the next form is the one that can finish, not the next in line (round 5 walked 0 -> 1 -> 2 -> 3: a mesh with 17 coincident centroids
    // took four redos, one more than the multi-GPU step allowed itself).
    if (c->sort_mode >= 3) return CD_ERR_SORT;                              // (the full form raises nothing)
    if (f & SORTF_FIXUP) { c->sort_mode = 3; c->left_frame = false; return SORT_REDO; }      // too many equal high halves: only the eight passes do without a fix-up hop
    if (f & SORTF_RUN) {
        // a run too long for the small windows: the large form, same passes -- unless keys also lie above the digits (then another form is due anyway)
        if (!(f & SORTF_ABOVE) && c->local_small_active && c->local_small_ok && c->sort_mode <= 1) { c->local_small_ok = false; return SORT_REDO; }
        c->sort_mode = 2; c->left_frame = false; return SORT_REDO;          // no windows: four global passes + fix-up (digits at bits 48..63 only make runs longer)
    }
    // SORTF_ABOVE alone: some key lies beyond the shifted digits (a centroid outside the Morton frame), no run was too long.  A mesh that leaves the frame may come
    // back: a context that went 0 -> 1 for THAT reason tries the first form again every SORT_RETRY_STEPS steps (sort_retry_tick; a try that fails costs one redone step in 64).
    if (c->sort_mode == 0) { c->sort_mode = 1; c->left_frame = true; c->steps_in_mode1 = 0; return SORT_REDO; }
    c->sort_mode = 2; c->left_frame = false; return SORT_REDO;
} }
// Once per CALL of a stepping entry point (not per redo), BEFORE a graph step computes its key: a context whose mesh had left the Morton frame (sort form 1) tries
// the first form again every SORT_RETRY_STEPS steps.  (Round 5 counted inside enqueue_morton_sort, which a graph replay does not run: ADVICE r05.)
static void sort_retry_tick(cd_ctx *c)
{
    if (c->sort_mode == 1 && c->left_frame && ++c->steps_in_mode1 >= SORT_RETRY_STEPS) { c->sort_mode = 0; c->steps_in_mode1 = 0; c->local_small_ok = true; graph_drop(c); }   // (the second form's runs are 16 x longer: the small windows get their chance again too)
}
extern "C++" {                                  // (templates: the enqueued sequence is a parameter)
// The sort's redo policy, in ONE place.  `attempt` enqueues one try of whatever contains the sort and ends in a synchronise that has brought the sort's flag words to the host
// (c->sort_flags); negative is an error, anything else the attempt's own result, which the caller gets back once the flags are clean.  A raised flag: judge_sort_flags has
// changed the form, the attempt runs again.
template <class Attempt> static int with_sort_redo(cd_ctx *c, Attempt attempt)
{
    for (int redo = 0;; ++redo) {
        const int rc = attempt();
        if (rc < 0) return rc;
        const int js = judge_sort_flags(c);
        if (js != SORT_REDO) return js ? js : rc;
        if (redo == SORT_REDO_MAX) return CD_ERR_SORT;
    }
}
// The read-back a fused step ends in when nothing else brings them: the sort's flag words (d_os_ticket[8..16]) and the root box, then the synchronise.
static int sync_with_flags(cd_ctx *c)
{
    HIPCHK(hipMemcpyAsync(c->sort_flags, c->d_os_ticket + 8, sizeof c->sort_flags, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->root_box_host, c->d_boxes, sizeof(double) * 6, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CD_OK;
}
// One fused step: sort + tree with one memset for every counter of the pipeline (Prezeroed, closed before a redo is decided and opened again for it), then `tail`, which
// enqueues whatever rides behind the tree and ENDS IN A SYNCHRONISE THAT HAS BROUGHT THE SORT FLAGS AND THE ROOT BOX TO THE HOST (sync_with_flags, or a traversal's report).
// Returns the tail's result (it may be CD_OVERFLOW) once the tree stands; what follows a good step is the caller's.
template <class Tail> static int fused_step(cd_ctx *c, Tail tail)
{
    const int rc = with_sort_redo(c, [&]() -> int {
        Prezeroed fused(c);
        int re = enqueue_morton_sort(c, !fused_build_next(c));
        if (!re) re = enqueue_tree(c);
        return re ? re : tail();
    });
    if (rc >= 0) { c->root_box_valid = true; c->stage = ST_REFIT; }
    return rc;
}
}  // extern "C++"
// events -> the stage times of a step's build (only with stage timing on are all of them recorded)
static void read_build_times(cd_ctx *c)
{
    c->stats.ms_morton = elapsed(c, EV_MORTON0, EV_MORTON1);
    c->stats.ms_sort = elapsed(c, EV_MORTON1, EV_SORT1);
    c->stats.ms_hierarchy = c->left.last_tree_fused ? 0.f : elapsed(c, EV_HIER0, EV_HIER1);
    c->stats.ms_refit = elapsed(c, EV_REFIT0, EV_REFIT1);
}

int cd_morton_sort(cd_ctx *c)
{
    if (!c) return CD_ERR_ARG;
    sort_retry_tick(c);
    const int rc = with_sort_redo(c, [c]() -> int {                            // (no tree: the flag words alone)
        const int re = enqueue_morton_sort(c);
        if (re) return re;
        HIPCHK(hipMemcpyAsync(c->sort_flags, c->d_os_ticket + 8, sizeof c->sort_flags, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return CD_OK;
    });
    if (rc) return rc;
    c->stats.ms_morton = elapsed(c, EV_MORTON0, EV_MORTON1);
    c->stats.ms_sort = elapsed(c, EV_MORTON1, EV_SORT1);
    c->stage = ST_SORTED;
    return CD_OK;
}

int cd_build_hierarchy(cd_ctx *c, uint32_t *parent_wrong_num)
{
    if (!c) return CD_ERR_ARG;
    if (c->stage < ST_SORTED) return CD_ERR_ORDER;
    int rc = enqueue_hierarchy(c, true);
    if (rc) return rc;
    uint32_t wrong = 0;
    HIPCHK(hipMemcpyAsync(&wrong, c->d_small, sizeof wrong, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stats.ms_hierarchy = elapsed(c, EV_HIER0, EV_HIER1);
    if (parent_wrong_num) *parent_wrong_num = wrong;
    c->stage = ST_BUILT;
    return CD_OK;
}

int cd_refit_boxes(cd_ctx *c)
{
    if (!c) return CD_ERR_ARG;
    c->root_box_valid = false;
    if (c->stage < ST_BUILT) return CD_ERR_ORDER;
    int rc = enqueue_refit(c, true);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stats.ms_refit = elapsed(c, EV_REFIT0, EV_REFIT1);
    c->stage = ST_REFIT;
    return CD_OK;
}

// Fused calls do not write the FP64 boxes of the internal nodes (nothing on their path reads them); whoever asks for
// them afterwards -- the exported tree, checkInternalNodes' uninitialised-box counter -- gets them from a full refit.
static int materialise_internal_boxes(cd_ctx *c)
{
    if (c->stage < ST_REFIT || (c->left.internal_boxes_valid && c->left.hierarchy_valid)) return CD_OK;
    int rc = CD_OK;
    if (!c->left.hierarchy_valid) rc = enqueue_hierarchy(c, false);             // k_fill_leaves (parent links reset) + k_hierarchy on the current keys
    if (!rc) rc = enqueue_refit(c, true, false);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return CD_OK;
}

static int run_check(cd_ctx *c, int which, uint32_t maxv, uint32_t *out, int nout)
{
    if (!c || !out) return CD_ERR_ARG;
    if (c->stage < ST_BUILT) return CD_ERR_ORDER;
    if (which != 2) { const int rm = materialise_internal_boxes(c); if (rm) return rm; }    // meta / parent / boxes of the reference-shaped tree
    const int n = (int)c->nt;
    hipStream_t s = c->stream;
    HIPCHK(hipEventRecord(c->ev[EV_CHK0], s));
    HIPCHK(hipMemsetAsync(c->d_small + 8, 0, 8 * sizeof(uint32_t), s));           // main.cu:113,121,129
    if (which == 0) { if (n > 1) k_check_internal<<<cdiv(n - 1, 256), 256, 0, s>>>(n, c->d_meta, c->d_parent, c->d_bounded, c->d_boxes, c->d_small + 8); }
    else if (which == 1) k_check_leaves<<<cdiv(n, 256), 256, 0, s>>>(n, c->d_parent, c->d_leaf, maxv, c->d_boxes, c->d_small + 8);
    else k_check_triangle_idx<<<cdiv(n, 256), 256, 0, s>>>(n, c->d_leaf, maxv, c->d_small + 8);
    HIPCHK(hipEventRecord(c->ev[EV_CHK1], s));
    HIPCHK(hipMemcpyAsync(out, c->d_small + 8, nout * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    c->stats.ms_check = elapsed(c, EV_CHK0, EV_CHK1);
    return CD_OK;
}
int cd_check_internal(cd_ctx *c, uint32_t out[5]) { return run_check(c, 0, 0, out, 5); }
int cd_check_leaves(cd_ctx *c, uint32_t out[4]) { return run_check(c, 1, c ? c->nv : 0, out, 4); }
int cd_check_triangle_idx(cd_ctx *c, uint32_t maxv, uint32_t *out) { return run_check(c, 2, maxv, out, 1); }

int cd_find_collisions(cd_ctx *c, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs)
{
    if (!c || (cap_pairs && !pairs)) return CD_ERR_ARG;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    return run_traversal(c, c->tb[0], nullptr, 0, pairs, cap_pairs, n_pairs);
}

int cd_build_tree(cd_ctx *c)
{
    if (!c) return CD_ERR_ARG;
    sort_retry_tick(c);
    const int rc = fused_step(c, [c] { return sync_with_flags(c); });
    if (rc) return rc;
    if (c->stage_events) read_build_times(c);
    return CD_OK;
}

int cd_self_collide(cd_ctx *c, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs)
{
    if (!c || (cap_pairs && !pairs)) return CD_ERR_ARG;
    sort_retry_tick(c);                                                    // (before a graph step computes its key)
    // CD_OPT_GRAPH: the steady-state step as one graph launch.  (Tried once, not per redo: a redo follows a raised sort flag, for which judge_sort_flags clears scratch_clean,
    //  and without scratch_clean no step is eligible.)
    if (graph_eligible(c)) {
        bool handled = false;
        const int rg = graph_step(c, pairs, cap_pairs, n_pairs, handled);
        if (rg < 0 || handled) return rg;
    }
    const int rc = fused_step(c, [&] { return run_traversal(c, c->tb[0], nullptr, 0, pairs, cap_pairs, n_pairs); });     // (its report carries the flags and the root box)
    if (rc < 0) return rc;
    if (c->stage_events) read_build_times(c);
    else c->stats.ms_morton = c->stats.ms_sort = c->stats.ms_hierarchy = c->stats.ms_refit = 0.f;
    const bool all_stamps = c->stage_events || (c->stamp_mask & 14u) == 14u;
    c->stats.ms_pipeline = all_stamps ? elapsed(c, EV_MORTON0, EV_TRAV1) + (c->stats.ms_traverse - elapsed(c, EV_TRAV0, EV_TRAV1)) : 0.f;   // + deep pass, if any
    c->stats.ms_build_block = (c->left.last_tree_fused && (c->stamp_mask & 1u)) ? elapsed(c, EV_BLK0, EV_BLK1) : 0.f;
    return rc;
}

int cd_brute_force(cd_ctx *c, int box_filter, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs)
{
    if (!c || (cap_pairs && !pairs)) return CD_ERR_ARG;
    int rc = ensure_pairs(c, c->tb[0], cap_pairs > 0 ? cap_pairs : 1);
    if (rc) return rc;
    hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(c->tb[0].d_state, 0, sizeof(TravState), s));
    k_brute_force<<<cdiv(c->nt, 256), 256, 0, s>>>(c->d_verts, c->d_vidx, c->d_ids, c->nt, box_filter, c->tb[0].d_pairs, cap_pairs, c->tb[0].d_state);
    HostCounters h;
    { int r = read_state(c, c->tb[0], h); if (r) return r; }
    HIPCHK(hipGetLastError());
    const uint64_t ncopy = h.n_pairs < cap_pairs ? h.n_pairs : cap_pairs;
    if (pairs && ncopy) HIPCHK(hipMemcpy(pairs, c->tb[0].d_pairs, sizeof(uint32_t) * 2 * ncopy, hipMemcpyDeviceToHost));
    // the device list now holds THIS call's pairs: cd_sorted_pairs / cd_collision_triangles refer to it
    c->stats.n_pairs = h.n_pairs; c->stats.pairs_tested = h.pairs_tested;
    c->last_pairs_on_device = ncopy;
    if (n_pairs) *n_pairs = h.n_pairs;
    return h.n_pairs > cap_pairs ? CD_OVERFLOW : CD_OK;
}

int cd_test_pairs(cd_ctx *c, const uint32_t *pairs, uint64_t np, uint8_t *out)
{
    if (!c || !pairs || !out) return CD_ERR_ARG;
    if (np == 0) return CD_OK;
    for (uint64_t k = 0; k < 2 * np; ++k) if (pairs[k] >= c->nt) return CD_ERR_INDEX;
    uint32_t *d_p = nullptr; uint8_t *d_o = nullptr;
    HIPCHK(hipMalloc(&d_p, sizeof(uint32_t) * 2 * np));
    if (hipMalloc(&d_o, np) != hipSuccess) { hipFree(d_p); return -(int)hipErrorOutOfMemory; }
    int rc = CD_OK;
    if (hipMemcpy(d_p, pairs, sizeof(uint32_t) * 2 * np, hipMemcpyHostToDevice) != hipSuccess) rc = -(int)hipErrorInvalidValue;
    if (!rc) {
        k_test_pairs<<<cdiv(np, 256), 256, 0, c->stream>>>(c->d_verts, c->d_vidx, c->d_ids, d_p, np, d_o);
        if (hipStreamSynchronize(c->stream) != hipSuccess || hipMemcpy(out, d_o, np, hipMemcpyDeviceToHost) != hipSuccess) rc = -(int)hipGetLastError();
    }
    hipFree(d_p); hipFree(d_o);
    return rc;
}

int cd_sorted_pairs(cd_ctx *c, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs)
{
    if (!c || !n_pairs || (cap_pairs && !pairs)) return CD_ERR_ARG;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (c->stats.n_pairs > c->last_pairs_on_device) return CD_OVERFLOW;     // the last traversal's list was truncated: rerun it with a larger cap
    const uint32_t m = (uint32_t)c->last_pairs_on_device;
    *n_pairs = m;
    if (m == 0) return CD_OK;
    int rc = pp_reserve(c, m);
    if (rc) return rc;
    hipStream_t s = c->stream;
    k_pairs_to_keys<<<cdiv(m, 256), 256, 0, s>>>(c->tb[0].d_pairs, m, c->pp_keys[0]);
    if ((rc = pp_sort(c, m))) return rc;
    k_keys_to_pairs<<<cdiv(m, 256), 256, 0, s>>>(c->pp_keys[0], m, reinterpret_cast<uint32_t *>(c->pp_keys[1]));
    const uint64_t ncopy = m < cap_pairs ? m : cap_pairs;
    if (ncopy) HIPCHK(hipMemcpyAsync(pairs, c->pp_keys[1], sizeof(uint32_t) * 2 * ncopy, hipMemcpyDeviceToHost, s));
    uint32_t f[8];
    HIPCHK(hipMemcpyAsync(f, reinterpret_cast<uint32_t *>(c->pp_os) + 8 * RADIX + 8, sizeof f, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    for (int i = 0; i < 8; ++i) if (f[i]) return CD_ERR_SORT;
    return m > cap_pairs ? CD_OVERFLOW : CD_OK;
}

int cd_collision_triangles(cd_ctx *c, uint32_t *ids, uint64_t cap, uint64_t *n)
{
    if (!c || !n || (cap && !ids)) return CD_ERR_ARG;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (c->stats.n_pairs > c->last_pairs_on_device) return CD_OVERFLOW;
    const uint64_t m2_64 = 2 * c->last_pairs_on_device;
    *n = 0;
    if (m2_64 == 0) return CD_OK;
    if (m2_64 > 0xfffffff0ull) return CD_ERR_ARG;
    const uint32_t m2 = (uint32_t)m2_64;
    int rc = pp_reserve(c, m2);
    if (rc) return rc;
    hipStream_t s = c->stream;
    k_ids_to_keys<<<cdiv(m2, 256), 256, 0, s>>>(c->tb[0].d_pairs, m2, c->pp_keys[0]);
    if ((rc = pp_sort(c, m2))) return rc;
    k_unique_flags<<<cdiv(m2, 256), 256, 0, s>>>(c->pp_keys[0], m2, c->pp_flags);
    k_scan_exclusive<<<1, 1024, 0, s>>>(c->pp_flags, m2);
    uint32_t *out = c->pp_vals[0], *d_count = reinterpret_cast<uint32_t *>(c->pp_os) + 8 * RADIX;   // ticket word 0 is free after the sort
    k_unique_scatter<<<cdiv(m2, 256), 256, 0, s>>>(c->pp_keys[0], c->pp_flags, m2, out, c->pp_cap, d_count);
    uint32_t cnt = 0, f[8];
    HIPCHK(hipMemcpyAsync(&cnt, d_count, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(f, reinterpret_cast<uint32_t *>(c->pp_os) + 8 * RADIX + 8, sizeof f, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    for (int i = 0; i < 8; ++i) if (f[i]) return CD_ERR_SORT;
    *n = cnt;
    const uint64_t ncopy = cnt < cap ? cnt : cap;
    if (ncopy) HIPCHK(hipMemcpy(ids, out, sizeof(uint32_t) * ncopy, hipMemcpyDeviceToHost));
    return cnt > cap ? CD_OVERFLOW : CD_OK;
}

int cd_export_keys(cd_ctx *c, uint64_t *keys, uint32_t *perm)
{
    if (!c) return CD_ERR_ARG;
    if (c->stage < ST_SORTED) return CD_ERR_ORDER;
    if (keys) HIPCHK(hipMemcpy(keys, c->d_keys[0], sizeof(uint64_t) * c->nt, hipMemcpyDeviceToHost));
    if (perm) HIPCHK(hipMemcpy(perm, c->d_perm[0], sizeof(uint32_t) * c->nt, hipMemcpyDeviceToHost));
    return CD_OK;
}

int cd_export_tree(cd_ctx *c, int32_t *parent, int32_t *left, int32_t *right, double *boxes, uint32_t *bounded)
{
    if (!c) return CD_ERR_ARG;
    if (c->stage < ST_BUILT) return CD_ERR_ORDER;
    const size_t n = c->nt;
    { const int rm = materialise_internal_boxes(c); if (rm) return rm; }      // after a fused call: the reference-shaped tree is built on request
    if (parent) HIPCHK(hipMemcpy(parent, c->d_parent, sizeof(int32_t) * (2 * n - 1), hipMemcpyDeviceToHost));
    if ((left || right) && n > 1) {
        std::vector<int4> m(n - 1);
        HIPCHK(hipMemcpy(m.data(), c->d_meta, sizeof(int4) * (n - 1), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n - 1; ++i) { if (left) left[i] = m[i].x; if (right) right[i] = m[i].y; }
    }
    if (boxes || bounded) { if (c->stage < ST_REFIT) return CD_ERR_ORDER; }

    if (boxes) HIPCHK(hipMemcpy(boxes, c->d_boxes, sizeof(double) * 6 * (2 * n - 1), hipMemcpyDeviceToHost));
    if (bounded && n > 1) HIPCHK(hipMemcpy(bounded, c->d_bounded, sizeof(uint32_t) * (n - 1), hipMemcpyDeviceToHost));
    return CD_OK;
}

/* Debug only (not in the public header): sums of the 12 spare words of the 64 counter shards of the last traversal. */
int cd_debug_counters(cd_ctx *c, unsigned long long out[12])
{
    if (!c || !out) return CD_ERR_ARG;
    std::vector<TravState> h(1);
    HIPCHK(hipMemcpy(h.data(), c->tb[0].d_state, sizeof(TravState), hipMemcpyDeviceToHost));
    for (int k = 0; k < 12; ++k) { out[k] = 0; for (int i = 0; i < NSHARD; ++i) out[k] += h[0].shard[i].pad[k]; }
    return CD_OK;
}

/* Debug only: the order hint's arrays -- per group of 64 leaves (ceil(nt / 64) words each) the score of the last fused build and the order made from the scores; per triangle (nt bytes) the time class its wave left in the last half traversal. */
int cd_debug_hint(cd_ctx *c, uint32_t *cost, uint32_t *order, uint8_t *tri)
{
    if (!c) return CD_ERR_ARG;
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t groups = ((size_t)c->nt + 63) / 64;
    if (tri) HIPCHK(hipMemcpy(tri, c->d_tri_cost, c->nt, hipMemcpyDeviceToHost));
    if (cost) HIPCHK(hipMemcpy(cost, c->d_cost, sizeof(uint32_t) * groups, hipMemcpyDeviceToHost));
    if (order) { if (!c->order_ready) return CD_ERR_ORDER; HIPCHK(hipMemcpy(order, c->d_order, sizeof(uint32_t) * groups, hipMemcpyDeviceToHost)); }
    return CD_OK;
}

/* Debug only: install an order for the next half traversal (must be a permutation of the groups; checked). */
int cd_debug_hint_set(cd_ctx *c, const uint32_t *order)
{
    if (!c || !order) return CD_ERR_ARG;
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint32_t groups = (c->nt + 63u) / 64u;
    std::vector<uint8_t> seen(groups, 0);
    for (uint32_t b = 0; b < groups; ++b) { if (order[b] >= groups || seen[order[b]]) return CD_ERR_ARG; seen[order[b]] = 1; }
    HIPCHK(hipMemcpy(c->d_order, order, sizeof(uint32_t) * groups, hipMemcpyHostToDevice));
    c->order_ready = true;
    return CD_OK;
}

int cd_debug_records(cd_ctx *c, void *recs, void *qboxes, int32_t *root)
{
    if (!c) return CD_ERR_ARG;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (recs) HIPCHK(hipMemcpy(recs, c->d_recs32, sizeof(NodeRec32) * (size_t)c->nt, hipMemcpyDeviceToHost));
    if (qboxes) { const int rq = ensure_qbox(c); if (rq) return rq; HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipMemcpy(qboxes, c->d_qbox, sizeof(LeafBox32) * (size_t)c->nt, hipMemcpyDeviceToHost)); }
    if (root) HIPCHK(hipMemcpy(root, c->d_root, sizeof(int32_t), hipMemcpyDeviceToHost));
    return CD_OK;
}

/* Debug only: the swept tree of the last CCD pass (cd_ccd.h) as its descent read it.  between = 0: this context's own (cd_find_ccd / cd_self_ccd);
 * 1: the other mesh's, as this context holds it for cd_find_ccd_between.  Records, up[] and M are copies; the pad is recomputed here
 * (the descent keeps it in registers).  Nothing is launched. */
int cd_debug_swept(cd_ctx *c, int between, void *recs, int32_t *up, uint32_t *m_bits, float *pad, uint32_t *n_leaves)
{
    if (!c || (between != 0 && between != 1)) return CD_ERR_ARG;
    const SweptBuf &sw = c->swept[between];
    const SweptBuf::Seen &seen = sw.seen;
    if (!seen.ran) return CD_ERR_ORDER;
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t n = seen.n;
    if (n >= 2) {                                                            // (one leaf: no records, no links)
        if (recs) HIPCHK(hipMemcpy(recs, sw.d_recs, sizeof(NodeRec32) * n, hipMemcpyDeviceToHost));
        if (up) HIPCHK(hipMemcpy(up, sw.d_up, sizeof(int32_t) * (2 * n - 1), hipMemcpyDeviceToHost));
    }
    if (m_bits) *m_bits = seen.m_bits;
    if (pad) {                                                               // ccd_pad's host twin: the same FP64 sum, rounded up to fp32
        float m; std::memcpy(&m, &seen.m_bits, sizeof m);
        const double v = 2.0 * seen.dist + 2.0 * seen.dist * PROX_SLACK + (double)m * PROX_SLACK;
        float f = INFINITY;
        if (v <= (double)FLT_MAX) { f = (float)v; if ((double)f < v) f = std::nextafterf(f, INFINITY); }
        *pad = f;
    }
    if (n_leaves) *n_leaves = seen.n;
    return CD_OK;
}

// morton3D / expand64Bits themselves, on caller-supplied inputs; no context (one-shot device buffers on the null stream)
static int morton_batch(const void *in, size_t in_bytes, uint64_t n, const double frame[FRAME_WORDS], uint64_t *out)
{
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const char *d_in = dev.in(static_cast<const char *>(in), in_bytes);
    uint64_t *d_out = dev.out<uint64_t>(n);
    const double *d_frame = frame ? dev.in(frame, FRAME_WORDS) : nullptr;
    if (dev.e == hipSuccess) {
        if (frame) k_morton_points<<<strided_grid(n, 256), 256>>>(reinterpret_cast<const double *>(d_in), n, d_frame, d_out);
        else k_expand_values<<<strided_grid(n, 256), 256>>>(reinterpret_cast<const uint64_t *>(d_in), n, d_out);
        dev.e = hipGetLastError();
    }
    dev.back(out, d_out, n);
    return dev.rc();
}
int cd_morton3d_points(const double *xyz, uint64_t n, const double offset[3], const double span[3], uint64_t *keys)
{
    if (!xyz || !keys || (!offset) != (!span)) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    double frame[FRAME_WORDS] = {0.004501, -0.476622, -0.381965, 3.08, 0.76, 2.36, 0.0, 0.0};           // morton.h:45,51,57
    if (offset) for (int a = 0; a < 3; ++a) { frame[a] = offset[a]; frame[3 + a] = span[a]; }
    return morton_batch(xyz, sizeof(double) * 3 * n, n, frame, keys);
}
// the same in a frame with a key layout (cd_math.h morton3d_layout: what k_morton computes in such a frame -- xyz is then the SUM of a triangle's three vertices
// per axis, not the centroid: cd_math.h, KeyLayout); layout 0 = cd_morton3d_points
int cd_morton3d_points_layout(const double *xyz, uint64_t n, const double offset[3], const double span[3], uint64_t layout, uint64_t *keys)
{
    if (!xyz || !keys || !offset || !span || !layout_ok(layout)) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    double frame[FRAME_WORDS] = {offset[0], offset[1], offset[2], span[0], span[1], span[2], 0.0, 0.0};
    std::memcpy(&frame[6], &layout, sizeof layout);
    return morton_batch(xyz, sizeof(double) * 3 * n, n, frame, keys);
}
int cd_expand64_values(const uint64_t *v, uint64_t n, uint64_t *out)
{
    if (!v || !out) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    return morton_batch(v, sizeof(uint64_t) * n, n, nullptr, out);
}

// checkBoxOverlap / Box::merge / checkTriangleContact themselves on caller-supplied operands; no context (one-shot buffers, null stream)
int cd_box_pairs(const double *a, const double *b, uint64_t n, uint8_t *overlap, double *merged)
{
    if (!a || !b || (!overlap && !merged)) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_a = dev.in(a, 6 * n), *d_b = dev.in(b, 6 * n);
    uint8_t *d_o = overlap ? dev.out<uint8_t>(n) : nullptr;
    double *d_m = merged ? dev.out<double>(6 * n) : nullptr;
    if (dev.e == hipSuccess) {
        k_box_pairs<<<strided_grid(n, 256), 256>>>(d_a, d_b, n, d_o, d_m);
        dev.e = hipGetLastError();
    }
    dev.back(overlap, d_o, n);
    dev.back(merged, d_m, 6 * n);
    return dev.rc();
}
int cd_tri_contact_points(const double *tri, uint64_t n, uint8_t *out)
{
    if (!tri || !out) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_t = dev.in(tri, 18 * n);
    uint8_t *d_o = dev.out<uint8_t>(n);
    if (dev.e == hipSuccess) {
        k_tri_contact_points<<<strided_grid(n, 256), 256>>>(d_t, n, d_o);
        dev.e = hipGetLastError();
    }
    dev.back(out, d_o, n);
    return dev.rc();
}

int cd_alloc_host_pairs(uint64_t cap_pairs, uint32_t **pairs)
{
    if (!pairs || cap_pairs == 0) return CD_ERR_ARG;
    *pairs = nullptr;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    void *p = nullptr;
    // (coherent = fine-grained: the memory the HSA memory model defines system-scope release / acquire between device and host on)
    HIPCHK(hipHostMalloc(&p, sizeof(uint32_t) * 2 * cap_pairs + 16, hipHostMallocCoherent));     // +16: the report kernel moves pairs as 16-byte quads
    PinnedPairs &pp = pinned_pairs();
    { std::lock_guard<std::mutex> lock(pp.mu); pp.v.push_back(PinnedPairs::Buf{static_cast<const uint32_t *>(p), cap_pairs, pp.next_id++}); }
    *pairs = static_cast<uint32_t *>(p);
    return CD_OK;
}
void cd_free_host_pairs(uint32_t *pairs)
{
    if (!pairs) return;
    PinnedPairs &pp = pinned_pairs();
    { std::lock_guard<std::mutex> lock(pp.mu);
      for (size_t i = 0; i < pp.v.size(); ++i) if (pp.v[i].p == pairs) { pp.v.erase(pp.v.begin() + (long)i); break; } }
    hipHostFree(pairs);
}


int cd_get_stats(cd_ctx *c, cd_stats *out) { if (!c || !out) return CD_ERR_ARG; *out = c->stats; return CD_OK; }
int cd_num_triangles(cd_ctx *c, uint32_t *nt) { if (!c || !nt) return CD_ERR_ARG; *nt = c->nt; return CD_OK; }

int cd_set_option(cd_ctx *c, int key, int64_t value)
{
    if (!c) return CD_ERR_ARG;
    if (key == CD_OPT_TRAVERSAL) { if (value != 0 && value != 1 && value != 3) return CD_ERR_ARG; c->trav_variant = (int)value; return CD_OK; }
    if (key == CD_OPT_QUERIES_PER_WAVE) { if (value < 64 || value > (1 << 20) || value % 64) return CD_ERR_ARG; c->queries_per_wave = (uint32_t)value; return CD_OK; }
    if (key == CD_OPT_SORT_FULL) { if (value < 0 || value > 2) return CD_ERR_ARG; c->sort_mode = value == 0 ? 0 : (value == 1 ? 3 : 2); c->left_frame = false; return CD_OK; }
    if (key == CD_OPT_STAGE_TIMING) { c->stage_events = value != 0; return CD_OK; }
    if (key == CD_OPT_GRAPH) { c->graph_opt = value != 0; if (!c->graph_opt) graph_drop(c); return CD_OK; }
    if (key == CD_OPT_POLL) { c->poll_opt = value != 0; return CD_OK; }
    if (key == CD_OPT_CELL_TABLE) {
        if (c->cell_table_opt == (value != 0)) return CD_OK;
        c->cell_table_opt = value != 0;
        HIPCHK(hipStreamSynchronize(c->stream));
        c->stage = ST_CREATED; c->root_box_valid = false;                  // the records of the tree that is there were encoded the other way
        return amb_refresh(c);
    }
    if (key == CD_OPT_ORDER_HINT) { c->order_hint = value != 0; c->order_hint_large = value == 2; c->order_ready = false; c->order_pending = false; graph_drop(c); return CD_OK; }       // (a captured step has its launches baked in)
    if (key == CD_OPT_KERNEL_STAMPS) { if (value < 0 || value > 15) return CD_ERR_ARG; c->stamp_mask = (uint32_t)value; return CD_OK; }
    return CD_ERR_ARG;
}

// Measurement hooks and test switches: their own entry point and their own key space, so that no hook can shadow an option
// (round 3: the polling scan's keys were once numbered like the keys the record tests use to ask for the stage-wise build).
// Setters return CD_OK; getters write *out (required) and ignore `value`.
int cd_debug_option(cd_ctx *c, int key, int64_t value, int64_t *out)
{
    if (!c) return CD_ERR_ARG;
    switch (key) {
    case CD_DBG_LDS_PAD:         c->dbg_lds_pad = (uint32_t)value; return CD_OK;
    case CD_DBG_EXACT_BLOCKS:    if (value < 1 || value > 65535) return CD_ERR_ARG; c->exact_blocks = (int)((value + NSHARD - 1) / NSHARD * NSHARD); return CD_OK;   // (a workgroup owns a shard: whole multiples of 64)
    case CD_DBG_NO_SHARED_PATH:  c->dbg_no_shared_path = value != 0; return CD_OK;
    case CD_DBG_DIAG:            c->dbg_diag = value != 0; return CD_OK;
    case CD_DBG_STAGEWISE_BUILD: c->dbg_no_fused_build = value != 0; return CD_OK;
    case CD_DBG_SPLIT_CROSS:     c->dbg_split_cross = value != 0; return CD_OK;
    case CD_DBG_SORT_WINDOWS:    if (value < 0 || value > 2) return CD_ERR_ARG; c->dbg_sort_windows = (uint32_t)value; c->local_small_ok = true; graph_drop(c); return CD_OK;
    case CD_DBG_REPORT_COPIES:   c->dbg_report_copies = value != 0; graph_drop(c); return CD_OK;
    case CD_DBG_STORE_QBOX:      c->dbg_store_qbox = value != 0; graph_drop(c); return CD_OK;
    case CD_DBG_BIG_OFFSETS:     c->dbg_big_offsets = value != 0; graph_drop(c); return CD_OK;
    case CD_DBG_POLL_SCAN:       c->dbg_poll_check = value != 0; return CD_OK;
    case CD_DBG_GET_POLL_STALE:     if (!out) return CD_ERR_ARG; *out = c->poll_stale; return CD_OK;
    case CD_DBG_GET_POLL_FALLBACKS: if (!out) return CD_ERR_ARG; *out = c->poll_fallbacks; return CD_OK;
    case CD_DBG_GET_POLLED_STEPS:   if (!out) return CD_ERR_ARG; *out = c->polled_steps; return CD_OK;
    case CD_DBG_GET_POLL_FB_WHY:    if (!out) return CD_ERR_ARG; *out = (int64_t)c->poll_fb_busy | ((int64_t)c->poll_fb_late_word << 16) | ((int64_t)c->poll_fb_lost << 32); return CD_OK;
    case CD_DBG_GET_POLL_MAX_WAIT_US: if (!out) return CD_ERR_ARG; *out = c->poll_max_wait_us; return CD_OK;
    case CD_DBG_GET_GRAPH_CAPTURES: if (!out) return CD_ERR_ARG; *out = (int64_t)c->graph_captures; return CD_OK;
    case CD_DBG_GET_GRAPH_REPLAYS:  if (!out) return CD_ERR_ARG; *out = (int64_t)c->graph_replays; return CD_OK;
    case CD_DBG_GET_TREE_WAS_FUSED: if (!out) return CD_ERR_ARG; *out = c->left.last_tree_fused ? 1 : 0; return CD_OK;
    case CD_DBG_GET_SORT_FORM:   if (out) *out = c->sort_mode; return CD_OK;
    case CD_DBG_SORT_CELLS:      if (value < 0 || value > 2) return CD_ERR_ARG; if ((uint32_t)value != c->dbg_sort_cells) { c->dbg_sort_cells = (uint32_t)value; c->cell_form = value == 2; } return CD_OK;   // (a change to 0: classic until a judged step says otherwise; the form is in the graph's key)
    case CD_DBG_GET_SORT_CELLS:  if (!out) return CD_ERR_ARG; *out = c->cell_form_used ? 1 : 0; return CD_OK;
    case CD_DBG_GET_CELL_STAT:   if (!out) return CD_ERR_ARG; *out = c->cell_stat; return CD_OK;
    case CD_DBG_GET_ORDER_STATE: {          // the order hint as it stands: 0 none built, 1 a permutation of the groups that differs from the plain order, 2 the plain order itself, -1 NOT a permutation (a bug)
        if (!out) return CD_ERR_ARG;
        *out = 0;
        if (!c->order_ready) return CD_OK;
        HIPCHK(hipStreamSynchronize(c->stream));
        const uint32_t groups = (c->nt + 63u) / 64u;
        std::vector<uint32_t> o(groups), plain(groups);
        HIPCHK(hipMemcpy(o.data(), c->d_order, sizeof(uint32_t) * groups, hipMemcpyDeviceToHost));
        std::vector<uint8_t> seen(groups, 0);
        bool perm = true, same = true;
        for (uint32_t b = 0; b < groups; ++b) {
            if (o[b] >= groups || seen[o[b]]) { perm = false; break; }
            seen[o[b]] = 1;
            same = same && o[b] == half_vblock_host(b, groups);
        }
        *out = !perm ? -1 : (same ? 2 : 1);
        return CD_OK;
    }
    default: return CD_ERR_ARG;
    }
}

int cd_set_vertex_id_base(cd_ctx *c, uint32_t base) { if (!c) return CD_ERR_ARG; c->vbase = base; return CD_OK; }

int cd_root_box(cd_ctx *c, double box[6])
{
    if (!c || !box) return CD_ERR_ARG;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (c->root_box_valid) { memcpy(box, c->root_box_host, sizeof(double) * 6); return CD_OK; }   // came back with an earlier read-back
    // n == 1: the only node is leaf 0 = node 0 as well
    HIPCHK(hipMemcpy(box, c->d_boxes, sizeof(double) * 6, hipMemcpyDeviceToHost));
    return CD_OK;
}

int cd_pack_queries(cd_ctx *c, const double box[6], void *d_out, uint64_t cap, uint64_t *n)
{
    if (!c || !box || !n || (cap && !d_out)) return CD_ERR_ARG;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    hipStream_t s = c->stream;
    // the box and the counter live in the context's small scratch words (d_small[104..117]), not in the traversal state:
    // packing does not disturb the statistics of the traversal before it
    double *d_box = reinterpret_cast<double *>(c->d_small + 104);
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(c->d_small + 116);
    { const int rq = ensure_qbox(c); if (rq) return rq; }
    HIPCHK(hipMemcpyAsync(d_box, box, sizeof(double) * 6, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), s));
    k_pack_queries<<<cdiv(c->nt, PACK_THREADS), PACK_THREADS, 0, s>>>(c->d_verts, c->d_leaf, c->d_boxes, c->d_qbox, (int)c->nt, d_box, 1, -1, nullptr,
                                                                       reinterpret_cast<ExtQuery *>(d_out), cap, d_cnt, c->vbase);
    unsigned long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, d_cnt, sizeof h, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    *n = h;
    return h > cap ? CD_OVERFLOW : CD_OK;
}

int cd_find_collisions_queries(cd_ctx *c, const void *d_queries, uint64_t nq, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs)
{
    if (!c || (cap_pairs && !pairs) || (nq && !d_queries) || nq > 0xffffffffull) return CD_ERR_ARG;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (nq == 0) { if (n_pairs) *n_pairs = 0; return CD_OK; }
    return run_traversal(c, c->tb[0], d_queries, nq, pairs, cap_pairs, n_pairs);
}

// ---- the witness of the pair queries (cd_witness.h) ---------------------------------------------------------------------------------
// NULL, or every member NULL: the plain call
static bool witness_wanted(const cd_witness_out *w) { return w && (w->faces || w->points || w->bary || w->feature); }
// The tail of a call that wants a witness or a contour.  rc: what the pass's results() returned; CD_OK or CD_OVERFLOW: the rows are
// there, so the per-row kernel runs (rows: witness_results / contour_results), and its error wins over rc.
extern "C++" {                                  // (a template: the per-row call is a parameter)
template <class Rows> static int rows_tail(bool wanted, int rc, Rows rows)
{
    if (!wanted || (rc != CD_OK && rc != CD_OVERFLOW)) return rc;
    const int rw = rows();
    return rw ? rw : rc;
}
}  // extern "C++"
// Behind a pass that is finished and read back (np = its pair count): the witness kernel over the rows the caller gets, on stream s, and
// the copies into w's arrays.  a, b: the contexts A's and B's triangles come from (the self calls: the same one); ax1 / bx1 / d_toi: the
// end positions and the rows' times on the device (CCD), NULL for proximity.
static int witness_results(hipStream_t s, const WitnessBuf &wb, uint64_t np, uint64_t cap_pairs, const cd_ctx *a, const double *ax1, const cd_ctx *b,
                           const double *bx1, const double *d_toi, const cd_witness_out *w)
{
    const uint64_t take = std::min(np, cap_pairs);
    if (!take) return CD_OK;
    uint32_t *faces = w->faces ? wb.d_faces : nullptr;
    double *points = w->points ? wb.d_points : nullptr, *bary = w->bary ? wb.d_bary : nullptr;
    uint8_t *feat = w->feature ? wb.d_feat : nullptr;
    auto rows = [&](auto toi) {
        k_pair_witness<decltype(toi)::value><<<cdiv(take, WITNESS_THREADS), WITNESS_THREADS, 0, s>>>(wb.d_leaf, take, a->d_leaf, a->d_perm[0], a->d_verts, ax1, b->d_leaf,
                                                                                                     b->d_perm[0], b->d_verts, bx1, d_toi, faces, points, bary, feat);
    };
    if (d_toi) rows(std::true_type{}); else rows(std::false_type{});
    HIPCHK(hipGetLastError());
    if (faces) HIPCHK(hipMemcpyAsync(w->faces, faces, sizeof(uint32_t) * 2 * take, hipMemcpyDeviceToHost, s));
    if (points) HIPCHK(hipMemcpyAsync(w->points, points, sizeof(double) * 6 * take, hipMemcpyDeviceToHost, s));
    if (bary) HIPCHK(hipMemcpyAsync(w->bary, bary, sizeof(double) * 4 * take, hipMemcpyDeviceToHost, s));
    if (feat) HIPCHK(hipMemcpyAsync(w->feature, feat, sizeof(uint8_t) * 2 * take, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CD_OK;
}

// ---- self-proximity (cd_proximity.h) ------------------------------------------------------------------------------------------------
// Own buffers (state, candidates, pairs, distances): the collision path's counters, pair list, statistics and captured step stay as they were.
static bool prox_dist_ok(double dist) { return dist >= 0.0 && dist <= 1.7976931348623157e308; }      // (NaN fails both)
// the two kernels of one pass and the read-back of the counters (no synchronisation)
static int prox_enqueue(cd_ctx *c, double dist, uint64_t cap_pairs, uint2 *wleaf = nullptr /* the witness calls: the hits' leaf positions */)
{
    hipStream_t s = c->stream;
    const uint32_t n = c->nt;
    PairBuf<ProxState> &q = c->prox;
    HIPCHK(hipMemsetAsync(q.state.d, 0, sizeof(ProxState), s));
    k_prox_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, s>>>(c->d_recs32, c->d_leaf, c->d_verts, c->d_boxes, (int)n, dist,
                                                                             c->d_os_ticket + 8, q.state.d, q.d_cand, q.shard_cap);
    auto exact = [&](auto wit) {
        k_prox_exact<decltype(wit)::value><<<dim3(shard_blocks(n), NSHARD), PROX_EXACT_THREADS, 0, s>>>(q.d_cand, q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, dist,
                                                                                                        q.state.d, q.d_pairs, q.d_dists, cap_pairs, wleaf);
    };
    if (wleaf) exact(std::true_type{}); else exact(std::false_type{});
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q.state.h, q.state.d, sizeof(ProxState), hipMemcpyDeviceToHost, s));
    return CD_OK;
}
static int prox_results(cd_ctx *c, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested)
{
    if (n_tested) *n_tested = c->prox.state.h->n_tested;
    return c->prox.results(pairs, nullptr, dists, cap_pairs, n_pairs);
}
static int prox_pass(cd_ctx *c, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested, uint2 *wleaf = nullptr)
{
    for (;;) {
        int rc = prox_enqueue(c, dist, cap_pairs, wleaf);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!c->prox.overflowed(rc)) { if (rc) return rc; break; }
    }
    return prox_results(c, pairs, dists, cap_pairs, n_pairs, n_tested);
}
static int prox_args(cd_ctx *c, double dist, uint32_t *pairs, uint64_t cap_pairs)
{
    if (!c || !prox_dist_ok(dist) || (cap_pairs && !pairs)) return CD_ERR_ARG;
    return CD_OK;
}
static int find_proximity(cd_ctx *c, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested, const cd_witness_out *w)
{
    int rc = prox_args(c, dist, pairs, cap_pairs);
    if (rc) return rc;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    const bool wanted = witness_wanted(w);
    PairBuf<ProxState> &q = c->prox;
    if ((rc = q.ensure(c->nt, cap_pairs)) || (wanted && (rc = q.wit.ensure(cap_pairs)))) return rc;
    rc = prox_pass(c, dist, pairs, dists, cap_pairs, n_pairs, n_tested, wanted ? q.wit.d_leaf : nullptr);
    return rows_tail(wanted, rc, [&] { return witness_results(c->stream, q.wit, q.state.h->n_pairs, cap_pairs, c, nullptr, c, nullptr, nullptr, w); });
}
int cd_find_proximity(cd_ctx *c, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested)
{ return find_proximity(c, dist, pairs, dists, cap_pairs, n_pairs, n_tested, nullptr); }
int cd_find_proximity_witness(cd_ctx *c, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested,
                              const cd_witness_out *w)
{ return find_proximity(c, dist, pairs, dists, cap_pairs, n_pairs, n_tested, w); }
int cd_self_proximity(cd_ctx *c, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested)
{
    int rc = prox_args(c, dist, pairs, cap_pairs);
    if (rc) return rc;
    if ((rc = c->prox.ensure(c->nt, cap_pairs))) return rc;
    sort_retry_tick(c);
    const cd_stats keep = c->stats;                                        // (the build inside does not count as a stage of the collision path)
    rc = fused_step(c, [&]() -> int { const int re = prox_enqueue(c, dist, cap_pairs); return re ? re : sync_with_flags(c); });   // the proximity pass behind the tree: one synchronisation
    if (!rc) {
        if (c->prox.overflowed(rc)) rc = prox_pass(c, dist, pairs, dists, cap_pairs, n_pairs, n_tested);
        else if (!rc) rc = prox_results(c, pairs, dists, cap_pairs, n_pairs, n_tested);
    }
    c->stats = keep;
    return rc;
}
int cd_tri_distance_points(const double *tri, uint64_t n, double *dist)
{
    if (!tri || !dist) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_t = dev.in(tri, 18 * n);
    double *d_o = dev.out<double>(n);
    if (dev.e == hipSuccess) {
        k_tri_distance_points<<<strided_grid(n, 256), 256>>>(d_t, n, d_o);
        dev.e = hipGetLastError();
    }
    dev.back(dist, d_o, n);
    return dev.rc();
}

int cd_tri_witness_points(const double *tri, uint64_t n, double *dist, double *points, double *bary, uint8_t *feature)
{
    if (!tri || !dist) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_t = dev.in(tri, 18 * n);
    double *d_d = dev.out<double>(n), *d_q = dev.out<double>(6 * n), *d_b = dev.out<double>(4 * n);
    uint8_t *d_f = dev.out<uint8_t>(2 * n);
    if (dev.e == hipSuccess) {
        k_tri_witness_points<<<strided_grid(n, WITNESS_THREADS), WITNESS_THREADS>>>(d_t, n, d_d, d_q, d_b, d_f);
        dev.e = hipGetLastError();
    }
    dev.back(dist, d_d, n);
    dev.back(points, d_q, 6 * n);
    dev.back(bary, d_b, 4 * n);
    dev.back(feature, d_f, 2 * n);
    return dev.rc();
}

// ---- continuous collision queries (cd_ccd.h) ------------------------------------------------------------------------------------
// Own buffers (x1, swept records, parent links, arrival counters, state, candidates, pairs, times, distances): the context's vertices,
// the collision path's counters, pair list, statistics and captured step, and the proximity buffers stay as they were.
static bool ccd_dist_ok(double dist) { return dist > 0.0 && dist <= 1.7976931348623157e308; }       // (NaN fails both)
static int ccd_buffers(cd_ctx *c, uint64_t cap_pairs)
{
    int rc = c->ccd.ensure(c->nt, cap_pairs);
    if (!rc) rc = c->ccd_x1.ensure(c->nv, 3);
    return rc ? rc : c->swept[0].ensure(c->nt);
}
// The swept refit of src's tree into sw (sized for src->nt >= 2 leaves): parent links, then the climb from the leaves moving from
// src's vertices to x1.  d_state: the pass's counters, which take M.  On stream s (the between queries run b's refit on a's).
static int enqueue_swept_refit(hipStream_t s, const cd_ctx *src, const double *x1, SweptBuf &sw, CcdState *d_state)
{
    const uint32_t n = src->nt;
    const uint32_t *flags = src->d_os_ticket + 8;
    HIPCHK(hipMemsetAsync(sw.d_up, 0xff, sizeof(int32_t) * 2 * (size_t)n, s));   // -1: no parent (the root; and any link a broken tree lacks)
    k_ccd_links<<<cdiv(n - 1, CCD_THREADS), CCD_THREADS, 0, s>>>(src->d_recs32, (int)n, flags, sw.d_recs, sw.d_up, sw.d_arrive);
    k_ccd_refit<<<cdiv(n, CCD_THREADS), CCD_THREADS, 0, s>>>(src->d_leaf, src->d_verts, x1, (int)n, flags, sw.d_up, sw.d_arrive, sw.d_recs, d_state);
    return CD_OK;
}
// x1 upload, swept refit, descent, exact pass and the read-back of the counters (no synchronisation)
static int ccd_enqueue(cd_ctx *c, const double *verts_end /* NULL: a redo, x1 is there */, double dist, uint64_t cap_pairs, uint2 *wleaf = nullptr)
{
    hipStream_t s = c->stream;
    const uint32_t n = c->nt;
    PairBuf<CcdState> &q = c->ccd;
    double *x1 = c->ccd_x1.d;
    if (verts_end) HIPCHK(hipMemcpyAsync(x1, verts_end, sizeof(double) * 3 * (size_t)c->nv, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(q.state.d, 0, sizeof(CcdState), s));
    if (n >= 2) {
        const int rc = enqueue_swept_refit(s, c, x1, c->swept[0], q.state.d);
        if (rc) return rc;
        k_ccd_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, s>>>(c->swept[0].d_recs, c->d_leaf, c->d_verts, x1, (int)n, dist,
                                                                               c->d_os_ticket + 8, q.state.d, q.d_cand, q.shard_cap);
        auto exact = [&](auto wit) {
            k_ccd_exact<decltype(wit)::value><<<dim3(shard_blocks(n), NSHARD), PROX_EXACT_THREADS, 0, s>>>(q.d_cand, q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, x1, dist,
                                                                                                           q.state.d, q.d_pairs, q.d_toi, q.d_dists, cap_pairs, wleaf);
        };
        if (wleaf) exact(std::true_type{}); else exact(std::false_type{});
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q.state.h, q.state.d, sizeof(CcdState), hipMemcpyDeviceToHost, s));
    return CD_OK;
}
// after a pass that is already enqueued and synchronised: redo it while a shard overflows, then the results
static int ccd_finish(cd_ctx *c, double dist, uint32_t *pairs, double *toi, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, cd_ccd_info *info,
                      uint2 *wleaf = nullptr)
{
    int rc;
    while (c->ccd.overflowed(rc)) {
        if ((rc = ccd_enqueue(c, nullptr, dist, cap_pairs, wleaf))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (rc) return rc;
    c->swept[0].seen = {true, c->nt, c->ccd.state.h->m_bits, dist};
    c->ccd.fill_info(info);
    return c->ccd.results(pairs, toi, dists, cap_pairs, n_pairs);
}
static int ccd_args(cd_ctx *c, const double *verts_end, double dist, uint32_t *pairs, uint64_t cap_pairs)
{
    if (!c || !verts_end || !ccd_dist_ok(dist) || (cap_pairs && !pairs)) return CD_ERR_ARG;
    return CD_OK;
}
static int find_ccd(cd_ctx *c, const double *verts_end, double dist, uint32_t *pairs, double *toi, double *dists, uint64_t cap_pairs, uint64_t *n_pairs,
                    cd_ccd_info *info, const cd_witness_out *w)
{
    int rc = ccd_args(c, verts_end, dist, pairs, cap_pairs);
    if (rc) return rc;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    const bool wanted = witness_wanted(w);
    PairBuf<CcdState> &q = c->ccd;
    if ((rc = ccd_buffers(c, cap_pairs)) || (wanted && (rc = q.wit.ensure(cap_pairs)))) return rc;
    uint2 *wleaf = wanted ? q.wit.d_leaf : nullptr;
    if ((rc = ccd_enqueue(c, verts_end, dist, cap_pairs, wleaf))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    rc = ccd_finish(c, dist, pairs, toi, dists, cap_pairs, n_pairs, info, wleaf);
    return rows_tail(wanted, rc, [&] { return witness_results(c->stream, q.wit, q.state.h->n_pairs, cap_pairs, c, c->ccd_x1.d, c, c->ccd_x1.d, q.d_toi, w); });
}
int cd_find_ccd(cd_ctx *c, const double *verts_end, double dist, uint32_t *pairs, double *toi, double *dists, uint64_t cap_pairs, uint64_t *n_pairs,
                cd_ccd_info *info)
{ return find_ccd(c, verts_end, dist, pairs, toi, dists, cap_pairs, n_pairs, info, nullptr); }
int cd_find_ccd_witness(cd_ctx *c, const double *verts_end, double dist, uint32_t *pairs, double *toi, double *dists, uint64_t cap_pairs, uint64_t *n_pairs,
                        cd_ccd_info *info, const cd_witness_out *w)
{ return find_ccd(c, verts_end, dist, pairs, toi, dists, cap_pairs, n_pairs, info, w); }
int cd_self_ccd(cd_ctx *c, const double *verts_end, double dist, uint32_t *pairs, double *toi, double *dists, uint64_t cap_pairs, uint64_t *n_pairs,
                cd_ccd_info *info)
{
    int rc = ccd_args(c, verts_end, dist, pairs, cap_pairs);
    if (rc) return rc;
    if ((rc = ccd_buffers(c, cap_pairs))) return rc;
    sort_retry_tick(c);
    const cd_stats keep = c->stats;                                        // (the build inside does not count as a stage of the collision path)
    rc = fused_step(c, [&]() -> int { const int re = ccd_enqueue(c, verts_end, dist, cap_pairs); return re ? re : sync_with_flags(c); });   // the CCD pass behind the tree: one synchronisation
    if (!rc) rc = ccd_finish(c, dist, pairs, toi, dists, cap_pairs, n_pairs, info);
    c->stats = keep;
    return rc;
}
int cd_ccd_points(const double *tri, uint64_t n, double dist, double *toi, double *dists, uint32_t *evals)
{
    if (!tri || !toi || !dists || !evals || !ccd_dist_ok(dist)) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_t = dev.in(tri, 36 * n);
    double *d_toi = dev.out<double>(n), *d_d = dev.out<double>(n);
    uint32_t *d_e = dev.out<uint32_t>(n);
    if (dev.e == hipSuccess) {
        k_ccd_points<<<strided_grid(n, CCD_THREADS), CCD_THREADS>>>(d_t, n, dist, d_toi, d_d, d_e);
        dev.e = hipGetLastError();
    }
    dev.back(toi, d_toi, n);
    dev.back(dists, d_d, n);
    dev.back(evals, d_e, n);
    return dev.rc();
}

// ---- queries between two meshes (cd_between.h) ------------------------------------------------------------------------------------
// Everything runs on a's stream, in buffers a owns (state, candidates, pairs, times, distances, x1 of both meshes, b's swept records):
// neither context's vertices, counters, statistics, pair list, captured step, proximity or CCD buffers are touched.  Both trees are
// finished (every call of the library blocks); b's stream is drained all the same before its records are read on a's.
static int bw_args(cd_ctx *a, cd_ctx *b, uint32_t *pairs, uint64_t cap_pairs)
{
    if (!a || !b || a == b || a->device != b->device || (cap_pairs && !pairs)) return CD_ERR_ARG;
    return CD_OK;
}
static int bw_buffers(cd_ctx *a, const cd_ctx *b, uint64_t cap_pairs, bool ccd)
{
    int rc = a->bw.ensure(a->nt, cap_pairs);
    if (!ccd || rc) return rc;
    if ((rc = a->bw_x1a.ensure(a->nv, 3)) || (rc = a->bw_x1b.ensure(b->nv, 3))) return rc;
    return a->swept[1].ensure(b->nt);
}
// one pass (CCD: a's M, b's swept refit; descent; exact stage) and the read-back of the counters (no synchronisation).  ax1 / bx1: device
// pointers to the end positions (CCD only).
static int bw_enqueue(cd_ctx *a, cd_ctx *b, int kind, double dist, uint64_t cap_pairs, const double *ax1, const double *bx1, uint2 *wleaf)
{
    hipStream_t s = a->stream;
    const uint32_t na = a->nt, nb = b->nt;
    const uint32_t *fa = a->d_os_ticket + 8, *fb = b->d_os_ticket + 8;
    PairBuf<CcdState> &q = a->bw;
    HIPCHK(hipMemsetAsync(q.state.d, 0, sizeof(CcdState), s));
    if (kind == BW_CCD) {
        k_between_mbits<<<cdiv(na, CCD_THREADS), CCD_THREADS, 0, s>>>(a->d_leaf, a->d_verts, ax1, (int)na, q.state.d);
        if (nb >= 2) { const int rc = enqueue_swept_refit(s, b, bx1, a->swept[1], q.state.d); if (rc) return rc; }
        k_between_descend<true><<<cdiv(na, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, s>>>(a->swept[1].d_recs, b->d_root, (int)nb, a->d_leaf, a->d_verts, ax1, (int)na,
                                                                                         a->d_boxes, b->d_boxes, dist, fa, fb, q.state.d, q.d_cand, q.shard_cap);
    } else {
        k_between_descend<false><<<cdiv(na, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, s>>>(b->d_recs32, b->d_root, (int)nb, a->d_leaf, a->d_verts, nullptr, (int)na,
                                                                                          a->d_boxes, b->d_boxes, dist, fa, fb, q.state.d, q.d_cand, q.shard_cap);
    }
    auto exact = [&](auto k, auto wit) {
        k_between_exact<decltype(k)::value, decltype(wit)::value><<<dim3(shard_blocks(na), NSHARD), PROX_EXACT_THREADS, 0, s>>>(
            q.d_cand, q.shard_cap, a->d_leaf, a->d_verts, ax1, b->d_leaf, b->d_verts, bx1, dist, q.state.d, q.d_pairs, q.d_toi, q.d_dists, cap_pairs, wleaf);
    };
    auto of_kind = [&](auto k) { if (wleaf) exact(k, std::true_type{}); else exact(k, std::false_type{}); };
    switch (kind) {
    case BW_CONTACT:   of_kind(std::integral_constant<int, BW_CONTACT>{}); break;      // (with leaf positions: the contour call)
    case BW_PROXIMITY: of_kind(std::integral_constant<int, BW_PROXIMITY>{}); break;
    default:           of_kind(std::integral_constant<int, BW_CCD>{}); break;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q.state.h, q.state.d, sizeof(CcdState), hipMemcpyDeviceToHost, s));
    return CD_OK;
}
// enqueue, synchronise, and again with a grown candidate buffer while a shard overflowed
static int bw_pass(cd_ctx *a, cd_ctx *b, int kind, double dist, uint64_t cap_pairs, const double *ax1, const double *bx1, uint2 *wleaf)
{
    for (;;) {
        int rc = bw_enqueue(a, b, kind, dist, cap_pairs, ax1, bx1, wleaf);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(a->stream));
        if (!a->bw.overflowed(rc)) return rc;
    }
}
static int bw_start(cd_ctx *a, cd_ctx *b, uint64_t cap_pairs, bool ccd)
{
    if (a->stage < ST_REFIT || b->stage < ST_REFIT) return CD_ERR_ORDER;
    int rc = bw_buffers(a, b, cap_pairs, ccd);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
    return CD_OK;
}
// (the contact query returns a contour: find_collisions_between, behind contour_results)
static int find_proximity_between(cd_ctx *a, cd_ctx *b, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested,
                                  const cd_witness_out *w)
{
    int rc = bw_args(a, b, pairs, cap_pairs);
    if (rc) return rc;
    if (!prox_dist_ok(dist)) return CD_ERR_ARG;
    const bool wanted = witness_wanted(w);
    PairBuf<CcdState> &q = a->bw;
    if ((rc = bw_start(a, b, cap_pairs, false)) || (wanted && (rc = q.wit.ensure(cap_pairs)))) return rc;
    if ((rc = bw_pass(a, b, BW_PROXIMITY, dist, cap_pairs, nullptr, nullptr, wanted ? q.wit.d_leaf : nullptr))) return rc;
    if (n_tested) *n_tested = q.state.h->n_tested;
    rc = q.results(pairs, nullptr, dists, cap_pairs, n_pairs);
    return rows_tail(wanted, rc, [&] { return witness_results(a->stream, q.wit, q.state.h->n_pairs, cap_pairs, a, nullptr, b, nullptr, nullptr, w); });
}
int cd_find_proximity_between(cd_ctx *a, cd_ctx *b, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested)
{ return find_proximity_between(a, b, dist, pairs, dists, cap_pairs, n_pairs, n_tested, nullptr); }
int cd_find_proximity_between_witness(cd_ctx *a, cd_ctx *b, double dist, uint32_t *pairs, double *dists, uint64_t cap_pairs, uint64_t *n_pairs,
                                      uint64_t *n_tested, const cd_witness_out *w)
{ return find_proximity_between(a, b, dist, pairs, dists, cap_pairs, n_pairs, n_tested, w); }
static int find_ccd_between(cd_ctx *a, const double *verts_end_a, cd_ctx *b, const double *verts_end_b, double dist, uint32_t *pairs, double *toi, double *dists,
                            uint64_t cap_pairs, uint64_t *n_pairs, cd_ccd_info *info, const cd_witness_out *w)
{
    int rc = bw_args(a, b, pairs, cap_pairs);
    if (rc) return rc;
    if (!ccd_dist_ok(dist)) return CD_ERR_ARG;
    const bool wanted = witness_wanted(w);
    PairBuf<CcdState> &q = a->bw;
    if ((rc = bw_start(a, b, cap_pairs, true)) || (wanted && (rc = q.wit.ensure(cap_pairs)))) return rc;
    const double *ax1 = a->d_verts, *bx1 = b->d_verts;                     // NULL: that mesh does not move (x1 = x0)
    if (verts_end_a) { HIPCHK(hipMemcpyAsync(a->bw_x1a.d, verts_end_a, sizeof(double) * 3 * (size_t)a->nv, hipMemcpyHostToDevice, a->stream)); ax1 = a->bw_x1a.d; }
    if (verts_end_b) { HIPCHK(hipMemcpyAsync(a->bw_x1b.d, verts_end_b, sizeof(double) * 3 * (size_t)b->nv, hipMemcpyHostToDevice, a->stream)); bx1 = a->bw_x1b.d; }
    if ((rc = bw_pass(a, b, BW_CCD, dist, cap_pairs, ax1, bx1, wanted ? q.wit.d_leaf : nullptr))) return rc;
    a->swept[1].seen = {true, b->nt, q.state.h->m_bits, dist};
    q.fill_info(info);
    rc = q.results(pairs, toi, dists, cap_pairs, n_pairs);
    return rows_tail(wanted, rc, [&] { return witness_results(a->stream, q.wit, q.state.h->n_pairs, cap_pairs, a, ax1, b, bx1, q.d_toi, w); });
}
int cd_find_ccd_between(cd_ctx *a, const double *verts_end_a, cd_ctx *b, const double *verts_end_b, double dist, uint32_t *pairs, double *toi, double *dists,
                        uint64_t cap_pairs, uint64_t *n_pairs, cd_ccd_info *info)
{ return find_ccd_between(a, verts_end_a, b, verts_end_b, dist, pairs, toi, dists, cap_pairs, n_pairs, info, nullptr); }
int cd_find_ccd_between_witness(cd_ctx *a, const double *verts_end_a, cd_ctx *b, const double *verts_end_b, double dist, uint32_t *pairs, double *toi,
                                double *dists, uint64_t cap_pairs, uint64_t *n_pairs, cd_ccd_info *info, const cd_witness_out *w)
{ return find_ccd_between(a, verts_end_a, b, verts_end_b, dist, pairs, toi, dists, cap_pairs, n_pairs, info, w); }
// ---- the contour of the contact queries (cd_contour.h) ------------------------------------------------------------------------------
// NULL, or every member NULL: no contour kernel
static bool contour_wanted(const cd_contour_out *w) { return w && (w->faces || w->code || w->param || w->points); }
// Behind a pass that is finished and read back (np = its pair count): the contour kernel over the rows the caller gets, on stream s, and
// the copies into w's arrays.  a, b: the contexts A's and B's triangles come from (the self call: the same one).
static int contour_results(hipStream_t s, const ContourBuf &cb, uint64_t np, uint64_t cap_pairs, const cd_ctx *a, const cd_ctx *b, const cd_contour_out *w)
{
    const uint64_t take = std::min(np, cap_pairs);
    if (!take) return CD_OK;
    uint32_t *faces = w->faces ? cb.d_faces : nullptr;
    uint8_t *code = w->code ? cb.d_code : nullptr;
    double *param = w->param ? cb.d_param : nullptr, *points = w->points ? cb.d_points : nullptr;
    k_pair_contour<<<cdiv(take, CONTOUR_THREADS), CONTOUR_THREADS, 0, s>>>(cb.d_leaf, take, a->d_leaf, a->d_perm[0], a->d_verts, b->d_leaf, b->d_perm[0], b->d_verts,
                                                                          faces, code, param, points);
    HIPCHK(hipGetLastError());
    if (faces) HIPCHK(hipMemcpyAsync(w->faces, faces, sizeof(uint32_t) * 2 * take, hipMemcpyDeviceToHost, s));
    if (code) HIPCHK(hipMemcpyAsync(w->code, code, sizeof(uint8_t) * 3 * take, hipMemcpyDeviceToHost, s));
    if (param) HIPCHK(hipMemcpyAsync(w->param, param, sizeof(double) * 6 * take, hipMemcpyDeviceToHost, s));
    if (points) HIPCHK(hipMemcpyAsync(w->points, points, sizeof(double) * 6 * take, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CD_OK;
}
// The self call.  Own buffers (state, candidates, pairs, leaf positions, outputs): the collision path's counters, pair list, statistics, order
// hint and captured step, and every other query's buffers, stay as they were.
int cd_find_collisions_contour(cd_ctx *c, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested, const cd_contour_out *w)
{
    if (!c || (cap_pairs && !pairs)) return CD_ERR_ARG;
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    const bool wanted = contour_wanted(w);
    PairBuf<ProxState> &q = c->cont;
    int rc = q.ensure(c->nt, cap_pairs);
    if (!rc && wanted) rc = q.con.ensure(cap_pairs);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const uint32_t n = c->nt;
    for (;;) {
        HIPCHK(hipMemsetAsync(q.state.d, 0, sizeof(ProxState), s));
        k_prox_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, s>>>(c->d_recs32, c->d_leaf, c->d_verts, c->d_boxes, (int)n, 0.0,
                                                                                 c->d_os_ticket + 8, q.state.d, q.d_cand, q.shard_cap);
        k_contour_exact<<<dim3(shard_blocks(n), NSHARD), PROX_EXACT_THREADS, 0, s>>>(q.d_cand, q.shard_cap, c->d_leaf, c->d_verts, q.state.d, q.d_pairs, cap_pairs,
                                                                                     wanted ? q.con.d_leaf : nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(q.state.h, q.state.d, sizeof(ProxState), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!q.overflowed(rc)) { if (rc) return rc; break; }
    }
    if (n_tested) *n_tested = q.state.h->n_tested;
    rc = q.results(pairs, nullptr, nullptr, cap_pairs, n_pairs);
    return rows_tail(wanted, rc, [&] { return contour_results(s, q.con, q.state.h->n_pairs, cap_pairs, c, c, w); });
}
// The call between two meshes (cd_between.h), in a's buffers.  w without a member set (or NULL): the plain call
static int find_collisions_between(cd_ctx *a, cd_ctx *b, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested, const cd_contour_out *w)
{
    int rc = bw_args(a, b, pairs, cap_pairs);
    if (rc) return rc;
    const bool wanted = contour_wanted(w);
    PairBuf<CcdState> &q = a->bw;
    if ((rc = bw_start(a, b, cap_pairs, false)) || (wanted && (rc = q.con.ensure(cap_pairs)))) return rc;
    if ((rc = bw_pass(a, b, BW_CONTACT, 0.0, cap_pairs, nullptr, nullptr, wanted ? q.con.d_leaf : nullptr))) return rc;
    if (n_tested) *n_tested = q.state.h->n_tested;
    rc = q.results(pairs, nullptr, nullptr, cap_pairs, n_pairs);
    return rows_tail(wanted, rc, [&] { return contour_results(a->stream, q.con, q.state.h->n_pairs, cap_pairs, a, b, w); });
}
int cd_find_collisions_between(cd_ctx *a, cd_ctx *b, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested)
{ return find_collisions_between(a, b, pairs, cap_pairs, n_pairs, n_tested, nullptr); }
int cd_find_collisions_between_contour(cd_ctx *a, cd_ctx *b, uint32_t *pairs, uint64_t cap_pairs, uint64_t *n_pairs, uint64_t *n_tested, const cd_contour_out *w)
{ return find_collisions_between(a, b, pairs, cap_pairs, n_pairs, n_tested, w); }
int cd_tri_isect_points(const double *tri, uint64_t n, uint8_t *code, double *param, double *points)
{
    if (!tri || !code) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_t = dev.in(tri, 18 * n);
    uint8_t *d_c = dev.out<uint8_t>(3 * n);
    double *d_p = param ? dev.out<double>(6 * n) : nullptr, *d_x = points ? dev.out<double>(6 * n) : nullptr;
    if (dev.e == hipSuccess) {
        k_tri_isect_points<<<strided_grid(n, CONTOUR_THREADS), CONTOUR_THREADS>>>(d_t, n, d_c, d_p, d_x);
        dev.e = hipGetLastError();
    }
    dev.back(code, d_c, 3 * n);
    dev.back(param, d_p, 6 * n);
    dev.back(points, d_x, 6 * n);
    return dev.rc();
}

// ---- ray queries (cd_rays.h) ------------------------------------------------------------------------------------------------------
// Own buffers (rays, results, counters): nothing any other call keeps is touched.
// every ray has a finite origin and direction, a direction that is not all zero and a tmax >= 0 (a NaN tmax fails the comparison)
static bool rays_ok(const double *rays, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        const double *r = rays + 7 * i;
        bool finite = true, zero = true;
        for (int k = 0; k < 6; ++k) finite = finite && std::isfinite(r[k]);
        for (int k = 3; k < 6; ++k) zero = zero && r[k] == 0.0;
        if (!finite || zero || !(r[6] >= 0.0)) return false;
    }
    return true;
}
int cd_cast_rays(cd_ctx *c, const double *rays, uint64_t n, int flags, uint32_t *face, uint32_t *ids, double *t, double *uv, uint8_t *side, cd_ray_info *info)
{
    const bool any = flags == CD_RAY_ANY;
    if (!c || (flags != 0 && !any) || (n && (!rays || !face)) || (any && (ids || t || uv || side)) || n > (1ull << 37)) return CD_ERR_ARG;
    if (!rays_ok(rays, n)) return CD_ERR_ARG;                               // before anything is launched: nothing is written for a bad ray
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { if (info) *info = cd_ray_info{0, 0, 0}; return CD_OK; }
    int rc = c->rays.ensure<RayCols>(n);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const RayCols k = c->rays.cols<RayCols>();
    if ((rc = c->rays.upload(s, k.rays, rays, 7, n))) return rc;
    const uint32_t grid = cdiv(n, RAY_THREADS);
    if (any) k_cast_rays<true><<<grid, RAY_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, c->d_boxes, (int)c->nt, k.rays, n, c->rays.state.d,
                                                            k.face, nullptr, nullptr, nullptr, nullptr);
    else k_cast_rays<false><<<grid, RAY_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, c->d_boxes, (int)c->nt, k.rays, n, c->rays.state.d,
                                                         k.face, wanted(ids, k.ids), wanted(t, k.t), wanted(uv, k.uv), wanted(side, k.side));
    if ((rc = c->rays.launched(s)) || (rc = fetch(s, face, k.face, 1, n)) || (rc = fetch(s, ids, k.ids, 1, n)) || (rc = fetch(s, t, k.t, 1, n)) ||
        (rc = fetch(s, uv, k.uv, 2, n)) || (rc = fetch(s, side, k.side, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    item_info(info, c->rays.state.h->n_hits, c->rays.state.h);
    return CD_OK;
}
int cd_ray_tri_points(const double *ray, const double *tri, uint64_t n, uint8_t *hit, double *t, double *uv, uint8_t *side)
{
    if (!ray || !tri || !hit) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_r = dev.in(ray, 7 * n), *d_p = dev.in(tri, 9 * n);
    double *d_t = dev.out<double>(n), *d_uv = dev.out<double>(2 * n);
    uint8_t *d_h = dev.out<uint8_t>(n), *d_s = dev.out<uint8_t>(n);
    if (dev.e == hipSuccess) {
        k_ray_tri_points<<<strided_grid(n, 256), 256>>>(d_r, d_p, n, d_h, d_t, d_uv, d_s);
        dev.e = hipGetLastError();
    }
    dev.back(hit, d_h, n);
    dev.back(t, d_t, n);
    dev.back(uv, d_uv, 2 * n);
    dev.back(side, d_s, n);
    return dev.rc();
}
// ---- closest-point queries (cd_points.h) ------------------------------------------------------------------------------------------
// Own buffers (points, results, counters): nothing any other call keeps is touched.
// every point has finite coordinates and an rmax >= 0 (a NaN rmax fails the comparison)
static bool points_ok(const double *points, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        const double *r = points + 4 * i;
        if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2]) || !(r[3] >= 0.0)) return false;
    }
    return true;
}
int cd_closest_points(cd_ctx *c, const double *points, uint64_t n, int flags, uint32_t *face, uint32_t *ids, double *dist, double *closest, double *uv,
                      uint8_t *feature, uint8_t *side, cd_point_info *info)
{
    const bool any = flags == CD_POINT_ANY;
    if (!c || (flags != 0 && !any) || (n && (!points || !face)) || (any && (ids || dist || closest || uv || feature || side)) || n > (1ull << 37)) return CD_ERR_ARG;
    if (!points_ok(points, n)) return CD_ERR_ARG;                           // before anything is launched: nothing is written for a bad point
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { if (info) *info = cd_point_info{0, 0, 0}; return CD_OK; }
    int rc = c->points.ensure<PointCols>(n);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const PointCols k = c->points.cols<PointCols>();
    if ((rc = c->points.upload(s, k.pts, points, 4, n))) return rc;
    const uint32_t grid = cdiv(n, POINT_THREADS);
    if (any) k_closest_points<true><<<grid, POINT_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, c->d_boxes, (int)c->nt, k.pts, n, c->points.state.d,
                                                                  k.face, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    else k_closest_points<false><<<grid, POINT_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, c->d_boxes, (int)c->nt, k.pts, n, c->points.state.d,
                                                               k.face, wanted(ids, k.ids), wanted(dist, k.dist), wanted(closest, k.closest), wanted(uv, k.uv),
                                                               wanted(feature, k.feature), wanted(side, k.side));
    if ((rc = c->points.launched(s)) || (rc = fetch(s, face, k.face, 1, n)) || (rc = fetch(s, ids, k.ids, 1, n)) || (rc = fetch(s, dist, k.dist, 1, n)) ||
        (rc = fetch(s, closest, k.closest, 3, n)) || (rc = fetch(s, uv, k.uv, 2, n)) || (rc = fetch(s, feature, k.feature, 1, n)) ||
        (rc = fetch(s, side, k.side, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    item_info(info, c->points.state.h->n_found, c->points.state.h);
    return CD_OK;
}
int cd_pt_tri_points(const double *points, const double *tri, uint64_t n, double *dist, double *closest, double *uv, uint8_t *feature, uint8_t *side)
{
    if (!points || !tri || !dist) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_p = dev.in(points, 3 * n), *d_t = dev.in(tri, 9 * n);
    double *d_d = dev.out<double>(n), *d_q = dev.out<double>(3 * n), *d_uv = dev.out<double>(2 * n);
    uint8_t *d_f = dev.out<uint8_t>(n), *d_s = dev.out<uint8_t>(n);
    if (dev.e == hipSuccess) {
        k_pt_tri_points<<<strided_grid(n, 256), 256>>>(d_p, d_t, n, d_d, d_q, d_uv, d_f, d_s);
        dev.e = hipGetLastError();
    }
    dev.back(dist, d_d, n);
    dev.back(closest, d_q, 3 * n);
    dev.back(uv, d_uv, 2 * n);
    dev.back(feature, d_f, n);
    dev.back(side, d_s, n);
    return dev.rc();
}
// ---- all-results item queries (cd_within.h) -----------------------------------------------------------------------------------------
// Own buffers (items, candidates, rows, counters): nothing any other call keeps is touched.  The pass is the pair queries': descent, exact
// stage, the counters' read-back, one synchronisation; a shard that overflowed grows the candidate buffer and the pass runs again.
// the argument rules both calls share, before the items are read
static int item_rows_args(const cd_ctx *c, const double *items, uint64_t n, const uint32_t *rows, uint64_t cap_rows, const uint64_t *n_rows)
{
    return (!c || !n_rows || n > 0xffffffffull || (n && !items) || (cap_rows && !rows)) ? CD_ERR_ARG : CD_OK;   // (the item index of a row is 32 bits)
}
extern "C++" {                                  // (a template: the two kernels of a pass are a parameter)
// enqueue(): memset of the counters aside, the descent and the exact stage of one pass on the stream
template <class Enqueue> static int item_rows_pass(cd_ctx *c, ItemRowsBuf &b, const double *items, uint64_t item_doubles, uint64_t n, Enqueue enqueue)
{
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(b.items.d, items, sizeof(double) * item_doubles * n, hipMemcpyHostToDevice, s));
    for (;;) {
        HIPCHK(hipMemsetAsync(b.q.state.d, 0, sizeof(ProxState), s));
        enqueue();
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(b.q.state.h, b.q.state.d, sizeof(ProxState), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        int rc = CD_OK;
        if (!b.q.overflowed(rc)) return rc;
    }
}
// after the pass: one of the rows' arrays into the caller's, if it was asked for
template <typename T> static int row_values(T *host, const T *dev, uint64_t elems, uint64_t take)
{
    if (host && take) HIPCHK(hipMemcpy(host, dev, sizeof(T) * elems * take, hipMemcpyDeviceToHost));
    return CD_OK;
}
}  // extern "C++"
// workgroups a shard in the exact stage: the candidates grow with the items as well as with the tree
static uint32_t item_rows_blocks(const cd_ctx *c, uint64_t n) { return shard_blocks((uint32_t)std::max<uint64_t>(c->nt, n)); }
int cd_points_within(cd_ctx *c, const double *points, uint64_t n, uint32_t *rows, uint64_t cap_rows, uint64_t *n_rows, uint64_t *n_tested, const cd_point_rows *out)
{
    int rc = item_rows_args(c, points, n, rows, cap_rows, n_rows);
    if (rc) return rc;
    if (!points_ok(points, n)) return CD_ERR_ARG;                           // before anything is launched: nothing is written for a bad point
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { *n_rows = 0; if (n_tested) *n_tested = 0; return CD_OK; }
    ItemRowsBuf &b = c->within;
    if ((rc = b.ensure<WithinRowCols>(n, 4, cap_rows))) return rc;
    const cd_point_rows want = out ? *out : cd_point_rows{};
    const WithinRowCols k = b.cols<WithinRowCols>();
    rc = item_rows_pass(c, b, points, 4, n, [&] {
        k_within_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, c->stream>>>(c->d_recs32, c->d_root, c->d_boxes, (int)c->nt, c->d_os_ticket + 8, b.items.d, n,
                                                                                         b.q.state.d, b.q.d_cand, b.q.shard_cap);
        k_within_exact<<<dim3(item_rows_blocks(c, n), NSHARD), PROX_EXACT_THREADS, 0, c->stream>>>(b.q.d_cand, b.q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, b.items.d, b.q.state.d,
                                                                                                   cap_rows, b.q.d_pairs, wanted(want.ids, k.ids), wanted(want.dist, b.q.d_dists),
                                                                                                   wanted(want.closest, k.closest), wanted(want.uv, k.uv),
                                                                                                   wanted(want.feature, k.feature), wanted(want.side, k.side));
    });
    if (rc) return rc;
    const uint64_t take = std::min<uint64_t>(b.q.state.h->n_pairs, cap_rows);
    if ((rc = row_values(want.ids, k.ids, 1, take)) || (rc = row_values(want.closest, k.closest, 3, take)) || (rc = row_values(want.uv, k.uv, 2, take)) ||
        (rc = row_values(want.feature, k.feature, 1, take)) || (rc = row_values(want.side, k.side, 1, take))) return rc;
    if (n_tested) *n_tested = b.q.state.h->n_tested;
    return b.q.results(rows, nullptr, want.dist, cap_rows, n_rows);
}
int cd_cast_rays_all(cd_ctx *c, const double *rays, uint64_t n, uint32_t *rows, uint64_t cap_rows, uint64_t *n_rows, uint64_t *n_tested, const cd_ray_rows *out)
{
    int rc = item_rows_args(c, rays, n, rows, cap_rows, n_rows);
    if (rc) return rc;
    if (!rays_ok(rays, n)) return CD_ERR_ARG;                               // before anything is launched: nothing is written for a bad ray
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { *n_rows = 0; if (n_tested) *n_tested = 0; return CD_OK; }
    ItemRowsBuf &b = c->rays_all;
    if ((rc = b.ensure<RayRowCols>(n, 7, cap_rows))) return rc;
    const cd_ray_rows want = out ? *out : cd_ray_rows{};
    const RayRowCols k = b.cols<RayRowCols>();
    rc = item_rows_pass(c, b, rays, 7, n, [&] {
        k_rays_all_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, c->stream>>>(c->d_recs32, c->d_root, c->d_boxes, (int)c->nt, c->d_os_ticket + 8, b.items.d, n,
                                                                                           b.q.state.d, b.q.d_cand, b.q.shard_cap);
        k_rays_all_exact<<<dim3(item_rows_blocks(c, n), NSHARD), PROX_EXACT_THREADS, 0, c->stream>>>(b.q.d_cand, b.q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, b.items.d,
                                                                                                     b.q.state.d, cap_rows, b.q.d_pairs, wanted(want.ids, k.ids),
                                                                                                     wanted(want.t, b.q.d_dists), wanted(want.uv, k.uv), wanted(want.side, k.side));
    });
    if (rc) return rc;
    const uint64_t take = std::min<uint64_t>(b.q.state.h->n_pairs, cap_rows);
    if ((rc = row_values(want.ids, k.ids, 1, take)) || (rc = row_values(want.uv, k.uv, 2, take)) || (rc = row_values(want.side, k.side, 1, take))) return rc;
    if (n_tested) *n_tested = b.q.state.h->n_tested;
    return b.q.results(rows, nullptr, want.t, cap_rows, n_rows);
}
// ---- swept-point queries (cd_sweep.h) -------------------------------------------------------------------------------------------------
// Own buffers (items, skip_vertex, x1, swept records and their counters, candidates, rows): nothing any other call keeps is touched --
// swept[0] / swept[1] and what cd_debug_swept reports of them included.  The all-rows call is the all-results item queries' pass with
// the swept refit in front of the descent; the first-contact call is one kernel behind the refit.
// every item has six finite coordinates and a dist that is finite and > 0 (ccd_dist_ok: a NaN fails)
static bool sweeps_ok(const double *items, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        const double *r = items + 7 * i;
        for (int k = 0; k < 6; ++k) if (!std::isfinite(r[k])) return false;
        if (!ccd_dist_ok(r[6])) return false;
    }
    return true;
}
// x1 (NULL: the context's own vertices, the mesh does not move) and skip_vertex (NULL: none) on the device, uploads on the stream
static int sweep_inputs(cd_ctx *c, const double *verts_end, const uint32_t *skip_vertex, uint64_t n, const double *&x1, const uint32_t *&skip)
{
    SweepBuf &b = c->sweep;
    int rc = b.cst.ensure();
    if (!rc && c->nt >= 2) rc = b.swept.ensure(c->nt);
    if (!rc && verts_end) rc = b.x1.ensure(c->nv, 3);
    if (!rc && skip_vertex) rc = b.skip.ensure(n, 1);
    if (rc) return rc;
    x1 = c->d_verts; skip = nullptr;
    if (verts_end) { HIPCHK(hipMemcpyAsync(b.x1.d, verts_end, sizeof(double) * 3 * (size_t)c->nv, hipMemcpyHostToDevice, c->stream)); x1 = b.x1.d; }
    if (skip_vertex) { HIPCHK(hipMemcpyAsync(b.skip.d, skip_vertex, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream)); skip = b.skip.d; }
    return CD_OK;
}
// the counters zeroed and, for a tree with records, the swept refit into this query's own records (M lands in the counters)
static int sweep_refit(cd_ctx *c, const double *x1)
{
    SweepBuf &b = c->sweep;
    HIPCHK(hipMemsetAsync(b.cst.d, 0, sizeof(CcdState), c->stream));
    return c->nt >= 2 ? enqueue_swept_refit(c->stream, c, x1, b.swept, b.cst.d) : CD_OK;
}
int cd_sweep_points_all(cd_ctx *c, const double *verts_end, const double *items, uint64_t n, const uint32_t *skip_vertex, uint32_t *rows, uint64_t cap_rows,
                        uint64_t *n_rows, const cd_sweep_rows *out, cd_ccd_info *info)
{
    int rc = item_rows_args(c, items, n, rows, cap_rows, n_rows);
    if (rc) return rc;
    if (!sweeps_ok(items, n)) return CD_ERR_ARG;                            // before anything is launched: nothing is written for a bad item
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { *n_rows = 0; if (info) *info = cd_ccd_info{0, 0, 0, 0}; return CD_OK; }
    SweepBuf &sb = c->sweep;
    ItemRowsBuf &b = sb.rows;
    if ((rc = b.ensure<SweepRowCols>(n, 7, cap_rows))) return rc;
    const double *x1 = nullptr; const uint32_t *d_skip = nullptr;
    if ((rc = sweep_inputs(c, verts_end, skip_vertex, n, x1, d_skip))) return rc;
    const cd_sweep_rows want = out ? *out : cd_sweep_rows{};
    const SweepRowCols k = b.cols<SweepRowCols>();
    int erc = CD_OK;                                                        // the first error of a pass's own enqueues
    rc = item_rows_pass(c, b, items, 7, n, [&] {
        hipStream_t s = c->stream;
        if ((erc = sweep_refit(c, x1))) return;
        k_sweep_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, s>>>(sb.swept.d_recs, c->d_root, (int)c->nt, c->d_os_ticket + 8, b.items.d, n, sb.cst.d,
                                                                                 b.q.state.d, b.q.d_cand, b.q.shard_cap);
        k_sweep_exact<<<dim3(item_rows_blocks(c, n), NSHARD), PROX_EXACT_THREADS, 0, s>>>(b.q.d_cand, b.q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, x1, b.items.d, d_skip,
                                                                                          b.q.state.d, sb.cst.d, cap_rows, b.q.d_pairs, wanted(want.ids, k.ids),
                                                                                          wanted(want.toi, k.toi), wanted(want.dist, b.q.d_dists),
                                                                                          wanted(want.closest, k.closest), wanted(want.uv, k.uv),
                                                                                          wanted(want.feature, k.feature), wanted(want.side, k.side));
        const hipError_t e = hipMemcpyAsync(sb.cst.h, sb.cst.d, sizeof(CcdState), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) erc = -(int)e;
    });
    if (rc || (rc = erc)) return rc;
    const uint64_t take = std::min<uint64_t>(b.q.state.h->n_pairs, cap_rows);
    if ((rc = row_values(want.ids, k.ids, 1, take)) || (rc = row_values(want.toi, k.toi, 1, take)) || (rc = row_values(want.closest, k.closest, 3, take)) ||
        (rc = row_values(want.uv, k.uv, 2, take)) || (rc = row_values(want.feature, k.feature, 1, take)) || (rc = row_values(want.side, k.side, 1, take))) return rc;
    if (info) {
        uint64_t cand = 0;
        for (int i = 0; i < NSHARD; ++i) cand += b.q.state.h->shard[i * PROX_SHARD_STRIDE];
        *info = cd_ccd_info{cand, b.q.state.h->n_tested, sb.cst.h->n_evals, sb.cst.h->n_unresolved};
    }
    return b.q.results(rows, nullptr, want.dist, cap_rows, n_rows);
}
int cd_sweep_points(cd_ctx *c, const double *verts_end, const double *items, uint64_t n, const uint32_t *skip_vertex, int flags, uint32_t *face, uint32_t *ids,
                    double *toi, double *dist, double *closest, double *uv, uint8_t *feature, uint8_t *side, cd_point_info *info)
{
    if (!c || flags != 0 || (n && (!items || !face)) || n > 0xffffffffull) return CD_ERR_ARG;
    if (!sweeps_ok(items, n)) return CD_ERR_ARG;                            // before anything is launched: nothing is written for a bad item
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { if (info) *info = cd_point_info{0, 0, 0}; return CD_OK; }
    SweepBuf &sb = c->sweep;
    int rc = sb.first.ensure<SweepFirstCols>(n);
    if (rc) return rc;
    const double *x1 = nullptr; const uint32_t *d_skip = nullptr;
    if ((rc = sweep_inputs(c, verts_end, skip_vertex, n, x1, d_skip))) return rc;
    hipStream_t s = c->stream;
    const SweepFirstCols k = sb.first.cols<SweepFirstCols>();
    if ((rc = sb.first.upload(s, k.items, items, 7, n)) || (rc = sweep_refit(c, x1))) return rc;
    k_sweep_first<<<cdiv(n, SWEEP_THREADS), SWEEP_THREADS, 0, s>>>(sb.swept.d_recs, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, x1, (int)c->nt, c->d_os_ticket + 8,
                                                                   k.items, d_skip, n, sb.cst.d, sb.first.state.d, k.face, wanted(ids, k.ids), wanted(toi, k.toi),
                                                                   wanted(dist, k.dist), wanted(closest, k.closest), wanted(uv, k.uv),
                                                                   wanted(feature, k.feature), wanted(side, k.side));
    if ((rc = sb.first.launched(s)) || (rc = fetch(s, face, k.face, 1, n)) || (rc = fetch(s, ids, k.ids, 1, n)) || (rc = fetch(s, toi, k.toi, 1, n)) ||
        (rc = fetch(s, dist, k.dist, 1, n)) || (rc = fetch(s, closest, k.closest, 3, n)) || (rc = fetch(s, uv, k.uv, 2, n)) ||
        (rc = fetch(s, feature, k.feature, 1, n)) || (rc = fetch(s, side, k.side, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    item_info(info, sb.first.state.h->n_found, sb.first.state.h);
    return CD_OK;
}
int cd_pt_advance_points(const double *items, const double *tri, uint64_t n, double *toi, double *dist, double *closest, double *uv, uint8_t *feature, uint8_t *side,
                         uint32_t *evals)
{
    if (!items || !tri || !toi) return CD_ERR_ARG;
    if (!sweeps_ok(items, n)) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_i = dev.in(items, 7 * n), *d_t = dev.in(tri, 18 * n);
    double *d_toi = dev.out<double>(n), *d_d = dev.out<double>(n), *d_q = dev.out<double>(3 * n);
    double *d_uv = dev.out<double>(2 * n);
    uint8_t *d_fs = dev.out<uint8_t>(2 * n);
    uint32_t *d_e = dev.out<uint32_t>(n);
    if (dev.e == hipSuccess) {
        k_pt_advance_points<<<strided_grid(n, CCD_THREADS), CCD_THREADS>>>(d_i, d_t, n, d_toi, d_d, d_q, d_uv, d_fs, d_fs + n, d_e);
        dev.e = hipGetLastError();
    }
    dev.back(toi, d_toi, n);
    dev.back(dist, d_d, n);
    dev.back(closest, d_q, 3 * n);
    dev.back(uv, d_uv, 2 * n);
    dev.back(feature, d_fs, n);
    dev.back(side, d_fs + n, n);
    dev.back(evals, d_e, n);
    return dev.rc();
}
// ---- nearest triangle and separation distance: between two meshes, and of a mesh against itself (cd_nearest.h) ---------------------
// Everything runs on a's stream, in buffers a owns (rows, leaf pairs, witness, counters), with ONE synchronisation: nothing any other
// call keeps is touched.  b == a is the mesh against itself (cd_nearest_self: the nearest NON-NEIGHBOURING triangle), which differs in
// its kernel and in w->faces: those are the faces that PLAYED A and B (not own, partner), a column of their own that k_pair_witness
// writes from the leaf pairs -- so there it runs whenever w asks for anything, and for faces alone it evaluates nothing.
#ifndef CD_NEAREST_SELF_SHARED_BOUND
#define CD_NEAREST_SELF_SHARED_BOUND 1                                      // (0: CD_NEAREST_MIN from the plain kernel's rows -- the build the shared bound was measured against)
#endif
using NearestRows = NearestCols<uint2>;
static int nearest_rows(cd_ctx *a, cd_ctx *b, ItemBuf<NearestState> &nb, double rmax, bool mn, uint32_t *faces, uint32_t *ids, double *dist, const cd_witness_out *w,
                        cd_nearest_info *info)
{
    const bool self = a == b;
    const uint64_t na = a->nt;
    const cd_witness_out want = w ? *w : cd_witness_out{};
    hipStream_t s = a->stream;
    const NearestRows k = nb.cols<NearestRows>(self);
    NearestState *st = nb.state.d, *h = nb.state.h;
    *h = NearestState{};
    std::memcpy(&h->min_bits, &rmax, sizeof rmax);                          // the shared bound starts at rmax
    HIPCHK(hipMemcpyAsync(st, h, sizeof(NearestState), hipMemcpyHostToDevice, s));
    const uint32_t grid = cdiv(na, NEAREST_THREADS);
#define CD_NEAREST_SELF(SHARED) k_nearest_self<SHARED><<<grid, NEAREST_THREADS, 0, s>>>(a->d_recs32, a->d_root, a->d_leaf, a->d_perm[0], a->d_verts, a->d_boxes, (int)na, rmax, st, \
                                                                                      k.faces, k.ids, k.dist, k.leaf)
#define CD_NEAREST_BETWEEN(MIN) k_nearest_between<MIN><<<grid, NEAREST_THREADS, 0, s>>>(b->d_recs32, b->d_root, b->d_leaf, b->d_perm[0], b->d_verts, b->d_boxes, (int)b->nt, \
                                                                                      a->d_leaf, a->d_perm[0], a->d_verts, a->d_boxes, (int)na, rmax, st, k.faces, k.ids, k.dist, k.leaf)
    if (self && mn) CD_NEAREST_SELF(CD_NEAREST_SELF_SHARED_BOUND != 0);
    else if (self) CD_NEAREST_SELF(false);
    else if (mn) CD_NEAREST_BETWEEN(true);
    else CD_NEAREST_BETWEEN(false);
#undef CD_NEAREST_SELF
#undef CD_NEAREST_BETWEEN
    if (mn) k_nearest_min<<<1, NEAREST_MIN_THREADS, 0, s>>>(na, na, st, k.faces, k.ids, k.dist, k.leaf);
    const uint64_t first = mn ? na : 0, rows = mn ? 1 : na;                 // the rows the caller gets
    const uint32_t *w_faces = self ? k.played : k.faces;                    // (between two meshes the faces that played A and B are the row's own)
    if (want.points || want.bary || want.feature || (self && want.faces))
        k_pair_witness<false><<<cdiv(rows, WITNESS_THREADS), WITNESS_THREADS, 0, s>>>(k.leaf + first, rows, a->d_leaf, a->d_perm[0], a->d_verts, nullptr,
                                                                                      b->d_leaf, b->d_perm[0], b->d_verts, nullptr, nullptr,
                                                                                      self ? wanted(want.faces, k.played + 2 * first) : nullptr,
                                                                                      wanted(want.points, k.points + 6 * first), wanted(want.bary, k.bary + 4 * first),
                                                                                      wanted(want.feature, k.feature + 2 * first));
    int rc;
    if ((rc = nb.launched(s)) || (rc = fetch(s, faces, k.faces + 2 * first, 2, rows)) || (rc = fetch(s, want.faces, w_faces + 2 * first, 2, rows)) ||
        (rc = fetch(s, ids, k.ids + 2 * first, 2, rows)) || (rc = fetch(s, dist, k.dist + first, 1, rows)) || (rc = fetch(s, want.points, k.points + 6 * first, 6, rows)) ||
        (rc = fetch(s, want.bary, k.bary + 4 * first, 4, rows)) || (rc = fetch(s, want.feature, k.feature + 2 * first, 2, rows))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    item_info(info, h->n_found, h);
    return CD_OK;
}
// Both trees are finished (every call of the library blocks); b's stream is drained all the same before its records are read on a's.
int cd_nearest_between(cd_ctx *a, cd_ctx *b, double rmax, int flags, uint32_t *faces, uint32_t *ids, double *dist, const cd_witness_out *w, cd_nearest_info *info)
{
    const bool mn = flags == CD_NEAREST_MIN;
    int rc = bw_args(a, b, faces, 1);                                       // (NULL faces: an argument error)
    if (rc) return rc;
    if (!(rmax >= 0.0) || (flags != 0 && !mn)) return CD_ERR_ARG;          // (a NaN rmax fails the comparison)
    if (a->stage < ST_REFIT || b->stage < ST_REFIT) return CD_ERR_ORDER;
    if ((rc = a->nearest.ensure<NearestRows>(a->nt + 1ull, false))) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
    return nearest_rows(a, b, a->nearest, rmax, mn, faces, ids, dist, w, info);
}
int cd_nearest_self(cd_ctx *c, double rmax, int flags, uint32_t *faces, uint32_t *ids, double *dist, const cd_witness_out *w, cd_nearest_info *info)
{
    const bool mn = flags == CD_NEAREST_MIN;
    if (!c || !faces || !(rmax >= 0.0) || (flags != 0 && !mn)) return CD_ERR_ARG;   // (a NaN rmax fails the comparison)
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    const int rc = c->nearest_self.ensure<NearestRows>(c->nt + 1ull, true);
    return rc ? rc : nearest_rows(c, c, c->nearest_self, rmax, mn, faces, ids, dist, w, info);
}
// ---- inside / outside and signed distance (cd_inside.h) ---------------------------------------------------------------------------
// Own buffers (points, results, counters): nothing any other call keeps is touched.
// what both calls reject before anything else is looked at: 0 when the arguments are in order
static int inside_args(const cd_ctx *c, const double *points, uint64_t n, int axis, int flags, const void *required)
{
    if (!c || axis < 0 || axis > 2 || (flags & ~CD_INSIDE_PARITY) || (n && (!points || !required)) || n > (1ull << 37)) return CD_ERR_ARG;
    for (uint64_t i = 0; i < 3 * n; ++i) if (!std::isfinite(points[i])) return CD_ERR_ARG;   // before anything is launched: nothing is written for a bad point
    return c->stage < ST_REFIT ? CD_ERR_ORDER : CD_OK;
}
static void launch_points_inside(cd_ctx *c, int axis, const double *d_pts, int stride, uint64_t n, int parity, PointState *st, uint8_t *inside, uint32_t *n_above,
                                 uint32_t *n_below, int32_t *w_above, int32_t *w_below)
{
    const uint32_t grid = cdiv(n, INSIDE_THREADS);
#define CD_INSIDE_LAUNCH(C) k_points_inside<C><<<grid, INSIDE_THREADS, 0, c->stream>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_verts, c->d_boxes, (int)c->nt, c->d_os_ticket + 8, \
                                                                                     d_pts, stride, n, parity, st, inside, n_above, n_below, w_above, w_below)
    if (axis == 0) CD_INSIDE_LAUNCH(0);
    else if (axis == 1) CD_INSIDE_LAUNCH(1);
    else CD_INSIDE_LAUNCH(2);
#undef CD_INSIDE_LAUNCH
}
int cd_points_inside(cd_ctx *c, const double *points, uint64_t n, int axis, int flags, uint8_t *inside, uint32_t *n_above, uint32_t *n_below, int32_t *w_above,
                     int32_t *w_below, cd_inside_info *info)
{
    int rc = inside_args(c, points, n, axis, flags, inside);
    if (rc) return rc;
    if (n == 0) { if (info) *info = cd_inside_info{0, 0, 0}; return CD_OK; }
    rc = c->inside.ensure<InsideCols>(n);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const InsideCols k = c->inside.cols<InsideCols>();
    if ((rc = c->inside.upload(s, k.pts, points, 3, n))) return rc;
    launch_points_inside(c, axis, k.pts, 3, n, flags & CD_INSIDE_PARITY, c->inside.state.d, k.inside, wanted(n_above, k.n_above), wanted(n_below, k.n_below),
                         wanted(w_above, k.w_above), wanted(w_below, k.w_below));
    if ((rc = c->inside.launched(s)) || (rc = fetch(s, inside, k.inside, 1, n)) || (rc = fetch(s, n_above, k.n_above, 1, n)) ||
        (rc = fetch(s, n_below, k.n_below, 1, n)) || (rc = fetch(s, w_above, k.w_above, 1, n)) || (rc = fetch(s, w_below, k.w_below, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    item_info(info, c->inside.state.h->n_found, c->inside.state.h);
    return CD_OK;
}
// k_closest_points<false> with rmax = +inf and k_points_inside on the same uploaded rows, one synchronisation; the sign is set on the host
int cd_signed_distance(cd_ctx *c, const double *points, uint64_t n, int axis, int flags, double *sdist, uint32_t *face, uint32_t *ids, double *closest, double *uv,
                       uint8_t *feature, uint8_t *inside, cd_point_info *info)
{
    int rc = inside_args(c, points, n, axis, flags, sdist);
    if (rc) return rc;
    if (n == 0) { if (info) *info = cd_point_info{0, 0, 0}; return CD_OK; }
    rc = c->sdist.ensure<PointCols>(n);
    if (!rc) rc = c->sdist_in.ensure();
    if (rc) return rc;
    std::vector<double> rows;                                               // cd_closest_points' rows: the point and rmax = +inf
    std::vector<uint8_t> in_host;
    try { rows.resize(4 * n); in_host.resize(inside ? 0 : n); } catch (const std::bad_alloc &) { return -(int)hipErrorOutOfMemory; }
    uint8_t *in = inside ? inside : in_host.data();
    for (uint64_t i = 0; i < n; ++i) { rows[4 * i] = points[3 * i]; rows[4 * i + 1] = points[3 * i + 1]; rows[4 * i + 2] = points[3 * i + 2]; rows[4 * i + 3] = HUGE_VAL; }
    hipStream_t s = c->stream;
    const PointCols k = c->sdist.cols<PointCols>();
    uint8_t *d_in = k.side;                                                 // (this call keeps inside where the closest-point layout keeps side)
    PointState *st = c->sdist.state.d, *h = c->sdist.state.h, *st_in = c->sdist_in.d, *h_in = c->sdist_in.h;
    if ((rc = c->sdist.upload(s, k.pts, rows.data(), 4, n))) return rc;
    HIPCHK(hipMemsetAsync(st_in, 0, sizeof(PointState), s));
    k_closest_points<false><<<cdiv(n, POINT_THREADS), POINT_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, c->d_boxes, (int)c->nt, k.pts, n, st,
                                                                            k.face, wanted(ids, k.ids), k.dist, wanted(closest, k.closest), wanted(uv, k.uv),
                                                                            wanted(feature, k.feature), nullptr);
    launch_points_inside(c, axis, k.pts, 4, n, flags & CD_INSIDE_PARITY, st_in, d_in, nullptr, nullptr, nullptr, nullptr);
    if ((rc = c->sdist.launched(s))) return rc;
    HIPCHK(hipMemcpyAsync(h_in, st_in, sizeof(PointState), hipMemcpyDeviceToHost, s));
    if ((rc = fetch(s, sdist, k.dist, 1, n)) || (rc = fetch(s, in, d_in, 1, n)) || (rc = fetch(s, face, k.face, 1, n)) || (rc = fetch(s, ids, k.ids, 1, n)) ||
        (rc = fetch(s, closest, k.closest, 3, n)) || (rc = fetch(s, uv, k.uv, 2, n)) || (rc = fetch(s, feature, k.feature, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < n; ++i) if (in[i] && sdist[i] > 0.0) sdist[i] = -sdist[i];   // (a dist of 0 stays +0)
    if (info) { info->n_found = h->n_found; info->node_visits = h->node_visits + h_in->node_visits; info->tri_tests = h->tri_tests + h_in->tri_tests; }
    return CD_OK;
}
int cd_column_tri_points(const double *points, const double *tri, uint64_t n, int axis, int8_t *cover, uint8_t *above, double *E, double *zc, double *S)
{
    if (!points || !tri || !cover || axis < 0 || axis > 2) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_p = dev.in(points, 3 * n), *d_t = dev.in(tri, 9 * n);
    int8_t *d_c = dev.out<int8_t>(n);
    uint8_t *d_a = dev.out<uint8_t>(n);
    double *d_e = dev.out<double>(3 * n), *d_z = dev.out<double>(n), *d_s = dev.out<double>(n);
    if (dev.e == hipSuccess) {
        k_column_tri_points<<<strided_grid(n, 256), 256>>>(d_p, d_t, n, axis, d_c, d_a, d_e, d_z, d_s);
        dev.e = hipGetLastError();
    }
    dev.back(cover, d_c, n);
    dev.back(above, d_a, n);
    dev.back(E, d_e, 3 * n);
    dev.back(zc, d_z, n);
    dev.back(S, d_s, n);
    return dev.rc();
}
// ---- box queries (cd_boxes.h) -----------------------------------------------------------------------------------------------------
// Own buffers (items, candidates, rows, counters): nothing any other call keeps is touched.  The rows call is the all-results item
// queries' pass; the count call is one kernel.
// every bound is finite and lo <= hi on every axis (a NaN fails)
static bool boxes_ok(const double *boxes, uint64_t n)
{
    for (uint64_t i = 0; i < 3 * n; ++i) {
        const double lo = boxes[2 * i], hi = boxes[2 * i + 1];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo <= hi)) return false;
    }
    return true;
}
int cd_boxes_overlap_all(cd_ctx *c, const double *boxes, uint64_t n, uint32_t *rows, uint64_t cap_rows, uint64_t *n_rows, uint64_t *n_tested, const cd_box_rows *out)
{
    int rc = item_rows_args(c, boxes, n, rows, cap_rows, n_rows);
    if (rc) return rc;
    if (!boxes_ok(boxes, n)) return CD_ERR_ARG;                             // before anything is launched: nothing is written for a bad box
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { *n_rows = 0; if (n_tested) *n_tested = 0; return CD_OK; }
    ItemRowsBuf &b = c->boxes_all;
    if ((rc = b.ensure<BoxRowCols>(n, 6, cap_rows))) return rc;
    const cd_box_rows want = out ? *out : cd_box_rows{};
    const BoxRowCols k = b.cols<BoxRowCols>();
    rc = item_rows_pass(c, b, boxes, 6, n, [&] {
        k_boxes_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, c->stream>>>(c->d_recs32, c->d_root, (int)c->nt, c->d_os_ticket + 8, b.items.d, n, b.q.state.d,
                                                                                        b.q.d_cand, b.q.shard_cap);
        k_boxes_exact<<<dim3(item_rows_blocks(c, n), NSHARD), PROX_EXACT_THREADS, 0, c->stream>>>(b.q.d_cand, b.q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, b.items.d, b.q.state.d,
                                                                                                  cap_rows, b.q.d_pairs, wanted(want.ids, k.ids), wanted(want.inside, k.inside));
    });
    if (rc) return rc;
    const uint64_t take = std::min<uint64_t>(b.q.state.h->n_pairs, cap_rows);
    if ((rc = row_values(want.ids, k.ids, 1, take)) || (rc = row_values(want.inside, k.inside, 1, take))) return rc;
    if (n_tested) *n_tested = b.q.state.h->n_tested;
    return b.q.results(rows, nullptr, nullptr, cap_rows, n_rows);
}
int cd_boxes_count(cd_ctx *c, const double *boxes, uint64_t n, int flags, uint32_t *count, uint32_t *n_inside, cd_box_info *info)
{
    if (!c || (flags & ~CD_BOX_ANY) || ((flags & CD_BOX_ANY) && n_inside) || n > 0xffffffffull || (n && (!boxes || !count))) return CD_ERR_ARG;
    if (!boxes_ok(boxes, n)) return CD_ERR_ARG;                             // before anything is launched: nothing is written for a bad box
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { if (info) *info = cd_box_info{0, 0, 0}; return CD_OK; }
    int rc = c->boxes_count.ensure<BoxCountCols>(n);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const BoxCountCols k = c->boxes_count.cols<BoxCountCols>();
    PointState *st = c->boxes_count.state.d;
    if ((rc = c->boxes_count.upload(s, k.boxes, boxes, 6, n))) return rc;
    const uint32_t grid = cdiv(n, BOXES_THREADS);
    if (flags & CD_BOX_ANY)
        k_boxes_count<true><<<grid, BOXES_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_verts, c->d_boxes, (int)c->nt, c->d_os_ticket + 8, k.boxes, n, st, k.count, nullptr);
    else
        k_boxes_count<false><<<grid, BOXES_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_verts, c->d_boxes, (int)c->nt, c->d_os_ticket + 8, k.boxes, n, st, k.count,
                                                            wanted(n_inside, k.n_inside));
    if ((rc = c->boxes_count.launched(s)) || (rc = fetch(s, count, k.count, 1, n)) || (rc = fetch(s, n_inside, k.n_inside, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    item_info(info, c->boxes_count.state.h->n_found, c->boxes_count.state.h);
    return CD_OK;
}
int cd_box_tri_points(const double *boxes, const double *tri, uint64_t n, uint8_t *hit, uint8_t *inside, uint8_t *code)
{
    if (n == 0) return CD_OK;
    if (!boxes || !tri || !hit) return CD_ERR_ARG;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_b = dev.in(boxes, 6 * n), *d_t = dev.in(tri, 9 * n);
    uint8_t *d_h = dev.out<uint8_t>(n), *d_i = dev.out<uint8_t>(n), *d_c = dev.out<uint8_t>(n);
    if (dev.e == hipSuccess) {
        k_box_tri_points<<<strided_grid(n, 256), 256>>>(d_b, d_t, n, d_h, d_i, d_c);
        dev.e = hipGetLastError();
    }
    dev.back(hit, d_h, n);
    dev.back(inside, d_i, n);
    dev.back(code, d_c, n);
    return dev.rc();
}
// ---- plane queries (cd_planes.h) ----------------------------------------------------------------------------------------------------
// Own buffers (items, candidates, rows, counters): nothing any other call keeps is touched.  The rows call is the all-results item
// queries' pass with the slab walk as its descent; the count call is one kernel.  Both launch one lane per (plane, slab).
// every member is finite and the normal is not (0, 0, 0)
static bool planes_ok(const double *planes, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        const double *p = planes + 4 * i;
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(p[3]) || (p[0] == 0.0 && p[1] == 0.0 && p[2] == 0.0)) return false;
    }
    return true;
}
// lanes of a launch over n planes: one per (plane, slab); 0: more than a grid of one-wave workgroups holds
static uint64_t plane_lanes(const cd_ctx *c, uint64_t n)
{
    const uint64_t lanes = n * ((c->nt + (uint64_t)PLANE_SLAB - 1) / PLANE_SLAB);
    return lanes <= (1ull << 36) ? lanes : 0;
}
int cd_planes_cut_all(cd_ctx *c, const double *planes, uint64_t n, uint32_t *rows, uint64_t cap_rows, uint64_t *n_rows, uint64_t *n_tested, const cd_plane_rows *out)
{
    int rc = item_rows_args(c, planes, n, rows, cap_rows, n_rows);
    if (rc) return rc;
    if (!planes_ok(planes, n)) return CD_ERR_ARG;                           // before anything is launched: nothing is written for a bad plane
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { *n_rows = 0; if (n_tested) *n_tested = 0; return CD_OK; }
    const uint64_t lanes = plane_lanes(c, n);
    if (!lanes) return CD_ERR_ARG;
    ItemRowsBuf &b = c->planes_all;
    if ((rc = b.ensure<PlaneRowCols>(n, 4, cap_rows))) return rc;
    const cd_plane_rows want = out ? *out : cd_plane_rows{};
    const PlaneRowCols k = b.cols<PlaneRowCols>();
    rc = item_rows_pass(c, b, planes, 4, n, [&] {
        k_planes_descend<<<cdiv(lanes, PLANES_THREADS), PLANES_THREADS, 0, c->stream>>>(c->d_recs32, c->d_root, c->d_boxes, (int)c->nt, c->d_os_ticket + 8, b.items.d, n,
                                                                                       b.q.state.d, b.q.d_cand, b.q.shard_cap);
        k_planes_exact<<<dim3(item_rows_blocks(c, n), NSHARD), PROX_EXACT_THREADS, 0, c->stream>>>(b.q.d_cand, b.q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, b.items.d, b.q.state.d,
                                                                                                   cap_rows, b.q.d_pairs, wanted(want.ids, k.ids), wanted(want.seg, k.seg),
                                                                                                   wanted(want.edge, k.edge), wanted(want.t, k.t), wanted(want.on, k.on));
    });
    if (rc) return rc;
    const uint64_t take = std::min<uint64_t>(b.q.state.h->n_pairs, cap_rows);
    if ((rc = row_values(want.ids, k.ids, 1, take)) || (rc = row_values(want.seg, k.seg, 6, take)) || (rc = row_values(want.edge, k.edge, 2, take)) ||
        (rc = row_values(want.t, k.t, 2, take)) || (rc = row_values(want.on, k.on, 1, take))) return rc;
    if (n_tested) *n_tested = b.q.state.h->n_tested;
    return b.q.results(rows, nullptr, nullptr, cap_rows, n_rows);
}
int cd_planes_count(cd_ctx *c, const double *planes, uint64_t n, uint32_t *n_cut, uint32_t *n_below, uint32_t *n_above, cd_plane_info *info)
{
    if (!c || n > 0xffffffffull || (n && (!planes || !n_cut))) return CD_ERR_ARG;
    if (!planes_ok(planes, n)) return CD_ERR_ARG;                           // before anything is launched: nothing is written for a bad plane
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { if (info) *info = cd_plane_info{0, 0, 0}; return CD_OK; }
    const uint64_t lanes = plane_lanes(c, n);
    if (!lanes) return CD_ERR_ARG;
    int rc = c->planes_count.ensure<PlaneCountCols>(n);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const PlaneCountCols k = c->planes_count.cols<PlaneCountCols>();
    if ((rc = c->planes_count.upload(s, k.planes, planes, 4, n))) return rc;
    HIPCHK(hipMemsetAsync(k.n_cut, 0, sizeof(uint32_t) * 3 * c->planes_count.block.cap, s));   // the three count columns lie one behind the other
    k_planes_count<<<cdiv(lanes, PLANES_THREADS), PLANES_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_verts, c->d_boxes, (int)c->nt, c->d_os_ticket + 8, k.planes, n,
                                                                         c->planes_count.state.d, k.n_cut, wanted(n_below, k.n_below), wanted(n_above, k.n_above));
    if ((rc = c->planes_count.launched(s)) || (rc = fetch(s, n_cut, k.n_cut, 1, n)) || (rc = fetch(s, n_below, k.n_below, 1, n)) || (rc = fetch(s, n_above, k.n_above, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    uint64_t found = 0;                                                     // (a plane's rows come from many lanes: the host counts the planes that have one)
    for (uint64_t i = 0; i < n; ++i) found += n_cut[i] != 0u;
    item_info(info, found, c->planes_count.state.h);
    return CD_OK;
}
int cd_plane_tri_points(const double *planes, const double *tri, uint64_t n, uint8_t *cls, double *seg, uint8_t *edge, double *t, uint8_t *on)
{
    if (n == 0) return CD_OK;
    if (!planes || !tri || !cls) return CD_ERR_ARG;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_p = dev.in(planes, 4 * n), *d_t = dev.in(tri, 9 * n);
    uint8_t *d_c = dev.out<uint8_t>(n), *d_e = dev.out<uint8_t>(2 * n), *d_on = dev.out<uint8_t>(n);
    double *d_s = dev.out<double>(6 * n), *d_tt = dev.out<double>(2 * n);
    if (dev.e == hipSuccess) {
        k_plane_tri_points<<<strided_grid(n, 256), 256>>>(d_p, d_t, n, d_c, d_s, d_e, d_tt, d_on);
        dev.e = hipGetLastError();
    }
    dev.back(cls, d_c, n);
    dev.back(seg, d_s, 6 * n);
    dev.back(edge, d_e, 2 * n);
    dev.back(t, d_tt, 2 * n);
    dev.back(on, d_on, n);
    return dev.rc();
}
// ---- segment queries (cd_segments.h) --------------------------------------------------------------------------------------------------
// Own buffers (items, candidates, rows, counters): nothing any other call keeps is touched.  The rows call is the all-results item
// queries' pass; the single-answer call is one kernel.
// every coordinate is finite and r >= 0 (a NaN r fails the comparison)
static bool segments_ok(const double *segs, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        const double *r = segs + 7 * i;
        for (int k = 0; k < 6; ++k) if (!std::isfinite(r[k])) return false;
        if (!(r[6] >= 0.0)) return false;
    }
    return true;
}
int cd_segments_within(cd_ctx *c, const double *segs, uint64_t n, uint32_t *rows, uint64_t cap_rows, uint64_t *n_rows, uint64_t *n_tested, const cd_segment_rows *out)
{
    int rc = item_rows_args(c, segs, n, rows, cap_rows, n_rows);
    if (rc) return rc;
    if (!segments_ok(segs, n)) return CD_ERR_ARG;                           // before anything is launched: nothing is written for a bad segment
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { *n_rows = 0; if (n_tested) *n_tested = 0; return CD_OK; }
    ItemRowsBuf &b = c->segments_all;
    if ((rc = b.ensure<SegmentRowCols>(n, 7, cap_rows))) return rc;
    const cd_segment_rows want = out ? *out : cd_segment_rows{};
    const SegmentRowCols k = b.cols<SegmentRowCols>();
    const SegOut o{wanted(want.ids, k.ids), wanted(want.dist, b.q.d_dists), wanted(want.s, k.s), wanted(want.on_seg, k.on_seg), wanted(want.on_tri, k.on_tri),
                   wanted(want.uv, k.uv), wanted(want.feature, k.feature), wanted(want.end, k.end), wanted(want.cross, k.cross), wanted(want.side, k.side)};
    rc = item_rows_pass(c, b, segs, 7, n, [&] {
        k_segments_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, c->stream>>>(c->d_recs32, c->d_root, c->d_boxes, (int)c->nt, c->d_os_ticket + 8, b.items.d, n,
                                                                                           b.q.state.d, b.q.d_cand, b.q.shard_cap);
        k_segments_exact<<<dim3(item_rows_blocks(c, n), NSHARD), PROX_EXACT_THREADS, 0, c->stream>>>(b.q.d_cand, b.q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, b.items.d,
                                                                                                     b.q.state.d, cap_rows, b.q.d_pairs, o);
    });
    if (rc) return rc;
    const uint64_t take = std::min<uint64_t>(b.q.state.h->n_pairs, cap_rows);
    if ((rc = row_values(want.ids, k.ids, 1, take)) || (rc = row_values(want.s, k.s, 1, take)) || (rc = row_values(want.on_seg, k.on_seg, 3, take)) ||
        (rc = row_values(want.on_tri, k.on_tri, 3, take)) || (rc = row_values(want.uv, k.uv, 2, take)) || (rc = row_values(want.feature, k.feature, 1, take)) ||
        (rc = row_values(want.end, k.end, 1, take)) || (rc = row_values(want.cross, k.cross, 1, take)) || (rc = row_values(want.side, k.side, 1, take))) return rc;
    if (n_tested) *n_tested = b.q.state.h->n_tested;
    return b.q.results(rows, nullptr, want.dist, cap_rows, n_rows);
}
int cd_segments_closest(cd_ctx *c, const double *segs, uint64_t n, int flags, uint32_t *face, const cd_segment_rows *out, cd_segment_info *info)
{
    const bool any = flags == CD_SEGMENT_ANY;
    if (!c || (flags != 0 && !any) || (n && (!segs || !face)) || (any && out) || n > 0xffffffffull) return CD_ERR_ARG;
    if (!segments_ok(segs, n)) return CD_ERR_ARG;                           // before anything is launched: nothing is written for a bad segment
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { if (info) *info = cd_segment_info{0, 0, 0}; return CD_OK; }
    int rc = c->segments.ensure<SegmentCols>(n);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const SegmentCols k = c->segments.cols<SegmentCols>();
    const cd_segment_rows want = out ? *out : cd_segment_rows{};
    if ((rc = c->segments.upload(s, k.segs, segs, 7, n))) return rc;
    const uint32_t grid = cdiv(n, SEGMENT_THREADS);
    if (any) k_segments_closest<true><<<grid, SEGMENT_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, c->d_boxes, (int)c->nt, k.segs, n,
                                                                      c->segments.state.d, k.face, SegOut{});
    else k_segments_closest<false><<<grid, SEGMENT_THREADS, 0, s>>>(c->d_recs32, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, c->d_boxes, (int)c->nt, k.segs, n,
                                                                   c->segments.state.d, k.face,
                                                                   SegOut{wanted(want.ids, k.ids), wanted(want.dist, k.dist), wanted(want.s, k.s), wanted(want.on_seg, k.on_seg),
                                                                          wanted(want.on_tri, k.on_tri), wanted(want.uv, k.uv), wanted(want.feature, k.feature),
                                                                          wanted(want.end, k.end), wanted(want.cross, k.cross), wanted(want.side, k.side)});
    if ((rc = c->segments.launched(s)) || (rc = fetch(s, face, k.face, 1, n)) || (rc = fetch(s, want.ids, k.ids, 1, n)) || (rc = fetch(s, want.dist, k.dist, 1, n)) ||
        (rc = fetch(s, want.s, k.s, 1, n)) || (rc = fetch(s, want.on_seg, k.on_seg, 3, n)) || (rc = fetch(s, want.on_tri, k.on_tri, 3, n)) ||
        (rc = fetch(s, want.uv, k.uv, 2, n)) || (rc = fetch(s, want.feature, k.feature, 1, n)) || (rc = fetch(s, want.end, k.end, 1, n)) ||
        (rc = fetch(s, want.cross, k.cross, 1, n)) || (rc = fetch(s, want.side, k.side, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    item_info(info, c->segments.state.h->n_found, c->segments.state.h);
    return CD_OK;
}
int cd_seg_tri_points(const double *segs, const double *tri, uint64_t n, double *dist, double *s, double *on_seg, double *on_tri, double *uv, uint8_t *feature, uint8_t *end,
                      uint8_t *cross, uint8_t *side)
{
    if (n == 0) return CD_OK;
    if (!segs || !tri || !dist) return CD_ERR_ARG;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_a = dev.in(segs, 6 * n), *d_t = dev.in(tri, 9 * n);
    double *d_d = dev.out<double>(n), *d_s = dev.out<double>(n), *d_qs = dev.out<double>(3 * n), *d_qt = dev.out<double>(3 * n), *d_uv = dev.out<double>(2 * n);
    uint8_t *d_f = dev.out<uint8_t>(n), *d_e = dev.out<uint8_t>(n), *d_c = dev.out<uint8_t>(n), *d_sd = dev.out<uint8_t>(n);
    if (dev.e == hipSuccess) {
        k_seg_tri_points<<<strided_grid(n, 256), 256>>>(d_a, d_t, n, SegOut{nullptr, d_d, d_s, d_qs, d_qt, d_uv, d_f, d_e, d_c, d_sd});
        dev.e = hipGetLastError();
    }
    dev.back(dist, d_d, n);
    dev.back(s, d_s, n);
    dev.back(on_seg, d_qs, 3 * n);
    dev.back(on_tri, d_qt, 3 * n);
    dev.back(uv, d_uv, 2 * n);
    dev.back(feature, d_f, n);
    dev.back(end, d_e, n);
    dev.back(cross, d_c, n);
    dev.back(side, d_sd, n);
    return dev.rc();
}
// ---- swept-segment queries (cd_sweep_segments.h) ------------------------------------------------------------------------------------------
// The swept-point queries' calls with 13 doubles an item, two skip indices an item and seg_tri's values a row.  The swept records, their
// counters and x1 are the swept-point queries' (c->sweep: every call refits them for itself); the items, the skip indices, the
// candidates, the rows and the first-contact block are this section's own.  swept[0] / swept[1] stay the last CCD pass's.
// every item has twelve finite coordinates and a dist that is finite and > 0 (ccd_dist_ok: a NaN fails)
static bool sweep_segments_ok(const double *items, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        const double *r = items + 13 * i;
        for (int k = 0; k < 12; ++k) if (!std::isfinite(r[k])) return false;
        if (!ccd_dist_ok(r[12])) return false;
    }
    return true;
}
// sweep_inputs for x1; skip_vertices (NULL: none), 2 an item, into this section's own array
static int sweep_segment_inputs(cd_ctx *c, const double *verts_end, const uint32_t *skip_vertices, uint64_t n, const double *&x1, const uint32_t *&skip)
{
    const uint32_t *none = nullptr;
    int rc = sweep_inputs(c, verts_end, nullptr, n, x1, none);
    if (!rc && skip_vertices) rc = c->sweep_segments.skip.ensure(n, 2);
    if (rc) return rc;
    skip = nullptr;
    if (skip_vertices) {
        HIPCHK(hipMemcpyAsync(c->sweep_segments.skip.d, skip_vertices, sizeof(uint32_t) * 2 * n, hipMemcpyHostToDevice, c->stream));
        skip = c->sweep_segments.skip.d;
    }
    return CD_OK;
}
int cd_sweep_segments_all(cd_ctx *c, const double *verts_end, const double *items, uint64_t n, const uint32_t *skip_vertices, uint32_t *rows, uint64_t cap_rows,
                          uint64_t *n_rows, const cd_sweep_segment_rows *out, cd_ccd_info *info)
{
    int rc = item_rows_args(c, items, n, rows, cap_rows, n_rows);
    if (rc) return rc;
    if (!sweep_segments_ok(items, n)) return CD_ERR_ARG;                    // before anything is launched: nothing is written for a bad item
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { *n_rows = 0; if (info) *info = cd_ccd_info{0, 0, 0, 0}; return CD_OK; }
    SweepBuf &sb = c->sweep;
    ItemRowsBuf &b = c->sweep_segments.rows;
    if ((rc = b.ensure<SweepSegmentRowCols>(n, 13, cap_rows))) return rc;
    const double *x1 = nullptr; const uint32_t *d_skip = nullptr;
    if ((rc = sweep_segment_inputs(c, verts_end, skip_vertices, n, x1, d_skip))) return rc;
    const cd_sweep_segment_rows want = out ? *out : cd_sweep_segment_rows{};
    const SweepSegmentRowCols k = b.cols<SweepSegmentRowCols>();
    const SweepSegOut o{SegOut{wanted(want.ids, k.ids), wanted(want.dist, b.q.d_dists), wanted(want.s, k.s), wanted(want.on_seg, k.on_seg), wanted(want.on_tri, k.on_tri),
                               wanted(want.uv, k.uv), wanted(want.feature, k.feature), wanted(want.end, k.end), wanted(want.cross, k.cross), wanted(want.side, k.side)},
                        wanted(want.toi, k.toi)};
    int erc = CD_OK;                                                        // the first error of a pass's own enqueues
    rc = item_rows_pass(c, b, items, 13, n, [&] {
        hipStream_t s = c->stream;
        if ((erc = sweep_refit(c, x1))) return;
        k_sweep_segments_descend<<<cdiv(n, PROX_DESC_THREADS), PROX_DESC_THREADS, 0, s>>>(sb.swept.d_recs, c->d_root, (int)c->nt, c->d_os_ticket + 8, b.items.d, n, sb.cst.d,
                                                                                          b.q.state.d, b.q.d_cand, b.q.shard_cap);
        k_sweep_segments_exact<<<dim3(item_rows_blocks(c, n), NSHARD), PROX_EXACT_THREADS, 0, s>>>(b.q.d_cand, b.q.shard_cap, c->d_leaf, c->d_perm[0], c->d_verts, x1, b.items.d,
                                                                                                   d_skip, b.q.state.d, sb.cst.d, cap_rows, b.q.d_pairs, o);
        const hipError_t e = hipMemcpyAsync(sb.cst.h, sb.cst.d, sizeof(CcdState), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) erc = -(int)e;
    });
    if (rc || (rc = erc)) return rc;
    const uint64_t take = std::min<uint64_t>(b.q.state.h->n_pairs, cap_rows);
    if ((rc = row_values(want.ids, k.ids, 1, take)) || (rc = row_values(want.toi, k.toi, 1, take)) || (rc = row_values(want.s, k.s, 1, take)) ||
        (rc = row_values(want.on_seg, k.on_seg, 3, take)) || (rc = row_values(want.on_tri, k.on_tri, 3, take)) || (rc = row_values(want.uv, k.uv, 2, take)) ||
        (rc = row_values(want.feature, k.feature, 1, take)) || (rc = row_values(want.end, k.end, 1, take)) || (rc = row_values(want.cross, k.cross, 1, take)) ||
        (rc = row_values(want.side, k.side, 1, take))) return rc;
    if (info) {
        uint64_t cand = 0;
        for (int i = 0; i < NSHARD; ++i) cand += b.q.state.h->shard[i * PROX_SHARD_STRIDE];
        *info = cd_ccd_info{cand, b.q.state.h->n_tested, sb.cst.h->n_evals, sb.cst.h->n_unresolved};
    }
    return b.q.results(rows, nullptr, want.dist, cap_rows, n_rows);
}
int cd_sweep_segments(cd_ctx *c, const double *verts_end, const double *items, uint64_t n, const uint32_t *skip_vertices, int flags, uint32_t *face,
                      const cd_sweep_segment_rows *out, cd_point_info *info)
{
    if (!c || flags != 0 || (n && (!items || !face)) || n > 0xffffffffull) return CD_ERR_ARG;
    if (!sweep_segments_ok(items, n)) return CD_ERR_ARG;                    // before anything is launched: nothing is written for a bad item
    if (c->stage < ST_REFIT) return CD_ERR_ORDER;
    if (n == 0) { if (info) *info = cd_point_info{0, 0, 0}; return CD_OK; }
    SweepBuf &sb = c->sweep;
    ItemBuf<PointState> &fb = c->sweep_segments.first;
    int rc = fb.ensure<SweepSegmentCols>(n);
    if (rc) return rc;
    const double *x1 = nullptr; const uint32_t *d_skip = nullptr;
    if ((rc = sweep_segment_inputs(c, verts_end, skip_vertices, n, x1, d_skip))) return rc;
    hipStream_t s = c->stream;
    const SweepSegmentCols k = fb.cols<SweepSegmentCols>();
    const cd_sweep_segment_rows want = out ? *out : cd_sweep_segment_rows{};
    if ((rc = fb.upload(s, k.items, items, 13, n)) || (rc = sweep_refit(c, x1))) return rc;
    k_sweep_segments_first<<<cdiv(n, SWEEP_SEGMENT_THREADS), SWEEP_SEGMENT_THREADS, 0, s>>>(
        sb.swept.d_recs, c->d_root, c->d_leaf, c->d_perm[0], c->d_verts, x1, (int)c->nt, c->d_os_ticket + 8, k.items, d_skip, n, sb.cst.d, fb.state.d, k.face,
        SweepSegOut{SegOut{wanted(want.ids, k.ids), wanted(want.dist, k.dist), wanted(want.s, k.s), wanted(want.on_seg, k.on_seg), wanted(want.on_tri, k.on_tri),
                           wanted(want.uv, k.uv), wanted(want.feature, k.feature), wanted(want.end, k.end), wanted(want.cross, k.cross), wanted(want.side, k.side)},
                    wanted(want.toi, k.toi)});
    if ((rc = fb.launched(s)) || (rc = fetch(s, face, k.face, 1, n)) || (rc = fetch(s, want.ids, k.ids, 1, n)) || (rc = fetch(s, want.toi, k.toi, 1, n)) ||
        (rc = fetch(s, want.dist, k.dist, 1, n)) || (rc = fetch(s, want.s, k.s, 1, n)) || (rc = fetch(s, want.on_seg, k.on_seg, 3, n)) ||
        (rc = fetch(s, want.on_tri, k.on_tri, 3, n)) || (rc = fetch(s, want.uv, k.uv, 2, n)) || (rc = fetch(s, want.feature, k.feature, 1, n)) ||
        (rc = fetch(s, want.end, k.end, 1, n)) || (rc = fetch(s, want.cross, k.cross, 1, n)) || (rc = fetch(s, want.side, k.side, 1, n))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    item_info(info, fb.state.h->n_found, fb.state.h);
    return CD_OK;
}
int cd_seg_advance_points(const double *items, const double *tri, uint64_t n, double *toi, double *dist, double *s, double *on_seg, double *on_tri, double *uv,
                          uint8_t *feature, uint8_t *end, uint8_t *cross, uint8_t *side, uint32_t *evals)
{
    if (!items || !tri || !toi) return CD_ERR_ARG;
    if (!sweep_segments_ok(items, n)) return CD_ERR_ARG;
    if (n == 0) return CD_OK;
    if (!have_device()) return CD_ERR_NO_DEVICE;
    OneShot dev;
    const double *d_i = dev.in(items, 13 * n), *d_t = dev.in(tri, 18 * n);
    double *d_toi = dev.out<double>(n), *d_d = dev.out<double>(n), *d_s = dev.out<double>(n), *d_qs = dev.out<double>(3 * n), *d_qt = dev.out<double>(3 * n);
    double *d_uv = dev.out<double>(2 * n);
    uint8_t *d_b = dev.out<uint8_t>(4 * n);                                 // feature, end, cross, side
    uint32_t *d_e = dev.out<uint32_t>(n);
    if (dev.e == hipSuccess) {
        k_seg_advance_points<<<strided_grid(n, CCD_THREADS), CCD_THREADS>>>(d_i, d_t, n, SweepSegOut{SegOut{nullptr, d_d, d_s, d_qs, d_qt, d_uv, d_b, d_b + n, d_b + 2 * n, d_b + 3 * n}, d_toi},
                                                                            d_e);
        dev.e = hipGetLastError();
    }
    dev.back(toi, d_toi, n);
    dev.back(dist, d_d, n);
    dev.back(s, d_s, n);
    dev.back(on_seg, d_qs, 3 * n);
    dev.back(on_tri, d_qt, 3 * n);
    dev.back(uv, d_uv, 2 * n);
    dev.back(feature, d_b, n);
    dev.back(end, d_b + n, n);
    dev.back(cross, d_b + 2 * n, n);
    dev.back(side, d_b + 3 * n, n);
    dev.back(evals, d_e, n);
    return dev.rc();
}
}  // extern "C"

#include "cd_multi.h"
