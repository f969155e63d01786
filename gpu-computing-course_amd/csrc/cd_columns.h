// cd_columns.h -- the device blocks of the per-item queries (mi355cd.hip), each stated ONCE as a list of columns.
// Host only, no HIP: a plain C++ program can include it (tests/test_columns_layout.py does, under the address sanitizer).
//
// A block of `cap` items is column after column, not item after item: column k starts at base + cap * (the bytes an item has in the
// columns before it).  A query's struct declares its columns in that order, each initialised by col<T>(elements an item), so the one
// list gives the bytes an item needs (column_bytes: the list walked without a block) and the pointers into an allocated block (carve).
// The order is doubles, 8-byte pairs, 4-byte words, bytes: no column's elements are larger than those of the column before it, so
// every column is aligned for every cap without padding.  A list that breaks this does not compile (the static_assert at the end).
#pragma once
#include <cstdint>
#include <cstdlib>

namespace cd {

inline void column_wider_than_the_one_before() { std::abort(); }           // not constexpr: reaching it fails the list's static_assert

struct Columns {
    char *base; uint64_t cap;                                               // the block and the items it holds (no block: sizes only)
    uint64_t bytes = 0, last = 8;                                           // bytes an item so far; element size of the last column
    constexpr Columns(char *block = nullptr, uint64_t items = 0) : base(block), cap(items) {}
    template <typename T> constexpr T *col(uint64_t elems)                  // the next column: `elems` elements of T an item
    {
        if (sizeof(T) > last) column_wider_than_the_one_before();
        T *p = base ? reinterpret_cast<T *>(base + bytes * cap) : nullptr;
        bytes += sizeof(T) * elems; last = sizeof(T);
        return p;
    }
};
// the bytes an item (a row) has in Cols' block: what the buffer's ensure() gets  (a...: what the list depends on, NearestCols' self)
template <class Cols, class... A> constexpr uint64_t column_bytes(A... a) { Cols k{Columns(), a...}; return k.bytes; }
// the columns of an allocated block of `cap` items
template <class Cols, class... A> Cols carve(char *base, uint64_t cap, A... a) { return Cols{Columns(base, cap), a...}; }

struct alignas(8) LeafPair { uint32_t x, y; };                              // stands in for HIP's uint2 where that is not defined

// ---- blocks of n items (ItemBuf::block) -------------------------------------------------------------------------------------------
struct RayCols : Columns {                      // cd_cast_rays: the ray, t, uv, face, ID, side
    double *rays = col<double>(7), *t = col<double>(1), *uv = col<double>(2); uint32_t *face = col<uint32_t>(1), *ids = col<uint32_t>(1); uint8_t *side = col<uint8_t>(1);
};
// cd_closest_points: the point with its rmax, dist, closest, uv, face, ID, feature, side.  cd_signed_distance's block is the same
// list (its first kernel is cd_closest_points'), except that it keeps `inside` where this one keeps `side`.
struct PointCols : Columns {
    double *pts = col<double>(4), *dist = col<double>(1), *closest = col<double>(3), *uv = col<double>(2); uint32_t *face = col<uint32_t>(1), *ids = col<uint32_t>(1);
    uint8_t *feature = col<uint8_t>(1), *side = col<uint8_t>(1);
};
struct SweepFirstCols : Columns {               // cd_sweep_points: the item, toi, dist, closest, uv, face, ID, feature, side
    double *items = col<double>(7), *toi = col<double>(1), *dist = col<double>(1), *closest = col<double>(3), *uv = col<double>(2);
    uint32_t *face = col<uint32_t>(1), *ids = col<uint32_t>(1); uint8_t *feature = col<uint8_t>(1), *side = col<uint8_t>(1);
};
// cd_nearest_between / cd_nearest_self, nt + 1 rows (the last one: CD_NEAREST_MIN's): dist, points, bary, leaf pair, faces, IDs,
// feature -- and for the mesh against itself (self) the faces that PLAYED A and B, behind the IDs
template <class Pair = LeafPair> struct NearestCols : Columns {
    static_assert(sizeof(Pair) == 8 && alignof(Pair) == 8, "two 32-bit leaf positions");
    bool self;
    double *dist = col<double>(1), *points = col<double>(6), *bary = col<double>(4); Pair *leaf = col<Pair>(1);
    uint32_t *faces = col<uint32_t>(2), *ids = col<uint32_t>(2), *played = self ? col<uint32_t>(2) : nullptr; uint8_t *feature = col<uint8_t>(2);
};
struct InsideCols : Columns {                   // cd_points_inside: the point, the four counts, inside
    double *pts = col<double>(3); uint32_t *n_above = col<uint32_t>(1), *n_below = col<uint32_t>(1); int32_t *w_above = col<int32_t>(1), *w_below = col<int32_t>(1);
    uint8_t *inside = col<uint8_t>(1);
};
struct BoxCountCols : Columns {                 // cd_boxes_count: the box, count, n_inside
    double *boxes = col<double>(6); uint32_t *count = col<uint32_t>(1), *n_inside = col<uint32_t>(1);
};
struct PlaneCountCols : Columns {               // cd_planes_count: the plane, n_cut, n_below, n_above
    double *planes = col<double>(4); uint32_t *n_cut = col<uint32_t>(1), *n_below = col<uint32_t>(1), *n_above = col<uint32_t>(1);
};
struct SegmentCols : Columns {                  // cd_segments_closest: the segment with its r, dist, s, on_seg, on_tri, uv, face, ID, feature, end, cross, side
    double *segs = col<double>(7), *dist = col<double>(1), *s = col<double>(1), *on_seg = col<double>(3), *on_tri = col<double>(3), *uv = col<double>(2);
    uint32_t *face = col<uint32_t>(1), *ids = col<uint32_t>(1); uint8_t *feature = col<uint8_t>(1), *end = col<uint8_t>(1), *cross = col<uint8_t>(1), *side = col<uint8_t>(1);
};
struct SweepSegmentCols : Columns {             // cd_sweep_segments: the item, toi, dist, s, on_seg, on_tri, uv, face, ID, feature, end, cross, side
    double *items = col<double>(13), *toi = col<double>(1), *dist = col<double>(1), *s = col<double>(1), *on_seg = col<double>(3), *on_tri = col<double>(3), *uv = col<double>(2);
    uint32_t *face = col<uint32_t>(1), *ids = col<uint32_t>(1); uint8_t *feature = col<uint8_t>(1), *end = col<uint8_t>(1), *cross = col<uint8_t>(1), *side = col<uint8_t>(1);
};

// ---- blocks of cap_rows rows (ItemRowsBuf::vals): what a row has besides (item, face) and its dist / t, which are the pair record's ----
struct WithinRowCols : Columns {                // cd_points_within: closest, uv, ID, feature, side
    double *closest = col<double>(3), *uv = col<double>(2); uint32_t *ids = col<uint32_t>(1); uint8_t *feature = col<uint8_t>(1), *side = col<uint8_t>(1);
};
struct RayRowCols : Columns {                   // cd_cast_rays_all: uv, ID, side
    double *uv = col<double>(2); uint32_t *ids = col<uint32_t>(1); uint8_t *side = col<uint8_t>(1);
};
struct SweepRowCols : Columns {                 // cd_sweep_points_all: toi, closest, uv, ID, feature, side
    double *toi = col<double>(1), *closest = col<double>(3), *uv = col<double>(2); uint32_t *ids = col<uint32_t>(1); uint8_t *feature = col<uint8_t>(1), *side = col<uint8_t>(1);
};
struct BoxRowCols : Columns {                   // cd_boxes_overlap_all (no dist): ID, inside
    uint32_t *ids = col<uint32_t>(1); uint8_t *inside = col<uint8_t>(1);
};
struct PlaneRowCols : Columns {                 // cd_planes_cut_all (no dist): the segment a b, t of each, ID, edge of each, on
    double *seg = col<double>(6), *t = col<double>(2); uint32_t *ids = col<uint32_t>(1); uint8_t *edge = col<uint8_t>(2), *on = col<uint8_t>(1);
};
struct SegmentRowCols : Columns {               // cd_segments_within: s, on_seg, on_tri, uv, ID, feature, end, cross, side
    double *s = col<double>(1), *on_seg = col<double>(3), *on_tri = col<double>(3), *uv = col<double>(2); uint32_t *ids = col<uint32_t>(1);
    uint8_t *feature = col<uint8_t>(1), *end = col<uint8_t>(1), *cross = col<uint8_t>(1), *side = col<uint8_t>(1);
};
struct SweepSegmentRowCols : Columns {          // cd_sweep_segments_all: toi, s, on_seg, on_tri, uv, ID, feature, end, cross, side
    double *toi = col<double>(1), *s = col<double>(1), *on_seg = col<double>(3), *on_tri = col<double>(3), *uv = col<double>(2); uint32_t *ids = col<uint32_t>(1);
    uint8_t *feature = col<uint8_t>(1), *end = col<uint8_t>(1), *cross = col<uint8_t>(1), *side = col<uint8_t>(1);
};

// every list is walked at compile time: one whose columns widen calls the function above, which is no constant expression
static_assert(column_bytes<RayCols>() + column_bytes<PointCols>() + column_bytes<SweepFirstCols>() + column_bytes<NearestCols<>>(false) + column_bytes<NearestCols<>>(true) +
              column_bytes<InsideCols>() + column_bytes<BoxCountCols>() + column_bytes<PlaneCountCols>() + column_bytes<WithinRowCols>() + column_bytes<RayRowCols>() + column_bytes<SweepRowCols>() +
              column_bytes<BoxRowCols>() + column_bytes<PlaneRowCols>() + column_bytes<SegmentCols>() + column_bytes<SegmentRowCols>() +
              column_bytes<SweepSegmentCols>() + column_bytes<SweepSegmentRowCols>() > 0, "a column's elements are larger than those of the column before it");

}  // namespace cd
