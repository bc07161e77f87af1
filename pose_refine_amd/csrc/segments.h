// segments.h -- depth-connected components of a frame: THE definition of a measured depth, the link test, a record's update and the order key
// (include/pose_refine.h states it in words), one copy for the kernels of segments.hip and the host twin of pr_segments.cpp, and the launchers
// of segments.hip.  Integers only: device and host agree bit for bit.
#pragma once
#include <stdint.h>

#include "pr_internal.h"

#if defined(__HIP__)
#define SEG_FN __host__ __device__ __forceinline__
#else
#define SEG_FN inline
#endif

namespace segments {

static_assert(sizeof(pr_segment_params) == 16 && sizeof(pr_segment) == 64, "pr_segment_params / pr_segment layout");

constexpr uint32_t kNone = 0xFFFFFFFFu;                          // a pixel without a measurement: its parent, its root; a root without a slot

// a pixel's depth as the link test takes it: 0 = not measured (a negative int32 included), else 1 .. 2^31 - 1
SEG_FN uint32_t depth_of(uint16_t v) { return (uint32_t)v; }
SEG_FN uint32_t depth_of(int32_t v) { return v > 0 ? (uint32_t)v : 0u; }
// two 4-neighbours with these depths are linked
SEG_FN bool linked(uint32_t a, uint32_t b, uint32_t jump) { return a != 0u && b != 0u && (a > b ? a - b : b - a) <= jump; }

// What a piece of a segment (a pixel, a run of a row) adds to its record, and the record as it is accumulated: min / max / add only, so any order
// and any split into pieces gives the same bytes.
struct Part { uint32_t x0, x1, y0, y1, dmin, dmax, n; uint64_t sx, sy, sd; };      // the piece's box, depth range and pixel count; sx, sy, sd: its sums of x, y and depth
struct Acc { uint32_t x0, y0, x1, y1, dmin, dmax, pixels, pad; uint64_t sx, sy, sd, pad2; };
static_assert(sizeof(Acc) == 64, "Acc: 64 bytes, whole 16-byte words");
SEG_FN Acc acc_empty() { return Acc{ kNone, kNone, 0u, 0u, kNone, 0u, 0u, 0u, 0ull, 0ull, 0ull, 0ull }; }
SEG_FN Part part_of_pixel(uint32_t x, uint32_t y, uint32_t d) { return Part{ x, x, y, y, d, d, 1u, (uint64_t)x, (uint64_t)y, (uint64_t)d }; }
// op: min32 / max32 / add32 / add64 on a word of the record (plain on the host, atomics on the device)
template <class Op>
SEG_FN void acc_merge(Acc *a, const Part &p, Op op)
{
    op.min32(&a->x0, p.x0); op.max32(&a->x1, p.x1); op.min32(&a->y0, p.y0); op.max32(&a->y1, p.y1);
    op.min32(&a->dmin, p.dmin); op.max32(&a->dmax, p.dmax); op.add32(&a->pixels, p.n);
    op.add64(&a->sx, p.sx); op.add64(&a->sy, p.sy); op.add64(&a->sd, p.sd);
}
// the order of the qualifying components: ascending key = pixels descending, then root ascending
SEG_FN uint64_t order_key(uint32_t pixels, uint32_t root) { return ((uint64_t)(0xFFFFFFFFu - pixels) << 32) | (uint64_t)root; }
// the label of the component at position `rank` (0-based) of that order
SEG_FN uint16_t label_of_rank(uint32_t rank, uint32_t n_found) { return rank < n_found ? (uint16_t)(rank + 1u) : (uint16_t)PR_SEGMENT_DROPPED; }
// the caller's record from an accumulated one
SEG_FN pr_segment record(uint32_t root, const Acc &a)
{
    pr_segment s;
    s.root = root; s.pixels = a.pixels; s.x0 = (uint16_t)a.x0; s.y0 = (uint16_t)a.y0; s.x1 = (uint16_t)a.x1; s.y1 = (uint16_t)a.y1;
    s.depth_min = a.dmin; s.depth_max = a.dmax; s.sum_x = a.sx; s.sum_y = a.sy; s.sum_depth = a.sd; s.reserved[0] = 0; s.reserved[1] = 0;
    return s;
}

}  // namespace segments

namespace prk {

constexpr uint32_t kSegChunk = 1024;                             // pixel indices per chunk of the root compaction (count, scan, emit)
// the control words of a call as the device leaves them (read back with the list of qualifying roots behind them)
struct SegControl { uint32_t n_qualifying, n_components, pad[2]; };
static_assert(sizeof(SegControl) == 16, "SegControl: one 16-byte word");
struct SegRoot { uint32_t root, pixels; };                       // one qualifying component, in root order

// segments.hip.  parent, count: one word per pixel; chunk_count[n_chunks], chunk_off[n_chunks + 1]; roots: PR_SEGMENT_MAX_ROOTS entries; acc: n_acc records
hipError_t launch_segment_init(SegControl *ctl, segments::Acc *acc, uint32_t n_acc, hipStream_t s);
// every pixel's parent = the lowest pixel of its component WITHIN its 64 x 16 tile (kNone: not measured); count zeroed
hipError_t launch_segment_tiles(const void *depth, bool depth_i32, uint32_t width, uint32_t height, uint32_t jump, uint32_t *parent, uint32_t *count, hipStream_t s);
// the links across tile borders united on the parent array
hipError_t launch_segment_seams(const void *depth, bool depth_i32, uint32_t width, uint32_t height, uint32_t jump, uint32_t *parent, hipStream_t s);
// parent = root for every pixel, count[root] = the component's pixels
hipError_t launch_segment_flatten(uint32_t width, uint32_t height, uint32_t *parent, uint32_t *count, hipStream_t s);
// the qualifying roots in root order into roots[] (at most PR_SEGMENT_MAX_ROOTS stored; ctl counts all), count[root] = the root's position there or kNone;
// then ctl and the stored roots to out_mapped (SegControl, then SegRoot[])
hipError_t launch_segment_compact(const uint32_t *parent, uint32_t *count, uint32_t n_px, uint32_t min_pixels, uint32_t *chunk_count, uint32_t *chunk_off,
                                  SegRoot *roots, SegControl *ctl, void *out_mapped, hipStream_t s);
// labels from rank_label[position of the pixel's root], the records of labels 1 .. n_found accumulated, roots_out (may be null) = parent
hipError_t launch_segment_relabel(const void *depth, bool depth_i32, uint32_t width, uint32_t height, const uint32_t *parent, const uint32_t *slot,
                                  const uint16_t *rank_label, uint32_t n_found, uint16_t *labels, uint32_t *roots_out, segments::Acc *acc, hipStream_t s);
// depth_out = depth_in where keep_bits has the pixel's label's bit (labels below n_keep only), else 0
hipError_t launch_segment_depth(const uint16_t *labels, const void *depth_in, void *depth_out, bool depth_i32, uint32_t n_px, const uint32_t *keep_bits,
                                uint32_t n_keep, hipStream_t s);

}  // namespace prk
