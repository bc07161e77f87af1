// frame_stage.h -- what the frame stages' host drivers share (pr_depth_filter.cpp, pr_reproject.cpp, pr_planes.cpp, pr_segments.cpp, pr_cloud.cpp,
// pr_ppf.cpp): the size rule of a depth frame, the depth gate and the window rule of a parameter block, the uint16 / int32 dispatch, and the layout
// of "one device block: a | b | c" with the blocks of the stages described by it.  Host only.  No HIP call in here: tools/job_sanitize.cpp runs the
// rules and the layouts under ASan / UBSan.  (A stage's write into the caller's memory is announced with note_write, pr_runtime.h, before the
// first launch that writes and after the last check that can still refuse.)
#pragma once
#include "pr_runtime.h"
#include "planes.h"
#include "ppf.h"
#include "segments.h"

namespace prr {

// ---- a depth frame as the stages that read or write one take it (pr_scene_planes_* and pr_ppf_scene_points_dev take a scene: frame_ok) ----
constexpr size_t kMaxDepthPixels = (size_t)1 << 26;
// what: whose size it is ("a frame", "the target", "sources[2]: a frame")
inline int depth_frame_ok(const char *fn, const char *what, size_t W, size_t H)
{
    if (W == 0 || H == 0 || W > 65535 || H > 65535 || W * H > kMaxDepthPixels) {
        set_error("%s: %s is 1 .. 65535 on a side and at most 2^26 pixels (got %zux%zu)", fn, what, W, H); return PR_ERR_INVALID;
    }
    return PR_OK;
}
// the same for a call that takes the pixels as one count
inline int depth_frame_ok(const char *fn, size_t n_px)
{
    if (n_px == 0 || n_px > kMaxDepthPixels) { set_error("%s: n_px must be 1 .. 2^26 (got %zu)", fn, n_px); return PR_ERR_INVALID; }
    return PR_OK;
}

// ---- the rules two parameter blocks share (block: the struct's name) ----
// the depth gate and the tolerance tol(d) = tol_mm + d * tol_permille / 1000
inline int gate_ok(const char *fn, const char *block, uint32_t min_mm, uint32_t max_mm, uint32_t tol_mm, uint32_t tol_permille)
{
    if (min_mm > 0x7FFFFFFFu || max_mm > 0x7FFFFFFFu || tol_mm > 0x7FFFFFFFu) {
        set_error("%s: %s: min_mm, max_mm and tol_mm must not exceed 2^31 - 1 (got %u, %u, %u)", fn, block, min_mm, max_mm, tol_mm); return PR_ERR_INVALID;
    }
    if (max_mm != 0 && min_mm > max_mm) { set_error("%s: %s: min_mm = %u lies above max_mm = %u", fn, block, min_mm, max_mm); return PR_ERR_INVALID; }
    if (tol_permille > 1000) { set_error("%s: %s: tol_permille must not exceed 1000 (got %u)", fn, block, tol_permille); return PR_ERR_INVALID; }
    return PR_OK;
}
// a square window of 2 radius + 1 pixels on a side and a count of its pixels other than the centre
inline int window_ok(const char *fn, const char *block, const char *radius_name, uint32_t radius, uint32_t max_radius, const char *count_name, uint32_t count)
{
    if (radius > max_radius) { set_error("%s: %s: %s must be 0 .. %u (got %u)", fn, block, radius_name, max_radius, radius); return PR_ERR_INVALID; }
    const uint32_t side = 2 * radius + 1;
    if (count != 0 && (radius == 0 || count > side * side - 1)) {
        set_error("%s: %s: %s = %u needs %s >= 1 and must not exceed (2 %s + 1)^2 - 1 = %u", fn, block, count_name, count, radius_name, radius_name, side * side - 1); return PR_ERR_INVALID;
    }
    return PR_OK;
}

// ---- a depth image is uint16 or int32: f(typed pointer), whatever f returns ----
template <class F>
inline auto with_depth(const void *p, bool is_i32, F &&f)
{
    if (is_i32) return f(static_cast<const int32_t *>(p));
    return f(static_cast<const uint16_t *>(p));
}
template <class F>
inline auto with_depth(void *p, bool is_i32, F &&f)
{
    if (is_i32) return f(static_cast<int32_t *>(p));
    return f(static_cast<uint16_t *>(p));
}
inline size_t depth_bytes(bool is_i32) { return is_i32 ? sizeof(int32_t) : sizeof(uint16_t); }

// ---- one block, several parts: take() hands out the parts' offsets in order, each on `align` bytes (a power of two) ----
struct Block {
    size_t end = 0;
    template <class T> size_t take(size_t count, size_t align = 16)
    {
        const size_t at = (end + align - 1) & ~(align - 1);
        end = at + sizeof(T) * count;
        return at;
    }
    size_t bytes() const { return end; }
};
template <class T> inline T *at(void *base, size_t off) { return reinterpret_cast<T *>(static_cast<unsigned char *>(base) + off); }
// the rows of a count-and-scan compaction: count[n] | off[n + 1], the total at off[n]
struct ScanRows {
    uint32_t *count, *off, *total;
    static size_t words(size_t n) { return 2 * n + 1; }
    ScanRows(void *base, size_t at_bytes, size_t n) : count(at<uint32_t>(base, at_bytes)), off(count + n), total(off + n) {}
};

// ---- the stages' blocks (the order of the parts and their alignments are the kernels': 16-byte accesses); b.bytes() is a block's size ----
// pr_scene_planes_dev: the rounds' records | row counts and offsets | the samples' points | their normals | the support table (unless the caller's), a row of PR_PLANE_MAX_CANDIDATES words per round
struct PlaneBlock {
    Block b;
    size_t rounds, rows, pts, nrm, support;
    PlaneBlock(uint32_t n_planes, uint32_t grid_rows, bool own_support)
        : rounds(b.take<prk::PlaneRound>(n_planes)), rows(b.take<uint32_t>(ScanRows::words(grid_rows))), pts(b.take<prk::PlaneSample>(PR_PLANE_MAX_SAMPLES)),
          nrm(b.take<pr_vec3>(PR_PLANE_MAX_SAMPLES)), support(b.take<uint32_t>(own_support ? (size_t)n_planes * PR_PLANE_MAX_CANDIDATES : 0)) {}
};
// pr_scene_segments_dev: control words | the records | the rank table | the qualifying roots | chunk counts and offsets | the forest | the per-root counts (by the word)
struct SegBlock {
    Block b;
    size_t ctl, acc, rank, roots, chunks, parent, count;
    SegBlock(uint32_t max_segments, uint32_t n_chunks, uint32_t n_px)
        : ctl(b.take<prk::SegControl>(1)), acc(b.take<segments::Acc>(max_segments)), rank(b.take<uint16_t>(PR_SEGMENT_MAX_ROOTS)), roots(b.take<prk::SegRoot>(PR_SEGMENT_MAX_ROOTS)),
          chunks(b.take<uint32_t>(ScanRows::words(n_chunks))), parent(b.take<uint32_t>(n_px)), count(b.take<uint32_t>(n_px, sizeof(uint32_t))) {}
};
// ... and the pinned block of a call: the control words and the roots behind them (one copy of the compaction) | the rank table | the records
struct SegPinned {
    Block b;
    size_t ctl = b.take<prk::SegControl>(1), roots = b.take<prk::SegRoot>(PR_SEGMENT_MAX_ROOTS), rank = b.take<uint16_t>(PR_SEGMENT_MAX_ROOTS), acc = b.take<segments::Acc>(PR_SEGMENT_MAX);
};
// pr_ppf_vote (n_models = 0: no table) and pr_ppf_vote_multi, the device block and its pinned twin: the model records (staged to the device) |
// the peaks of all models | the references (both read back: back_words() 32-bit words from `peaks` on)
struct VoteBlock {
    Block b;
    size_t models, peaks, refs;
    VoteBlock(uint32_t n_models, uint32_t n_refs, uint32_t n_peaks)
        : models(b.take<prk::PpfModelRec>(n_models)), peaks(b.take<pr_ppf_peak>((size_t)n_refs * n_peaks * (n_models ? n_models : 1))), refs(b.take<prk::PpfRef>(n_refs)) {}
    uint32_t back_words() const { return (uint32_t)((b.bytes() - peaks) / sizeof(uint32_t)); }
};

}  // namespace prr
