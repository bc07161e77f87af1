// pr_segments.cpp -- pr_segment_* / pr_scene_segments_*: the parameters, the order and the rank table (one copy for both forms), the host twin
// of the labelling and the launches of segments.hip
#include <vector>

#include "pr_runtime.h"
#include "frame_stage.h"
#include "segments.h"

namespace prr {

// a parameter block as a caller hands it over: pr_segment_describe's rules.  No HIP call in here.
static int segment_params_ok(const char *fn, const pr_segment_params *sp)
{
    if (!sp) { set_error("%s: null pr_segment_params", fn); return PR_ERR_INVALID; }
    if (sp->jump_mm > 0x7FFFFFFFu) { set_error("%s: pr_segment_params: jump_mm must not exceed 2^31 - 1 (got %u)", fn, sp->jump_mm); return PR_ERR_INVALID; }
    if (sp->min_pixels == 0) { set_error("%s: pr_segment_params: min_pixels must not be 0", fn); return PR_ERR_INVALID; }
    if (sp->max_segments == 0 || sp->max_segments > PR_SEGMENT_MAX) { set_error("%s: pr_segment_params: max_segments must be 1 .. PR_SEGMENT_MAX = %d (got %u)", fn, PR_SEGMENT_MAX, sp->max_segments); return PR_ERR_INVALID; }
    if (sp->reserved != 0) { set_error("%s: pr_segment_params: reserved must be 0", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
static int segment_cap_ok(const char *fn, uint32_t n_qualifying, uint32_t min_pixels)
{
    if (n_qualifying > PR_SEGMENT_MAX_ROOTS) {
        set_error("%s: %u components of at least %u pixels, at most PR_SEGMENT_MAX_ROOTS = %d (raise min_pixels)", fn, n_qualifying, min_pixels, PR_SEGMENT_MAX_ROOTS); return PR_ERR_INVALID;
    }
    return PR_OK;
}
// The qualifying components (in root order) put in the order of the definition: order[rank] = position in the list, rank_label[position] = the label
// its pixels take.  Returns n_found.
static uint32_t rank_roots(const prk::SegRoot *list, uint32_t n, uint32_t max_segments, std::vector<uint32_t> &order, uint16_t *rank_label)
{
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n);          // (the keys are distinct: a root occurs once)
    for (uint32_t j = 0; j < n; ++j) keyed[j] = { segments::order_key(list[j].pixels, list[j].root), j };
    std::sort(keyed.begin(), keyed.end());
    order.resize(n);
    for (uint32_t rank = 0; rank < n; ++rank) order[rank] = keyed[rank].second;
    const uint32_t n_found = std::min(n, max_segments);
    for (uint32_t rank = 0; rank < n; ++rank) rank_label[order[rank]] = segments::label_of_rank(rank, n_found);
    return n_found;
}
struct PlainOp {
    void min32(uint32_t *p, uint32_t v) const { *p = std::min(*p, v); }
    void max32(uint32_t *p, uint32_t v) const { *p = std::max(*p, v); }
    void add32(uint32_t *p, uint32_t v) const { *p += v; }
    void add64(uint64_t *p, uint64_t v) const { *p += v; }
};

// the host's forest: the same rule (a link points to the lower index), one pixel after the other, with path halving
static uint32_t host_find(std::vector<uint32_t> &parent, uint32_t x)
{
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
}
static void host_union(std::vector<uint32_t> &parent, uint32_t a, uint32_t b)
{
    a = host_find(parent, a); b = host_find(parent, b);
    if (a == b) return;
    if (a < b) std::swap(a, b);
    parent[a] = b;
}
template <class T>
static int segments_host(const char *fn, const T *depth, uint32_t W, uint32_t H, const pr_segment_params &sp, uint16_t *labels_out, uint32_t *roots_out,
                         pr_segment *segments_out, uint32_t *n_found, uint32_t *n_qualifying, uint32_t *n_components)
{
    const uint32_t n_px = W * H;
    std::vector<uint32_t> parent(n_px), count(n_px, 0);
    for (uint32_t i = 0; i < n_px; ++i) parent[i] = segments::depth_of(depth[i]) ? i : segments::kNone;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t i = y * W + x, d = segments::depth_of(depth[i]);
            if (x > 0 && segments::linked(d, segments::depth_of(depth[i - 1]), sp.jump_mm)) host_union(parent, i, i - 1);
            if (y > 0 && segments::linked(d, segments::depth_of(depth[i - W]), sp.jump_mm)) host_union(parent, i, i - W);
        }
    for (uint32_t i = 0; i < n_px; ++i)
        if (parent[i] != segments::kNone) { parent[i] = host_find(parent, i); ++count[parent[i]]; }
    std::vector<prk::SegRoot> list;
    uint32_t n_comp = 0;
    for (uint32_t i = 0; i < n_px; ++i) {
        if (parent[i] != i) continue;
        ++n_comp;
        if (count[i] >= sp.min_pixels) list.push_back(prk::SegRoot{ i, count[i] });
    }
    const uint32_t nq = (uint32_t)list.size();
    PR_TRY(segment_cap_ok(fn, nq, sp.min_pixels));                  // nothing written before
    std::vector<uint32_t> order;
    std::vector<uint16_t> rank_label(nq);
    const uint32_t found = rank_roots(list.data(), nq, sp.max_segments, order, rank_label.data());
    for (uint32_t i = 0; i < n_px; ++i) if (parent[i] == i) count[i] = segments::kNone;       // count[root] becomes the root's position, as on the device
    for (uint32_t j = 0; j < nq; ++j) count[list[j].root] = j;
    std::vector<segments::Acc> acc(found, segments::acc_empty());
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t i = y * W + x, r = parent[i];
            if (roots_out) roots_out[i] = r;
            uint16_t lab = 0;
            if (r != segments::kNone) lab = count[r] == segments::kNone ? (uint16_t)PR_SEGMENT_DROPPED : rank_label[count[r]];
            labels_out[i] = lab;
            if (lab >= 1 && lab <= found) segments::acc_merge(&acc[lab - 1u], segments::part_of_pixel(x, y, segments::depth_of(depth[i])), PlainOp{});
        }
    for (uint32_t k = 0; k < found; ++k) segments_out[k] = segments::record(list[order[k]].root, acc[k]);
    *n_found = found;
    if (n_qualifying) *n_qualifying = nq;
    if (n_components) *n_components = n_comp;
    return PR_OK;
}

constexpr size_t kSegKeepBytes = 16 * ((PR_SEGMENT_MAX + 1 + 127) / 128);      // pr_segment_depth_dev's keep bits, whole 16-byte words (128 labels each)

}  // namespace prr

using namespace prr;

extern "C" {

int pr_segment_describe(uint32_t jump_mm, uint32_t min_pixels, uint32_t max_segments, pr_segment_params *out)
{
    const char *fn = "pr_segment_describe";
    if (!out) { set_error("%s: null out", fn); return PR_ERR_INVALID; }
    const pr_segment_params sp = { jump_mm, min_pixels, max_segments, 0u };
    PR_TRY(segment_params_ok(fn, &sp));
    *out = sp;
    return PR_OK;
}

int pr_scene_segments_host(const void *depth, int depth_is_i32, size_t width, size_t height, const pr_segment_params *params, uint16_t *labels_out,
                           uint32_t *roots_out, pr_segment *segments_out, uint32_t *n_found, uint32_t *n_qualifying, uint32_t *n_components)
{
    const char *fn = "pr_scene_segments_host";
    PR_TRY(segment_params_ok(fn, params));
    if (!depth || !labels_out || !segments_out || !n_found) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(depth_frame_ok(fn, "a frame", width, height));
    return with_depth(depth, depth_is_i32 != 0, [&](auto *d) {
        return segments_host(fn, d, (uint32_t)width, (uint32_t)height, *params, labels_out, roots_out, segments_out, n_found, n_qualifying, n_components);
    });
}

int pr_scene_segments_dev(const void *depth_dev, int depth_is_i32, size_t width, size_t height, const pr_segment_params *params, uint16_t *labels_dev_out,
                          uint32_t *roots_dev_out, pr_segment *segments_host, uint32_t *n_found, uint32_t *n_qualifying, uint32_t *n_components)
{
    const char *fn = "pr_scene_segments_dev";
    PR_TRY(segment_params_ok(fn, params));                          // every check before any device use
    if (!depth_dev || !labels_dev_out || !segments_host || !n_found) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(depth_frame_ok(fn, "a frame", width, height));
    PR_ENTER();
    const pr_segment_params sp = *params;
    const uint32_t W = (uint32_t)width, H = (uint32_t)height, n_px = W * H, n_chunks = (n_px + prk::kSegChunk - 1) / prk::kSegChunk;
    const bool i32 = depth_is_i32 != 0;
    const SegBlock l(sp.max_segments, n_chunks, n_px);
    const SegPinned pin;
    PR_TRY(g->seg_tmp.ensure(l.b.bytes()));
    PR_TRY(g->h_seg.ensure(pin.b.bytes()));
    void *d = g->seg_tmp.p, *hp = g->h_seg.p, *hd = g->h_seg.dev;
    prk::SegControl *ctl = at<prk::SegControl>(d, l.ctl);
    segments::Acc *acc = at<segments::Acc>(d, l.acc);
    uint16_t *rank_dev = at<uint16_t>(d, l.rank);
    prk::SegRoot *roots = at<prk::SegRoot>(d, l.roots);
    const ScanRows chunks(d, l.chunks, n_chunks);
    uint32_t *parent = at<uint32_t>(d, l.parent), *count = at<uint32_t>(d, l.count);

    HIP_TRY(prk::launch_segment_init(ctl, acc, sp.max_segments, g->stream));
    HIP_TRY(prk::launch_segment_tiles(depth_dev, i32, W, H, sp.jump_mm, parent, count, g->stream));
    HIP_TRY(prk::launch_segment_seams(depth_dev, i32, W, H, sp.jump_mm, parent, g->stream));
    HIP_TRY(prk::launch_segment_flatten(W, H, parent, count, g->stream));
    HIP_TRY(prk::launch_segment_compact(parent, count, n_px, sp.min_pixels, chunks.count, chunks.off, roots, ctl, hd, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    const prk::SegControl c = *at<prk::SegControl>(hp, pin.ctl);
    PR_TRY(segment_cap_ok(fn, c.n_qualifying, sp.min_pixels));      // nothing of the caller's written before
    const prk::SegRoot *list = at<prk::SegRoot>(hp, pin.roots);
    std::vector<uint32_t> order;
    const uint32_t found = rank_roots(list, c.n_qualifying, sp.max_segments, order, at<uint16_t>(hp, pin.rank));
    note_write(labels_dev_out, sizeof(uint16_t) * (size_t)n_px);
    if (roots_dev_out) note_write(roots_dev_out, sizeof(uint32_t) * (size_t)n_px);
    // (the same launches whatever the frame holds: at least one word of the table and one record travel)
    HIP_TRY(prk::launch_stage_words(at<unsigned char>(hd, pin.rank), rank_dev, std::max<size_t>(sizeof(uint16_t) * c.n_qualifying, 16), g->stream));
    HIP_TRY(prk::launch_segment_relabel(depth_dev, i32, W, H, parent, count, rank_dev, found, labels_dev_out, roots_dev_out, acc, g->stream));
    const uint32_t acc_words = (uint32_t)(sizeof(segments::Acc) / sizeof(uint32_t));
    HIP_TRY(prk::launch_copy_words32(acc, at<unsigned char>(hd, pin.acc), acc_words * std::max(found, 1u), g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    const segments::Acc *got = at<segments::Acc>(hp, pin.acc);
    for (uint32_t k = 0; k < found; ++k) {
        if (got[k].pixels != list[order[k]].pixels) { set_error("%s: segment %u gathered %u pixels, its component has %u", fn, k + 1, got[k].pixels, list[order[k]].pixels); return PR_ERR_HIP; }
        segments_host[k] = segments::record(list[order[k]].root, got[k]);
    }
    *n_found = found;
    if (n_qualifying) *n_qualifying = c.n_qualifying;
    if (n_components) *n_components = c.n_components;
    return PR_OK;
}

int pr_segment_depth_dev(const uint16_t *labels_dev, const void *depth_in_dev, int depth_is_i32, size_t n_px, const uint8_t *keep_host, uint32_t n_keep,
                         void *depth_out_dev)
{
    const char *fn = "pr_segment_depth_dev";
    if (!labels_dev || !depth_in_dev || !depth_out_dev || (n_keep && !keep_host)) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(depth_frame_ok(fn, n_px));
    if (n_keep > PR_SEGMENT_MAX + 1) { set_error("%s: n_keep must not exceed PR_SEGMENT_MAX + 1 = %d (got %u)", fn, PR_SEGMENT_MAX + 1, n_keep); return PR_ERR_INVALID; }
    PR_ENTER();
    PR_TRY(g->seg_tmp.ensure(kSegKeepBytes));
    PR_TRY(g->h_seg.ensure(SegPinned().b.bytes()));
    uint32_t *bits = g->h_seg.as<uint32_t>();
    std::memset(bits, 0, kSegKeepBytes);
    for (uint32_t k = 1; k < n_keep; ++k) if (keep_host[k]) bits[k >> 5] |= 1u << (k & 31u);      // label 0 is never kept
    HIP_TRY(prk::launch_stage_words(g->h_seg.dev, g->seg_tmp.p, kSegKeepBytes, g->stream));
    note_write(depth_out_dev, n_px * depth_bytes(depth_is_i32 != 0));
    HIP_TRY(prk::launch_segment_depth(labels_dev, depth_in_dev, depth_out_dev, depth_is_i32 != 0, (uint32_t)n_px, g->seg_tmp.as<uint32_t>(), n_keep, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

int pr_segment_roi(const pr_segment *segment, size_t width, size_t height, uint32_t margin, pr_roi *roi_out)
{
    const char *fn = "pr_segment_roi";
    if (!segment || !roi_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(depth_frame_ok(fn, "a frame", width, height));
    if (segment->x0 > segment->x1 || segment->y0 > segment->y1 || segment->x1 >= width || segment->y1 >= height) {
        set_error("%s: the box [%u, %u] x [%u, %u] does not lie in a %zux%zu frame", fn, segment->x0, segment->x1, segment->y0, segment->y1, width, height); return PR_ERR_INVALID;
    }
    const uint64_t m = margin;
    const uint64_t x0 = segment->x0 > m ? segment->x0 - m : 0, y0 = segment->y0 > m ? segment->y0 - m : 0;
    const uint64_t x1 = std::min<uint64_t>(segment->x1 + m, width - 1), y1 = std::min<uint64_t>(segment->y1 + m, height - 1);
    *roi_out = pr_roi{ (int)x0, (int)y0, (int)(x1 - x0 + 1), (int)(y1 - y0 + 1) };
    return PR_OK;
}

}  // extern "C"
