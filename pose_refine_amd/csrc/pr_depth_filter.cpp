// pr_depth_filter.cpp -- pr_depth_filter_* / pr_depth_fuse_*: the parameters' rules (one copy for every entry point), the host twins of the
// filter and the fuse over the shared definition of depth_filter.h, and the launches of depth_filter.hip
#include <vector>

#include "pr_runtime.h"
#include "frame_stage.h"
#include "depth_filter.h"

namespace prr {

// a parameter block as a caller hands it over: pr_depth_filter_describe's rules.  No HIP call in here.
static int filter_params_ok(const char *fn, const pr_depth_filter_params *p)
{
    if (!p) { set_error("%s: null pr_depth_filter_params", fn); return PR_ERR_INVALID; }
    PR_TRY(gate_ok(fn, "pr_depth_filter_params", p->min_mm, p->max_mm, p->tol_mm, p->tol_permille));
    if (p->fly_min_support > 8) { set_error("%s: pr_depth_filter_params: fly_min_support must be 0 .. 8 (got %u)", fn, p->fly_min_support); return PR_ERR_INVALID; }
    PR_TRY(window_ok(fn, "pr_depth_filter_params", "radius", p->radius, PR_DEPTH_FILTER_MAX_RADIUS, "fill_min", p->fill_min));
    if (p->reserved != 0) { set_error("%s: pr_depth_filter_params: reserved must be 0", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
static int filter_args_ok(const char *fn, const void *in, size_t W, size_t H, const pr_depth_filter_params *p, const void *out)
{
    PR_TRY(filter_params_ok(fn, p));
    if (!in || !out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (in == out) { set_error("%s: depth_out must not be depth_in (the filter is a stencil)", fn); return PR_ERR_INVALID; }
    return depth_frame_ok(fn, "a frame", W, H);
}
static int fuse_args_ok(const char *fn, const void *const *frames, uint32_t n_frames, size_t n_px, uint32_t min_frames, const void *out)
{
    if (!frames || !out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (n_frames == 0 || n_frames > PR_DEPTH_FUSE_MAX) { set_error("%s: n_frames must be 1 .. PR_DEPTH_FUSE_MAX = %d (got %u)", fn, PR_DEPTH_FUSE_MAX, n_frames); return PR_ERR_INVALID; }
    if (min_frames == 0 || min_frames > n_frames) { set_error("%s: min_frames must be 1 .. n_frames = %u (got %u)", fn, n_frames, min_frames); return PR_ERR_INVALID; }
    PR_TRY(depth_frame_ok(fn, n_px));
    for (uint32_t f = 0; f < n_frames; ++f) if (!frames[f]) { set_error("%s: frames[%u] is null", fn, f); return PR_ERR_INVALID; }
    return PR_OK;
}

// the host's filter: the stages one after the other over whole frames, each from the definition the kernel compiles
template <class T, int R>
static void filter_host(const T *in, uint32_t W, uint32_t H, const pr_depth_filter_params &p, T *out, uint8_t *flags, pr_depth_filter_counts *counts)
{
    const size_t n_px = (size_t)W * H;
    std::vector<uint32_t> G(n_px), F(n_px);
    for (size_t i = 0; i < n_px; ++i) G[i] = dfilt::gate(dfilt::depth_of(in[i]), p);
    const auto at = [&](const std::vector<uint32_t> &a, int64_t x, int64_t y) { return (x < 0 || y < 0 || x >= (int64_t)W || y >= (int64_t)H) ? 0u : a[(size_t)y * W + (size_t)x]; };
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) F[(size_t)y * W + x] = dfilt::flying(p, [&](int dx, int dy) { return at(G, (int64_t)x + dx, (int64_t)y + dy); });
    pr_depth_filter_counts c{};
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const dfilt::Out o = dfilt::pixel_out<R>(p, dfilt::depth_of(in[i]), G[i], [&](int dx, int dy) { return at(F, (int64_t)x + dx, (int64_t)y + dy); });
            out[i] = (T)o.depth;
            if (flags) flags[i] = (uint8_t)o.flag;
            c.n[o.flag]++;
        }
    if (counts) *counts = c;
}
template <class T>
static void filter_host_r(const T *in, uint32_t W, uint32_t H, const pr_depth_filter_params &p, T *out, uint8_t *flags, pr_depth_filter_counts *counts)
{
    if (p.radius == 0) filter_host<T, 0>(in, W, H, p, out, flags, counts);
    else if (p.radius == 1) filter_host<T, 1>(in, W, H, p, out, flags, counts);
    else filter_host<T, 2>(in, W, H, p, out, flags, counts);
}
template <class T>
static void fuse_host(const void *const *frames, uint32_t n_frames, size_t n_px, uint32_t min_frames, T *out, uint8_t *count_out)
{
    for (size_t i = 0; i < n_px; ++i) {                           // (out may be one of the frames: a pixel's values are read before it is written)
        uint32_t v[8], k;
        for (uint32_t f = 0; f < prk::kDepthFuseMax; ++f) v[f] = f < n_frames ? dfilt::depth_of(static_cast<const T *>(frames[f])[i]) : 0u;
        out[i] = (T)dfilt::fuse(v, min_frames, &k);
        if (count_out) count_out[i] = (uint8_t)k;
    }
}

}  // namespace prr

using namespace prr;

extern "C" {

int pr_depth_filter_describe(uint32_t min_mm, uint32_t max_mm, uint32_t tol_mm, uint32_t tol_permille, uint32_t fly_min_support, uint32_t radius,
                             uint32_t fill_min, pr_depth_filter_params *out)
{
    const char *fn = "pr_depth_filter_describe";
    if (!out) { set_error("%s: null out", fn); return PR_ERR_INVALID; }
    const pr_depth_filter_params p = { min_mm, max_mm, tol_mm, tol_permille, fly_min_support, radius, fill_min, 0u };
    PR_TRY(filter_params_ok(fn, &p));
    *out = p;
    return PR_OK;
}

int pr_depth_fuse_host(const void *const *frames, uint32_t n_frames, int depth_is_i32, size_t n_px, uint32_t min_frames, void *depth_out, uint8_t *count_out)
{
    PR_TRY(fuse_args_ok("pr_depth_fuse_host", frames, n_frames, n_px, min_frames, depth_out));
    with_depth(depth_out, depth_is_i32 != 0, [&](auto *out) { fuse_host(frames, n_frames, n_px, min_frames, out, count_out); });
    return PR_OK;
}

int pr_depth_fuse_dev(const void *const *frames, uint32_t n_frames, int depth_is_i32, size_t n_px, uint32_t min_frames, void *depth_out_dev, uint8_t *count_out_dev)
{
    const char *fn = "pr_depth_fuse_dev";
    PR_TRY(fuse_args_ok(fn, frames, n_frames, n_px, min_frames, depth_out_dev));      // every check before any device use
    PR_ENTER();
    prk::FuseFrames ff;
    for (uint32_t f = 0; f < prk::kDepthFuseMax; ++f) ff.p[f] = frames[f < n_frames ? f : 0];
    note_write(depth_out_dev, n_px * depth_bytes(depth_is_i32 != 0));
    if (count_out_dev) note_write(count_out_dev, n_px);
    HIP_TRY(prk::launch_depth_fuse(ff, n_frames, depth_is_i32 != 0, (uint32_t)n_px, min_frames, depth_out_dev, count_out_dev, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

int pr_depth_filter_host(const void *depth_in, int depth_is_i32, size_t width, size_t height, const pr_depth_filter_params *params, void *depth_out,
                         uint8_t *flags_out, pr_depth_filter_counts *counts_out)
{
    PR_TRY(filter_args_ok("pr_depth_filter_host", depth_in, width, height, params, depth_out));
    with_depth(depth_out, depth_is_i32 != 0, [&](auto *out) {
        using T = std::remove_pointer_t<decltype(out)>;
        filter_host_r(static_cast<const T *>(depth_in), (uint32_t)width, (uint32_t)height, *params, out, flags_out, counts_out);
    });
    return PR_OK;
}

int pr_depth_filter_dev(const void *depth_in_dev, int depth_is_i32, size_t width, size_t height, const pr_depth_filter_params *params, void *depth_out_dev,
                        uint8_t *flags_dev_out, pr_depth_filter_counts *counts_host)
{
    const char *fn = "pr_depth_filter_dev";
    PR_TRY(filter_args_ok(fn, depth_in_dev, width, height, params, depth_out_dev));      // every check before any device use
    PR_ENTER();
    const size_t n_px = width * height;
    PR_TRY(g->dfilt_tmp.ensure(sizeof(prk::FilterControl)));
    PR_TRY(g->h_dfilt.ensure(sizeof(prk::FilterControl)));
    prk::FilterControl *ctl = g->dfilt_tmp.as<prk::FilterControl>();
    note_write(depth_out_dev, n_px * depth_bytes(depth_is_i32 != 0));
    if (flags_dev_out) note_write(flags_dev_out, n_px);
    HIP_TRY(prk::launch_depth_filter_init(ctl, g->stream));
    HIP_TRY(prk::launch_depth_filter(depth_in_dev, depth_is_i32 != 0, (uint32_t)width, (uint32_t)height, *params, depth_out_dev, flags_dev_out, ctl, g->stream));
    HIP_TRY(prk::launch_copy_words32(ctl, g->h_dfilt.dev, (uint32_t)(sizeof(prk::FilterControl) / sizeof(uint32_t)), g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    const prk::FilterControl got = *g->h_dfilt.as<prk::FilterControl>();
    uint64_t sum = 0;
    for (uint32_t c = 0; c < 6; ++c) sum += got.n[c];
    if (sum != n_px) { set_error("%s: the flags of %llu pixels were counted, the frame has %zu", fn, (unsigned long long)sum, n_px); return PR_ERR_HIP; }
    if (counts_host) { for (uint32_t c = 0; c < 6; ++c) counts_host->n[c] = got.n[c]; counts_host->reserved[0] = counts_host->reserved[1] = 0; }
    return PR_OK;
}

}  // extern "C"
