// pr_reproject.cpp -- pr_reproject_describe / pr_depth_reproject_*: the rules of the parameters, the sources and the target (one copy for both entry
// points), the host twin over the shared definition of reproject.h, and the launches of reproject.hip
#include <vector>

#include "pr_runtime.h"
#include "frame_stage.h"
#include "depth_filter.h"
#include "reproject.h"

namespace prr {

// a parameter block as a caller hands it over: pr_reproject_describe's rules.  No HIP call in here.
static int reproject_params_ok(const char *fn, const pr_reproject_params *p)
{
    if (!p) { set_error("%s: null pr_reproject_params", fn); return PR_ERR_INVALID; }
    if (p->splat < 1 || p->splat > 3) { set_error("%s: pr_reproject_params: splat must be 1 .. 3 (got %u)", fn, p->splat); return PR_ERR_INVALID; }
    PR_TRY(gate_ok(fn, "pr_reproject_params", p->min_mm, p->max_mm, p->tol_mm, p->tol_permille));
    PR_TRY(window_ok(fn, "pr_reproject_params", "occl_radius", p->occl_radius, PR_REPROJECT_MAX_RADIUS, "occl_min_front", p->occl_min_front));
    if (p->reserved != 0) { set_error("%s: pr_reproject_params: reserved must be 0", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
static bool pinhole_ok(float fx, float fy, float cx, float cy) { return std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy) && fx > 0.0f && fy > 0.0f; }
static int reproject_args_ok(const char *fn, const pr_reproject_source *src, uint32_t n_sources, size_t W, size_t H, float fx, float fy, float cx, float cy,
                             const pr_reproject_params *p, const void *out)
{
    PR_TRY(reproject_params_ok(fn, p));
    if (!src || !out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (n_sources == 0 || n_sources > PR_REPROJECT_MAX_SOURCES) { set_error("%s: n_sources must be 1 .. PR_REPROJECT_MAX_SOURCES = %d (got %u)", fn, PR_REPROJECT_MAX_SOURCES, n_sources); return PR_ERR_INVALID; }
    PR_TRY(depth_frame_ok(fn, "the target", W, H));
    if (!pinhole_ok(fx, fy, cx, cy)) { set_error("%s: the target's intrinsics must be finite with fx, fy > 0", fn); return PR_ERR_INVALID; }
    for (uint32_t i = 0; i < n_sources; ++i) {
        const pr_reproject_source &s = src[i];
        if (!s.data) { set_error("%s: sources[%u].data is null", fn, i); return PR_ERR_INVALID; }
        if (s.data == out) { set_error("%s: depth_out must not be sources[%u].data", fn, i); return PR_ERR_INVALID; }
        if (s.reserved != 0) { set_error("%s: sources[%u].reserved must be 0", fn, i); return PR_ERR_INVALID; }
        const uintptr_t at = reinterpret_cast<uintptr_t>(s.data);
        if (s.kind == PR_SRC_DEPTH_U16 || s.kind == PR_SRC_DEPTH_I32) {
            char what[40];
            std::snprintf(what, sizeof what, "sources[%u]: a frame", i);
            PR_TRY(depth_frame_ok(fn, what, s.width, s.height));
            if (s.n_points != 0) { set_error("%s: sources[%u]: n_points of a frame must be 0", fn, i); return PR_ERR_INVALID; }
            if (!pinhole_ok(s.fx, s.fy, s.cx, s.cy)) { set_error("%s: sources[%u]: the intrinsics must be finite with fx, fy > 0", fn, i); return PR_ERR_INVALID; }
            if (at % depth_bytes(s.kind == PR_SRC_DEPTH_I32)) { set_error("%s: sources[%u].data is not aligned to its element", fn, i); return PR_ERR_INVALID; }
        } else if (s.kind == PR_SRC_CLOUD) {
            if (s.n_points == 0 || s.n_points > ((uint64_t)1 << 26)) { set_error("%s: sources[%u]: a cloud holds 1 .. 2^26 points (got %llu)", fn, i, (unsigned long long)s.n_points); return PR_ERR_INVALID; }
            if (at % 4u) { set_error("%s: sources[%u].data is not aligned to its element", fn, i); return PR_ERR_INVALID; }
        } else { set_error("%s: sources[%u].kind = %u is not a PR_SRC_* value", fn, i, s.kind); return PR_ERR_INVALID; }
        for (int k = 0; k < 16; ++k) if (!std::isfinite(s.T[k])) { set_error("%s: sources[%u].T is not finite", fn, i); return PR_ERR_INVALID; }
        if (s.T[12] != 0.0f || s.T[13] != 0.0f || s.T[14] != 0.0f || s.T[15] != 1.0f) { set_error("%s: the last row of sources[%u].T must be (0, 0, 0, 1)", fn, i); return PR_ERR_INVALID; }
    }
    return PR_OK;
}
static rpj::Rigid rigid_of(const pr_reproject_source &s)
{
    rpj::Rigid T;
    for (int k = 0; k < 12; ++k) T.m[k] = s.T[k];
    return T;
}

// the host's scatter of one source into the key plane; n[]: its samples, invalid, range, outside
static void scatter_point(const rpj::Rigid &T, const rpj::Target &t, uint32_t source, float px, float py, float pz, std::vector<uint32_t> &keys, uint32_t (&n)[4])
{
    const rpj::Splat sp = rpj::project(T, t, px, py, pz);
    n[0]++;
    if (sp.code != rpj::kDrawn) { n[sp.code]++; return; }
    const uint32_t key = rpj::key_of(sp.d, source);
    for (int y = sp.y0; y < sp.y1; ++y)
        for (int x = sp.x0; x < sp.x1; ++x) { uint32_t &k = keys[(size_t)y * t.width + (size_t)x]; k = key < k ? key : k; }
}
template <class D>
static void scatter_frame_host(const D *d, const pr_reproject_source &s, uint32_t source, const rpj::Target &t, std::vector<uint32_t> &keys, uint32_t (&n)[4])
{
    const rpj::Rigid T = rigid_of(s);
    for (uint32_t y = 0; y < s.height; ++y)
        for (uint32_t x = 0; x < s.width; ++x) {
            const uint32_t d0 = dfilt::depth_of(d[(size_t)y * s.width + x]);
            if (d0 == 0u) continue;
            if (d0 > rpj::kMaxDepth) { n[0]++; n[rpj::kRange]++; continue; }
            float px, py, pz;
            rpj::frame_point(x, y, d0, s.fx, s.fy, s.cx, s.cy, px, py, pz);
            scatter_point(T, t, source, px, py, pz, keys, n);
        }
}
template <class O, int R>
static void resolve_host(const std::vector<uint32_t> &keys, uint32_t W, uint32_t H, const pr_reproject_params &p, O *out, uint8_t *source_out, pr_reproject_counts &c)
{
    const auto z_at = [&](int64_t x, int64_t y) { return (x < 0 || y < 0 || x >= (int64_t)W || y >= (int64_t)H) ? 0u : rpj::depth_of_key(keys[(size_t)y * W + (size_t)x]); };
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const uint32_t key = keys[i], z0 = rpj::depth_of_key(key);
            uint32_t o = 0u, s = PR_REPROJECT_NONE;
            if (z0 != 0u) {
                c.covered++;
                if (rpj::hidden<R>(p, z0, [&](int dx, int dy) { return z_at((int64_t)x + dx, (int64_t)y + dy); })) { s = PR_REPROJECT_HIDDEN; c.hidden++; }
                else { o = z0; s = key & 7u; c.kept++; c.source[s].won++; }
            }
            out[i] = (O)o;
            if (source_out) source_out[i] = (uint8_t)s;
        }
}

}  // namespace prr

using namespace prr;

extern "C" {

int pr_reproject_describe(uint32_t splat, uint32_t min_mm, uint32_t max_mm, uint32_t tol_mm, uint32_t tol_permille, uint32_t occl_radius, uint32_t occl_min_front,
                          pr_reproject_params *out)
{
    const char *fn = "pr_reproject_describe";
    if (!out) { set_error("%s: null out", fn); return PR_ERR_INVALID; }
    const pr_reproject_params p = { splat, min_mm, max_mm, tol_mm, tol_permille, occl_radius, occl_min_front, 0u };
    PR_TRY(reproject_params_ok(fn, &p));
    *out = p;
    return PR_OK;
}

int pr_depth_reproject_host(const pr_reproject_source *sources, uint32_t n_sources, size_t width, size_t height, float fx, float fy, float cx, float cy,
                            int depth_is_i32, const pr_reproject_params *params, void *depth_out, uint8_t *source_out, pr_reproject_counts *counts_out)
{
    PR_TRY(reproject_args_ok("pr_depth_reproject_host", sources, n_sources, width, height, fx, fy, cx, cy, params, depth_out));
    const uint32_t W = (uint32_t)width, H = (uint32_t)height;
    const rpj::Target t = rpj::make_target(W, H, fx, fy, cx, cy, depth_is_i32 != 0, *params);
    std::vector<uint32_t> keys((size_t)W * H, rpj::kNoKey);
    pr_reproject_counts c{};
    for (uint32_t i = 0; i < n_sources; ++i) {
        const pr_reproject_source &s = sources[i];
        uint32_t n[4] = { 0u, 0u, 0u, 0u };
        if (s.kind != PR_SRC_CLOUD) with_depth(s.data, s.kind == PR_SRC_DEPTH_I32, [&](auto *d) { scatter_frame_host(d, s, i, t, keys, n); });
        else {
            const pr_vec3 *pts = static_cast<const pr_vec3 *>(s.data);
            const rpj::Rigid T = rigid_of(s);
            for (uint64_t k = 0; k < s.n_points; ++k) scatter_point(T, t, i, pts[k].x, pts[k].y, pts[k].z, keys, n);
        }
        c.source[i].samples = n[0]; c.source[i].invalid = n[rpj::kInvalid]; c.source[i].range = n[rpj::kRange]; c.source[i].outside = n[rpj::kOutside];
        c.source[i].drawn = n[0] - n[1] - n[2] - n[3];
    }
    with_depth(depth_out, depth_is_i32 != 0, [&](auto *out) {
        using O = std::remove_pointer_t<decltype(out)>;
        if (params->occl_radius == 0) resolve_host<O, 0>(keys, W, H, *params, out, source_out, c);
        else if (params->occl_radius == 1) resolve_host<O, 1>(keys, W, H, *params, out, source_out, c);
        else resolve_host<O, 2>(keys, W, H, *params, out, source_out, c);
    });
    if (counts_out) *counts_out = c;
    return PR_OK;
}

int pr_depth_reproject_dev(const pr_reproject_source *sources, uint32_t n_sources, size_t width, size_t height, float fx, float fy, float cx, float cy,
                           int depth_is_i32, const pr_reproject_params *params, void *depth_out_dev, uint8_t *source_dev_out, pr_reproject_counts *counts_host)
{
    const char *fn = "pr_depth_reproject_dev";
    PR_TRY(reproject_args_ok(fn, sources, n_sources, width, height, fx, fy, cx, cy, params, depth_out_dev));      // every check before any device use
    PR_ENTER();
    const uint32_t W = (uint32_t)width, H = (uint32_t)height, n_px = W * H;
    const rpj::Target t = rpj::make_target(W, H, fx, fy, cx, cy, depth_is_i32 != 0, *params);
    prk::ReprojSources ss{};
    uint32_t blocks = 0;
    for (uint32_t i = 0; i < n_sources; ++i) {
        const pr_reproject_source &s = sources[i];
        prk::ReprojSource &d = ss.s[i];
        d.data = s.data; d.kind = s.kind; d.width = s.width;
        d.n = s.kind == PR_SRC_CLOUD ? (uint32_t)s.n_points : s.width * s.height;
        d.fx = s.fx; d.fy = s.fy; d.cx = s.cx; d.cy = s.cy; d.T = rigid_of(s);
        d.first_block = blocks;
        blocks += prk::reproject_blocks(s.kind, s.data, d.n);
    }
    for (uint32_t i = n_sources; i < rpj::kMaxSources; ++i) { ss.s[i] = ss.s[0]; ss.s[i].n = 0u; ss.s[i].first_block = blocks; }      // (not read: no workgroup is theirs)
    ss.n_sources = n_sources; ss.n_blocks = blocks;
    // one device block: the key plane | (on 256 bytes) the control words
    Block b;
    const size_t keys_at = b.take<uint32_t>(n_px), ctl_at = b.take<prk::ReprojControl>(1, 256);
    PR_TRY(g->reproj_tmp.ensure(b.bytes()));
    PR_TRY(g->h_reproj.ensure(sizeof(prk::ReprojControl)));
    uint32_t *keys = at<uint32_t>(g->reproj_tmp.p, keys_at);
    prk::ReprojControl *ctl = at<prk::ReprojControl>(g->reproj_tmp.p, ctl_at);
    g->h_reproj.as<prk::ReprojControl>()->done = 0u;             // (what an earlier call left there is not taken for this call's)
    note_write(depth_out_dev, (size_t)n_px * depth_bytes(depth_is_i32 != 0));
    if (source_dev_out) note_write(source_dev_out, n_px);
    HIP_TRY(prk::launch_reproject_clear(keys, n_px, ctl, g->stream));
    HIP_TRY(prk::launch_reproject_scatter(ss, t, keys, ctl, g->stream));
    HIP_TRY(prk::launch_reproject_resolve(keys, W, H, *params, depth_is_i32 != 0, depth_out_dev, source_dev_out, ctl, g->h_reproj.dev_as<prk::ReprojControl>(), g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    const prk::ReprojControl got = *g->h_reproj.as<prk::ReprojControl>();
    const uint32_t n_tiles = ((W + 63u) / 64u) * ((H + 15u) / 16u);
    if (got.done != n_tiles || got.covered != got.hidden + got.kept) {
        set_error("%s: %u of %u tiles reported, %u covered pixels against %u hidden and %u kept", fn, got.done, n_tiles, got.covered, got.hidden, got.kept); return PR_ERR_HIP;
    }
    if (counts_host) {
        pr_reproject_counts c{};
        for (uint32_t i = 0; i < n_sources; ++i) {
            c.source[i].samples = got.src[i][0]; c.source[i].invalid = got.src[i][rpj::kInvalid]; c.source[i].range = got.src[i][rpj::kRange]; c.source[i].outside = got.src[i][rpj::kOutside];
            c.source[i].drawn = got.src[i][0] - got.src[i][1] - got.src[i][2] - got.src[i][3];
            c.source[i].won = got.won[i];
        }
        c.covered = got.covered; c.hidden = got.hidden; c.kept = got.kept;
        *counts_host = c;
    }
    return PR_OK;
}

}  // extern "C"
