// depth_filter.h -- depth conditioning of a frame: THE definition of a measured depth, the tolerance, the gate, the support test, the lower-median
// selection, a pixel's output and flag, and the per-pixel median over frames (include/pose_refine.h states them in words), one copy for the
// kernels of depth_filter.hip and the host twins of pr_depth_filter.cpp, and the launchers of depth_filter.hip.  Integers only: device and host
// agree bit for bit.
#pragma once
#include <stdint.h>

#include "pr_internal.h"

#if defined(__HIP__)
#define DF_FN __host__ __device__ __forceinline__
#define DF_UNROLL _Pragma("unroll")
#else
#define DF_FN inline
#define DF_UNROLL
#endif

namespace dfilt {

static_assert(sizeof(pr_depth_filter_params) == 32 && sizeof(pr_depth_filter_counts) == 32, "pr_depth_filter_params / pr_depth_filter_counts layout");

constexpr uint32_t kNone = 0xFFFFFFFFu;                          // a candidate that takes no part in a selection: above every depth (<= 2^31 - 1)

// a pixel's depth: 0 = not measured (a non-positive int32 included), else 1 .. 2^31 - 1
DF_FN uint32_t depth_of(uint16_t v) { return (uint32_t)v; }
DF_FN uint32_t depth_of(int32_t v) { return v > 0 ? (uint32_t)v : 0u; }
DF_FN uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
DF_FN uint32_t tol(uint32_t d, const pr_depth_filter_params &p) { return p.tol_mm + (uint32_t)((uint64_t)d * p.tol_permille / 1000u); }
DF_FN uint32_t gate(uint32_t d0, const pr_depth_filter_params &p) { return (d0 != 0u && d0 >= p.min_mm && (p.max_mm == 0u || d0 <= p.max_mm)) ? d0 : 0u; }
// a measured value q that lies within t of c
DF_FN bool supported(uint32_t q, uint32_t c, uint32_t t) { return q != 0u && absdiff(q, c) <= t; }

// F[p] from the gated depths around p.  g(dx, dy): G at that offset from p, 0 outside the frame.
template <class G>
DF_FN uint32_t flying(const pr_depth_filter_params &p, G g)
{
    const uint32_t g0 = g(0, 0);
    if (g0 == 0u || p.fly_min_support == 0u) return g0;
    const uint32_t t = tol(g0, p);
    uint32_t n = 0;
    DF_UNROLL
    for (int dy = -1; dy <= 1; ++dy) {
        DF_UNROLL
        for (int dx = -1; dx <= 1; ++dx)
            if (dx != 0 || dy != 0) n += supported(g(dx, dy), g0, t) ? 1u : 0u;
    }
    return n >= p.fly_min_support ? g0 : 0u;
}

// The lower median of the k candidates of v that are not kNone (k >= 1): candidate i's rank is the number of j with v_j < v_i, or v_j == v_i and
// j < i; the candidate of rank (k - 1) / 2 is taken.  Every pair is compared once and raises one of the two ranks.  Fully unrolled: no index
// depends on a run-time value, so v and the ranks stay in registers.
template <int N>
DF_FN uint32_t lower_median(const uint32_t (&v)[N], uint32_t k)
{
    uint32_t rank[N];
    DF_UNROLL
    for (int i = 0; i < N; ++i) rank[i] = 0;
    DF_UNROLL
    for (int i = 0; i < N; ++i) {
        DF_UNROLL
        for (int j = i + 1; j < N; ++j) {
            const uint32_t lt = v[j] < v[i] ? 1u : 0u;                // v_j < v_i: j goes before i; otherwise (v_i <= v_j, i < j) i goes before j
            rank[i] += lt; rank[j] += 1u - lt;
        }
    }
    const uint32_t want = (k - 1u) >> 1;
    uint32_t m = 0;
    DF_UNROLL
    for (int i = 0; i < N; ++i) m |= rank[i] == want ? v[i] : 0u;       // (the ranks are a permutation: one hit; a kNone ranks at k or above)
    return m;
}

struct Out { uint32_t depth, flag; };
// A pixel's output and flag from its raw depth d0, its gated depth g0 and the F values of its window.  R: the radius; f(dx, dy): F at that
// offset from the pixel, 0 outside the frame.  A measured pixel selects among the window's values within tol of its own, an unmeasured one
// among all of them: ONE selection with one of two masks.
template <int R, class F>
DF_FN Out pixel_out(const pr_depth_filter_params &p, uint32_t d0, uint32_t g0, F f)
{
    const uint32_t f0 = f(0, 0);
    if (d0 != 0u && g0 == 0u) return Out{ 0u, (uint32_t)PR_DEPTH_GATED };
    if (d0 != 0u && f0 == 0u) return Out{ 0u, (uint32_t)PR_DEPTH_FLYING };
    if (R == 0) return d0 != 0u ? Out{ f0, (uint32_t)PR_DEPTH_KEPT } : Out{ 0u, (uint32_t)PR_DEPTH_UNMEASURED };
    if (d0 == 0u && p.fill_min == 0u) return Out{ 0u, (uint32_t)PR_DEPTH_UNMEASURED };
    constexpr int S = 2 * R + 1, N = S * S;
    const bool own = d0 != 0u;
    const uint32_t t0 = own ? tol(f0, p) : 0u;
    uint32_t v[N], k = 0;
    DF_UNROLL
    for (int dy = -R; dy <= R; ++dy) {
        DF_UNROLL
        for (int dx = -R; dx <= R; ++dx) {
            const uint32_t q = f(dx, dy);
            const bool in = own ? supported(q, f0, t0) : q != 0u;
            v[(dy + R) * S + (dx + R)] = in ? q : kNone;
            k += in ? 1u : 0u;
        }
    }
    const uint32_t m = lower_median<N>(v, k);                      // (one call for both masks: the lanes of a wavefront do not take it twice; k == 0: no rank matches, m = 0)
    if (own) return Out{ m, m == d0 ? (uint32_t)PR_DEPTH_KEPT : (uint32_t)PR_DEPTH_SMOOTHED };      // (k >= 1: S holds F[p])
    if (k < p.fill_min) return Out{ 0u, (uint32_t)PR_DEPTH_UNMEASURED };      // (fill_min >= 1: k >= 1 below)
    const uint32_t tm = tol(m, p);
    uint32_t a = 0;
    DF_UNROLL
    for (int i = 0; i < N; ++i) a += (v[i] != kNone && absdiff(v[i], m) <= tm) ? 1u : 0u;
    return a >= p.fill_min ? Out{ m, (uint32_t)PR_DEPTH_FILLED } : Out{ 0u, (uint32_t)PR_DEPTH_UNMEASURED };
}

// ---- the median over frames --------------------------------------------------------------------------------------------------------------
DF_FN void cswap(uint32_t &a, uint32_t &b) { const uint32_t lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }
// eight values in ascending order: the 19-exchange network in six layers
DF_FN void sort8(uint32_t (&v)[8])
{
    cswap(v[0], v[2]); cswap(v[1], v[3]); cswap(v[4], v[6]); cswap(v[5], v[7]);
    cswap(v[0], v[4]); cswap(v[1], v[5]); cswap(v[2], v[6]); cswap(v[3], v[7]);
    cswap(v[0], v[1]); cswap(v[2], v[3]); cswap(v[4], v[5]); cswap(v[6], v[7]);
    cswap(v[2], v[4]); cswap(v[3], v[5]);
    cswap(v[1], v[4]); cswap(v[3], v[6]);
    cswap(v[1], v[2]); cswap(v[3], v[4]); cswap(v[5], v[6]);
}
// A pixel's fused depth from its eight slots (the D0 values of the frames; a slot beyond n_frames holds 0): the unmeasured ones go to the end
// of the order, the lower median of the rest is picked without indexing by a run-time value.  *count = the measured ones.
DF_FN uint32_t fuse(uint32_t (&v)[8], uint32_t min_frames, uint32_t *count)
{
    uint32_t k = 0;
    DF_UNROLL
    for (int i = 0; i < 8; ++i) { k += v[i] != 0u ? 1u : 0u; v[i] = v[i] != 0u ? v[i] : kNone; }
    *count = k;
    sort8(v);
    const uint32_t want = (k - 1u) >> 1;                           // (k == 0: no slot matches, and the test below gives 0 anyway)
    uint32_t m = 0;
    DF_UNROLL
    for (int i = 0; i < 8; ++i) m = (uint32_t)i == want ? v[i] : m;
    return (k >= min_frames && k != 0u) ? m : 0u;
}

}  // namespace dfilt

namespace prk {

constexpr uint32_t kDepthFuseMax = PR_DEPTH_FUSE_MAX;
struct FuseFrames { const void *p[kDepthFuseMax]; };              // the frames of a call, by value in the kernel's arguments (a slot beyond n_frames repeats frame 0 and is not read)
// the control words of a filter call as the device leaves them: the pixels per flag code
struct FilterControl { uint32_t n[6], pad[2]; };
static_assert(sizeof(FilterControl) == 32 && sizeof(FilterControl) == sizeof(pr_depth_filter_counts), "FilterControl: two 16-byte words, pr_depth_filter_counts' layout");

// depth_filter.hip
hipError_t launch_depth_filter_init(FilterControl *ctl, hipStream_t s);
// out, flags (may be null) and the counts added into ctl: one workgroup per 64 x 16 tile
hipError_t launch_depth_filter(const void *depth_in, bool depth_i32, uint32_t width, uint32_t height, const pr_depth_filter_params &params, void *depth_out,
                               uint8_t *flags, FilterControl *ctl, hipStream_t s);
// depth_out (may be one of the frames) and count_out (may be null) over n_px pixels
hipError_t launch_depth_fuse(const FuseFrames &frames, uint32_t n_frames, bool depth_i32, uint32_t n_px, uint32_t min_frames, void *depth_out, uint8_t *count_out,
                             hipStream_t s);

}  // namespace prk
