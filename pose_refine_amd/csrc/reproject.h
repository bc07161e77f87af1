// reproject.h -- z-buffered point reprojection: THE definition of a source's sample, the rigid transform, the depth, the footprint, the key and the
// visibility test (include/pose_refine.h states them in words), one copy for the kernels of reproject.hip and the host twin of pr_reproject.cpp,
// and the launchers of reproject.hip.  float32 without contraction and with the correctly rounded division up to the footprint, integers from
// there on: device and host agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pr_internal.h"

#if defined(__HIP__)
#define RP_FN __host__ __device__ __forceinline__
#define RP_UNROLL _Pragma("unroll")
#else
#define RP_FN inline
#define RP_UNROLL
#endif

namespace rpj {

static_assert(sizeof(pr_reproject_params) == 32 && sizeof(pr_reproject_source) == 112 && sizeof(pr_reproject_counts) == 288,
              "pr_reproject_params / pr_reproject_source / pr_reproject_counts layout");

constexpr uint32_t kMaxSources = PR_REPROJECT_MAX_SOURCES;
constexpr uint32_t kMaxDepth = (1u << 28) - 1u;                   // the largest depth a key holds: (d << 3) | source stays below 2^31
constexpr uint32_t kNoKey = 0xFFFFFFFFu;                          // a pixel no sample landed on: above every key
enum Outcome : uint32_t { kDrawn = 0, kInvalid = 1, kRange = 2, kOutside = 3 };

// the target of a call as every sample sees it: the frame, its pinhole, the depth gate [lo, hi] and the footprint
struct Target {
    uint32_t width, height;
    float fx, fy, cx, cy;
    uint32_t lo, hi;                                             // max(1, min_mm); the smallest of max_mm (when non-zero), 65535 for a uint16 output, 2^28 - 1
    uint32_t splat;                                              // 1 .. 3
    float h;                                                     // 0.5f * (float)(2 - splat): 0.5, 0 or -0.5
};
inline Target make_target(uint32_t width, uint32_t height, float fx, float fy, float cx, float cy, bool out_i32, const pr_reproject_params &p)
{
    Target t;
    t.width = width; t.height = height; t.fx = fx; t.fy = fy; t.cx = cx; t.cy = cy;
    t.lo = p.min_mm > 1u ? p.min_mm : 1u;
    t.hi = out_i32 ? kMaxDepth : 65535u;
    if (p.max_mm != 0u && p.max_mm < t.hi) t.hi = p.max_mm;
    t.splat = p.splat;
    t.h = 0.5f * (float)(2 - (int)p.splat);
    return t;
}

// a source's rigid transform: the first three rows of T
struct Rigid { float m[12]; };

RP_FN bool finite3(float x, float y, float z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }
RP_FN uint32_t tol(uint32_t d, const pr_reproject_params &p) { return p.tol_mm + (uint32_t)((uint64_t)d * p.tol_permille / 1000u); }

// pixel (x, y) of a frame source with depth D0 (1 .. 2^28 - 1) as a point of the source camera: backproject_pixel's expression
RP_FN void frame_point(uint32_t x, uint32_t y, uint32_t d0, float fx, float fy, float cx, float cy, float &px, float &py, float &pz)
{
    const float z = (float)d0 / 1000.0f;
    px = ((float)x - cx) / fx * z;
    py = ((float)y - cy) / fy * z;
    pz = z;
}

// what a sample writes: its depth and the clipped square x0 .. x1 - 1 by y0 .. y1 - 1 (not empty when code == kDrawn)
struct Splat { uint32_t code, d; int x0, y0, x1, y1; };

// a point p of a source, through the source's transform and the target's pinhole
RP_FN Splat project(const Rigid &T, const Target &t, float px, float py, float pz)
{
    Splat s{ kInvalid, 0u, 0, 0, 0, 0 };
    if (!finite3(px, py, pz)) return s;
    const float qx = ((T.m[0] * px + T.m[1] * py) + T.m[2] * pz) + T.m[3];
    const float qy = ((T.m[4] * px + T.m[5] * py) + T.m[6] * pz) + T.m[7];
    const float qz = ((T.m[8] * px + T.m[9] * py) + T.m[10] * pz) + T.m[11];
    if (!(finite3(qx, qy, qz) && qz > 0.0f)) return s;
    s.code = kRange;
    const float df = floorf(qz * 1000.0f + 0.5f);                  // an integer value, 0 or above, or +inf
    if (!(df < 2147483648.0f)) return s;
    const uint32_t d = (uint32_t)df;                               // exact: the gate compares integers
    if (d < t.lo || d > t.hi) return s;
    s.code = kOutside;
    const float u = qx / qz * t.fx + t.cx, v = qy / qz * t.fy + t.cy;
    const float x0f = floorf(u + t.h), y0f = floorf(v + t.h);
    if (!(x0f > -4.0f && x0f < (float)t.width && y0f > -4.0f && y0f < (float)t.height)) return s;      // (in float: a NaN fails)
    const int x0 = (int)x0f, y0 = (int)y0f, n = (int)t.splat;      // -3 .. width - 1, -3 .. height - 1
    s.x0 = x0 < 0 ? 0 : x0; s.y0 = y0 < 0 ? 0 : y0;
    s.x1 = x0 + n > (int)t.width ? (int)t.width : x0 + n;
    s.y1 = y0 + n > (int)t.height ? (int)t.height : y0 + n;
    if (s.x1 <= s.x0 || s.y1 <= s.y0) return s;
    s.code = kDrawn; s.d = d;
    return s;
}

RP_FN uint32_t key_of(uint32_t d, uint32_t source) { return (d << 3) | source; }
RP_FN uint32_t depth_of_key(uint32_t key) { return key == kNoKey ? 0u : key >> 3; }

// Is the measured pixel with depth z0 hidden?  R: the radius; z(dx, dy): Z at that offset from the pixel, 0 outside the frame.
template <int R, class Z>
RP_FN bool hidden(const pr_reproject_params &p, uint32_t z0, Z z)
{
    if (R == 0 || p.occl_min_front == 0u) return false;
    const uint32_t t0 = tol(z0, p);
    uint32_t front = 0;
    RP_UNROLL
    for (int dy = -R; dy <= R; ++dy) {
        RP_UNROLL
        for (int dx = -R; dx <= R; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const uint32_t q = z(dx, dy);
            front += (q != 0u && q + t0 < z0) ? 1u : 0u;             // (q < 2^28 and t0 < 2^31 + 2^28: no overflow)
        }
    }
    return front >= p.occl_min_front;
}

}  // namespace rpj

namespace prk {

// a source as the scatter kernel reads it, and the sources of a call: by value in the kernel's arguments
struct ReprojSource {
    const void *data;
    uint32_t kind, width;                                        // width: a frame's row length
    uint32_t n;                                                  // a frame's pixels or a cloud's points
    uint32_t first_block;                                        // the source's chunks are the workgroups first_block .. the next source's - 1
    float fx, fy, cx, cy;
    rpj::Rigid T;
};
struct ReprojSources { ReprojSource s[rpj::kMaxSources]; uint32_t n_sources, n_blocks; };
// the control words of a call as the device leaves them
struct ReprojControl {
    uint32_t src[rpj::kMaxSources][4];                           // per source: samples, invalid, range, outside
    uint32_t won[rpj::kMaxSources];
    uint32_t covered, hidden, kept, done;                        // done: the resolve tiles that have added their counts
    uint32_t pad[4];
};
static_assert(sizeof(ReprojControl) == 192, "ReprojControl: twelve 16-byte words");

constexpr uint32_t kReprojThreads = 256;
// the workgroups a source takes in the scatter launch
uint32_t reproject_blocks(uint32_t kind, const void *data, uint32_t n);

// reproject.hip
hipError_t launch_reproject_clear(uint32_t *keys, uint32_t n_px, ReprojControl *ctl, hipStream_t s);
hipError_t launch_reproject_scatter(const ReprojSources &src, const rpj::Target &target, uint32_t *keys, ReprojControl *ctl, hipStream_t s);
// out, the source image (may be null) and the frame's counts; the tile that finishes last copies the control words to ctl_out (pinned)
hipError_t launch_reproject_resolve(const uint32_t *keys, uint32_t width, uint32_t height, const pr_reproject_params &params, bool out_i32, void *depth_out,
                                    uint8_t *source_out, ReprojControl *ctl, ReprojControl *ctl_out, hipStream_t s);

}  // namespace prk
