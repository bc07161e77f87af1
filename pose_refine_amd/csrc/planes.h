// planes.h -- support planes of a depth frame: THE definition of sample, support test, moment grid and label (include/pose_refine.h states it in
// words), one copy for the kernels of planes.hip and the host twin of pr_planes.cpp, and the launchers of planes.hip.  float32, no contraction
// (-ffp-contract=off), + - * only per sample; the moments are integers: device and host agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "pr_internal.h"

#if defined(__HIP__)
#define PLANE_FN __host__ __device__ __forceinline__
#else
#define PLANE_FN inline
#endif

namespace planes {

static_assert(sizeof(pr_plane_params) == 32 && sizeof(pr_plane) == 48, "pr_plane_params / pr_plane layout");

PLANE_FN float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
PLANE_FN bool has_normal(float nx, float ny, float nz) { return nx != 0.0f || ny != 0.0f || nz != 0.0f; }
// pixel px of the dense arrays is a sample (on the stride grid: the caller's business)
PLANE_FN bool sample_keep(const float *pcd, const float *normal, size_t px)
{
    const float z = pcd[px * 3 + 2];
    return has_normal(normal[px * 3], normal[px * 3 + 1], normal[px * 3 + 2]) && z > 0.0f && z * 1000.0f <= 65535.0f;
}
PLANE_FN bool normal_agrees(float cos_min, float ax, float ay, float az, float bx, float by, float bz)
{
    return cos_min == -2.0f || dot3(ax, ay, az, bx, by, bz) >= cos_min;
}
// sample (p, m) supports the plane through pc with normal nc
PLANE_FN bool supports(float tau_mm, float cos_min, float pcx, float pcy, float pcz, float ncx, float ncy, float ncz, float px, float py, float pz,
                       float mx, float my, float mz)
{
    const float r = dot3(ncx, ncy, ncz, px - pcx, py - pcy, pz - pcz);
    return fabsf(r) <= tau_mm && normal_agrees(cos_min, ncx, ncy, ncz, mx, my, mz);
}
// a coordinate on the 1/16 mm grid of the moments (a value no int64 holds: 0)
PLANE_FN int64_t quantise(float coord_mm)
{
    const double q = rint((double)coord_mm * 16.0);
    return (q > -9.0e18 && q < 9.0e18) ? (int64_t)q : (int64_t)0;
}
// the ten moments of one point, in pr_scene_planes_dev's order: n, x, y, z, xx, xy, xz, yy, yz, zz (unsigned: sums wrap the same way everywhere)
PLANE_FN void point_moments(float x, float y, float z, uint64_t m[10])
{
    const uint64_t qx = (uint64_t)quantise(x), qy = (uint64_t)quantise(y), qz = (uint64_t)quantise(z);
    m[0] = 1; m[1] = qx; m[2] = qy; m[3] = qz;
    m[4] = qx * qx; m[5] = qx * qy; m[6] = qx * qz; m[7] = qy * qy; m[8] = qy * qz; m[9] = qz * qz;
}
// the label a pixel WITHOUT one takes in round k (1-based) against the fitted plane (n, offset), or 0; p in metres as the scene holds it
PLANE_FN uint8_t pixel_label(const pr_plane_params &pp, uint32_t k, float nx, float ny, float nz, float offset, float px_m, float py_m, float pz_m,
                             float mx, float my, float mz)
{
    const float h = dot3(nx, ny, nz, px_m * 1000.0f, py_m * 1000.0f, pz_m * 1000.0f) - offset;
    if (fabsf(h) <= pp.label_tau_mm && (!has_normal(mx, my, mz) || normal_agrees(pp.cos_min, nx, ny, nz, mx, my, mz))) return (uint8_t)k;
    if (k == 1 && pp.drop_behind && h < -pp.label_tau_mm) return (uint8_t)PR_PLANE_BEHIND;
    return 0;
}
// the winner's key: support in the high word, the candidate's index inverted in the low one (the largest key = most support, then lowest index)
PLANE_FN uint64_t winner_key(uint32_t support, uint32_t cand) { return ((uint64_t)support << 32) | (uint64_t)(0xFFFFFFFFu - cand); }

}  // namespace planes

namespace prk {

// one round of the peel as the device leaves it (read back whole): the winner's key, its inliers' moments, what the label pass changed
struct PlaneRound { uint64_t key; uint64_t m[10]; uint32_t labelled, behind; uint64_t pad[2]; };
static_assert(sizeof(PlaneRound) == 112 && sizeof(PlaneRound) % 16 == 0, "PlaneRound: whole 16-byte words");
struct PlaneSample { float x, y, z; uint32_t px; };       // mm, and the pixel it came from
static_assert(sizeof(PlaneSample) == 16, "PlaneSample: one 16-byte word");

// planes.hip.  gh = ceil(height / stride) sampled rows: row_count[gh], row_off[gh + 1] (the last word: the total)
hipError_t launch_plane_sample_count(const float *pcd, const float *normal, uint32_t width, uint32_t height, uint32_t stride, uint32_t *row_count,
                                     uint32_t *row_off, hipStream_t s);
hipError_t launch_plane_sample_emit(const float *pcd, const float *normal, uint32_t width, uint32_t height, uint32_t stride, const uint32_t *row_off,
                                    PlaneSample *points, pr_vec3 *normals, hipStream_t s);
// labels = no depth / 0 over the frame, the rounds' records and the support table zeroed
hipError_t launch_plane_init(const float *pcd, uint32_t n_px, uint8_t *labels, PlaneRound *rounds, uint32_t n_rounds, uint32_t *support, uint32_t n_support,
                             hipStream_t s);
// one round up to its record: support[n_cand] (zero on entry) counted, the winner's key, the winner's moments (none when no candidate has support);
// a sample is alive while its pixel's label is 0
hipError_t launch_plane_round(const pr_plane_params &pp, const PlaneSample *points, const pr_vec3 *normals, uint32_t n, uint32_t n_cand, const uint8_t *labels,
                              uint32_t n_cus, uint32_t *support, PlaneRound *round, hipStream_t s);
hipError_t launch_plane_label(const pr_plane_params &pp, uint32_t k, const float plane[4], const float *pcd, const float *normal, uint32_t n_px, uint8_t *labels,
                              PlaneRound *round, hipStream_t s);
hipError_t launch_plane_clear_depth(const uint8_t *labels, const void *depth_in, void *depth_out, bool depth_i32, uint32_t n_px, hipStream_t s);

}  // namespace prk
