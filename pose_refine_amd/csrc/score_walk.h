// score_walk.h -- what the kernels of the scoring path share (verify.hip, select.hip, cover.hip, contour.hip, contour_fit.hip, normals.hip, compose.hip, vsd.hip and nobody else): the workgroup's
// part of a hypothesis' pixel box, the test of a rendered depth against the scene, the sum of a workgroup's counters, the launchers' loop
// gfx950 (CDNA4, wave64); integer arithmetic only, differences in 64 bits: every value is bit-identical to the CPU restatement.
#pragma once
#include "pr_launch.h"

namespace prk {

// ---- the box walk: one workgroup = kBoxRowsPerBlock image rows of the box of hypothesis blockIdx.y, 4 wavefronts x 4 rows, lanes along a row ----
struct BoxBlock { int4 bb; int r_lo, r_hi, row0; };                 // the pixel box, its image rows (raster rows run flipped), the first of this wavefront's four rows
// false: no row of the box in this workgroup -- the same for every thread, so the kernel returns before any barrier
__device__ __forceinline__ bool box_block(const int4 bb, uint32_t height, BoxBlock &b)
{
    b.bb = bb;
    b.r_lo = (int)height - 1 - b.bb.w; b.r_hi = (int)height - 1 - b.bb.y;
    const int blk0 = (int)(blockIdx.x * kBoxRowsPerBlock);
    b.row0 = blk0 + (int)(threadIdx.x >> 6) * 4;
    return !(b.bb.x > b.bb.z || b.r_lo > b.r_hi || blk0 > b.r_hi || blk0 + (int)kBoxRowsPerBlock - 1 < b.r_lo);
}
__device__ __forceinline__ bool box_block(const int4 *__restrict__ bbox, uint32_t height, BoxBlock &b) { return box_block(bbox[blockIdx.y], height, b); }

// ---- a pixel box in the words of a bit plane (select.hip's planes, cover.hip's claimed plane) ----
struct WordBox { int r0, r1, w0, w1; };                              // image rows and frame words of a pixel box; empty: r0 > r1
__device__ __forceinline__ WordBox word_box(const int4 bb, uint32_t height)
{
    WordBox b;
    b.r0 = (int)height - 1 - bb.w; b.r1 = (int)height - 1 - bb.y; b.w0 = bb.x >> 6; b.w1 = bb.z >> 6;
    if (bb.x > bb.z || bb.x < 0 || b.r0 < 0 || b.r1 >= (int)height) { b.r0 = 1; b.r1 = 0; }      // (boxes are clipped to the frame: the range tests never fire)
    return b;
}

// c / d for c * d < 2^32 by one multiply: fast_div_magic(d) = floor(2^32 / d) + 1 errs by less than c * d / 2^32 < 1 (d == 1: the quotient is c)
__device__ __forceinline__ uint32_t fast_div_magic(uint32_t d) { return d > 1 ? 0xffffffffu / d + 1u : 0u; }
__device__ __forceinline__ uint32_t fast_div(uint32_t c, uint32_t magic) { return magic ? __umulhi(c, magic) : c; }

// ---- the depth test: what an inlier is for the ranking, the selection, the contour gate, the normal agreement and the composition ----
__device__ __forceinline__ bool rendered(int32_t d) { return d > 0 && d != INT_MAX; }      // something was drawn here (INT_MAX: the render's background)
// the four tests of pr_pose_score for a rendered depth d against the scene value s: 0 inlier, 1 occluded (s < d - tau), 2 violation (s > d + tau), 3 missing
__device__ __forceinline__ uint32_t depth_class(int32_t d, int32_t s, int64_t tau)
{
    if (s <= 0) return 3;
    const int64_t diff = (int64_t)d - (int64_t)s;                     // 64 bits: no overflow for any int32 pair
    return diff > tau ? 1u : (diff < -tau ? 2u : 0u);
}

// ---- the edge rule of the contour check and the contour fit (contour.hip, contour_fit.hip), on normalised values: c > 0 is the pixel's depth; a
// neighbour is 0 when it is empty (no surface: infinitely far), its depth when it has one, and kNoNeighbour when it lies outside the image
// (ignored: an object cut by the border has no contour there).
constexpr int32_t kNoNeighbour = -1;
__device__ __forceinline__ bool edge_trigger(int32_t c, int32_t n, int64_t jump)
{
    return n == 0 || (n > 0 && (int64_t)n - (int64_t)c > jump);     // 64 bits: no overflow for any int32 pair
}

// ---- the reduction: N counters per lane -> a wave sum each, the four wavefronts' sums through LDS, one barrier.  Every thread of the 256-thread
// workgroup calls it; thread k < N gets the workgroup's total of counter k (the others 0) and does its own atomic with it.  Integer adds: exact in any order.
template <uint32_t N>
__device__ __forceinline__ uint32_t block_totals(const uint32_t (&v)[N])
{
    __shared__ uint32_t part[4][N];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
        const uint32_t w = wave_sum_u32(v[k]);
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
    const uint32_t k = threadIdx.x;
    return k < N ? part[0][k] + part[1][k] + part[2][k] + part[3][k] : 0u;
}

// ---- the launchers.  launch(scene) with the scene pointer as what it is: kernels templated on the scene type deduce it from the argument
template <typename Launch>
static inline void with_scene(const void *scene, bool scene_i32, Launch &&launch)
{
    if (scene_i32) launch(static_cast<const int32_t *>(scene));
    else launch(static_cast<const uint16_t *>(scene));
}
// The hypotheses of a rendered batch (launch_render_boxes' layout: full frames, or packed boxes with their offsets) in launches of at most 32768
// (grid.y is limited to 65535): launch(BoxLaunch, scene) for hypotheses p0 .. p0 + grid.y - 1; what else is per hypothesis the launcher offsets by p0 itself
struct BoxLaunch { uint32_t p0; dim3 grid; const int32_t *depth; const uint32_t *box_off; };
template <typename Launch>
static inline hipError_t for_box_launches(const int32_t *depth, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height,
                                          const void *scene, bool scene_i32, Launch &&launch)
{
    for (uint32_t p0 = 0; p0 < n_poses; p0 += 32768) {
        const uint32_t np = (n_poses - p0 < 32768) ? (n_poses - p0) : 32768;
        const BoxLaunch b{ p0, dim3((height + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock, np), box_off ? depth : depth + (size_t)p0 * width * height,
                           box_off ? box_off + p0 : nullptr };
        with_scene(scene, scene_i32, [&](auto *sc) { launch(b, sc); });
    }
    return hipGetLastError();
}

}  // namespace prk
