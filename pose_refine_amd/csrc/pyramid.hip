// pyramid.hip -- coarse-to-fine refinement (pr_refine_pyramid): the strided clouds of every hypothesis, level by level, from the fused path's depth boxes
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
//
// The level cloud of stride s is the subsequence of the stride-1 cloud (d2c_emit_box_kernel: the rendered box pixels, row-major, back-projected at their
// FRAME coordinates) whose frame pixel satisfies x % s == 0 && row % s == 0.  Two kernels: one pass over the depth boxes counts the samples of every level
// per row (the depth is read once for all levels; the rows are scanned by d2c_scan_kernel like any other image), and one launch per level writes that
// level's clouds, lane k of a wavefront on the k-th SAMPLED pixel of a sampled row, each point moved by the hypothesis' accumulated transform on its way out.
#include "pr_launch.h"

namespace prk {

// row_count[(level * n_poses + hypothesis) * height + row] = samples of that level in that image row (0 outside the box and in rows the level skips).
// One wavefront per four image rows, as count_box_kernel: four loads in flight per lane before the first ballot.
__global__ __launch_bounds__(256) void pyramid_count_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                            const uint32_t *__restrict__ box_off, PyramidStrides lv, uint32_t n_poses,
                                                            uint32_t *__restrict__ row_count)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t pose = blockIdx.y;
    const int4 bb = bbox[pose];
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t row = blockIdx.x * kBoxRowsPerBlock + (threadIdx.x >> 6) * 4 + r;
        if (row >= height) return;
        const int ry = (int)height - 1 - (int)row;                  // raster row of this image row
        uint32_t sampled = 0;                                       // bit l: level l takes this row (wave-uniform)
#pragma unroll
        for (uint32_t l = 0; l < PR_PYRAMID_MAX_LEVELS; ++l) if (l < lv.n && row % lv.s[l] == 0) sampled |= 1u << l;
        uint32_t cnt[PR_PYRAMID_MAX_LEVELS];
#pragma unroll
        for (uint32_t l = 0; l < PR_PYRAMID_MAX_LEVELS; ++l) cnt[l] = 0;
        if (sampled && ry >= bb.y && ry <= bb.w) {
            const int32_t *line = box_line(const_cast<int32_t *>(depth), box_off, bb, pose, row, width, height);
            for (int x0 = bb.x; x0 <= bb.z; x0 += 256) {
                int32_t v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int x = x0 + 64 * j + (int)lane; v[j] = (x <= bb.z) ? line[x] : 0; }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t x = (uint32_t)(x0 + 64 * j) + lane;
                    const bool valid = v[j] > 0 && v[j] != INT_MAX;
#pragma unroll
                    for (uint32_t l = 0; l < PR_PYRAMID_MAX_LEVELS; ++l)
                        if (sampled >> l & 1u) cnt[l] += (uint32_t)__popcll(__ballot(valid && x % lv.s[l] == 0));
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (uint32_t l = 0; l < PR_PYRAMID_MAX_LEVELS; ++l)
                if (l < lv.n) row_count[((size_t)l * n_poses + pose) * height + row] = cnt[l];
        }
    }
}

// One level's clouds.  A workgroup takes kBoxRowsPerBlock SAMPLED rows of one hypothesis (sampled row j = image row j * stride), a wavefront four of them;
// lane k of a step holds the k-th multiple of `stride` at or behind the box's left edge, so every load is a pixel the level keeps.  The valid ones are
// compacted by ballot / popcount behind the row's offset (row-major order, as d2c_emit_box_kernel).  apply: the point goes through the carry's transform
// (levels behind the first: transform_pcd of the ORIGINAL point by the accumulated T, one rounding path).
__global__ __launch_bounds__(256) void pyramid_emit_kernel(const int32_t *__restrict__ depth, uint32_t width, uint32_t height, const int4 *__restrict__ bbox,
                                                           const uint32_t *__restrict__ box_off, float fx, float fy, float cx, float cy, uint32_t stride,
                                                           const uint32_t *__restrict__ row_count, const uint32_t *__restrict__ row_off,
                                                           const PyramidCarry *__restrict__ carry, uint32_t apply, pr_vec3 *__restrict__ cloud)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t pose = blockIdx.y;
    const int4 bb = bbox[pose];
    const PyramidCarry &pc = carry[pose];                        // uniform address: one 64-byte scalar load
    float M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = pc.T[i];
    const int xs0 = (int)(((uint32_t)bb.x + stride - 1) / stride * stride);      // first sampled column of the box (the box is clipped to the frame: bb.x >= 0)
    const int step = (int)(64u * stride);
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t row = (blockIdx.x * kBoxRowsPerBlock + (threadIdx.x >> 6) * 4 + r) * stride;
        if (row >= height) return;
        if (row_count[(size_t)pose * height + row] == 0) continue;  // also: every row outside the box
        const int32_t *line = box_line(const_cast<int32_t *>(depth), box_off, bb, pose, row, width, height);
        pr_vec3 *out = cloud + pc.start + row_off[(size_t)pose * height + row];
        uint32_t done = 0;
        for (int xb = xs0; xb <= bb.z; xb += PR_PYRAMID_EMIT_LOADS * step) {      // independent loads in flight per lane
            int32_t dv[PR_PYRAMID_EMIT_LOADS];
#pragma unroll
            for (int j = 0; j < PR_PYRAMID_EMIT_LOADS; ++j) { const int x = xb + j * step + (int)(lane * stride); dv[j] = (x <= bb.z) ? line[x] : 0; }
#pragma unroll
            for (int j = 0; j < PR_PYRAMID_EMIT_LOADS; ++j) {
                const int x = xb + j * step + (int)(lane * stride);
                const int32_t d = dv[j];
                const bool v = d > 0 && d != INT_MAX;
                const unsigned long long m = __ballot(v);
                if (v) {
                    const uint32_t k = done + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                    const pr_vec3 p = backproject_pixel(x, row, d, fx, fy, cx, cy);
                    out[k] = apply ? transform_point(M, p) : p;
                }
                done += (uint32_t)__popcll(m);
            }
        }
    }
}

hipError_t launch_pyramid_counts(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height,
                                 const PyramidStrides &lv, uint32_t *row_count, uint32_t *row_off, uint32_t *counts, hipStream_t s)
{
    if (n_poses == 0 || lv.n == 0) return hipSuccess;
    for (uint32_t p0 = 0; p0 < n_poses; p0 += 32768) {
        const uint32_t np = (n_poses - p0 < 32768) ? (n_poses - p0) : 32768;
        // (the level planes are n_poses * height apart: a piece writes its hypotheses' rows of every plane)
        hipLaunchKernelGGL(pyramid_count_kernel, dim3((height + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock, np), dim3(256), 0, s,
                           depth + (box_off ? 0 : (size_t)p0 * width * height), bbox + p0, width, height, box_off ? box_off + p0 : nullptr, lv, n_poses,
                           row_count + (size_t)p0 * height);
    }
    // every (level, hypothesis) is one image of `height` rows to the scan: offsets per row, counts[level * n_poses + hypothesis]
    for (uint32_t i0 = 0; i0 < lv.n * n_poses; i0 += 32768) {
        const uint32_t ni = (lv.n * n_poses - i0 < 32768) ? (lv.n * n_poses - i0) : 32768;
        const hipError_t e = launch_d2c_scan(row_count + (size_t)i0 * height, height, row_off + (size_t)i0 * height, counts + i0, ni, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

hipError_t launch_pyramid_emit(const int32_t *depth, uint32_t n_poses, uint32_t width, uint32_t height, const int4 *bbox, const uint32_t *box_off,
                               float fx, float fy, float cx, float cy, uint32_t stride, const uint32_t *row_count, const uint32_t *row_off,
                               const PyramidCarry *carry, bool apply, pr_vec3 *cloud, hipStream_t s)
{
    if (n_poses == 0 || stride == 0) return hipSuccess;
    const uint32_t gh = (height + stride - 1) / stride;              // sampled rows of a frame
    for (uint32_t p0 = 0; p0 < n_poses; p0 += 32768) {
        const uint32_t np = (n_poses - p0 < 32768) ? (n_poses - p0) : 32768;
        hipLaunchKernelGGL(pyramid_emit_kernel, dim3((gh + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock, np), dim3(256), 0, s,
                           depth + (box_off ? 0 : (size_t)p0 * width * height), width, height, bbox + p0, box_off ? box_off + p0 : nullptr, fx, fy, cx, cy, stride,
                           row_count + (size_t)p0 * height, row_off + (size_t)p0 * height, carry + p0, apply ? 1u : 0u, cloud);
    }
    return hipGetLastError();
}

}  // namespace prk
