// verify.hip -- render-and-compare scoring: the depth boxes of a rendered batch (launch_render_boxes) against one scene depth frame, integer counts per hypothesis
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "pr_launch.h"

namespace prk {

// One workgroup = 16 image rows of one hypothesis' box (count_box_kernel's shape: 4 wavefronts x 4 rows, lanes along a row).  A box pixel holds
// the rendered depth r (INT_MAX where nothing was drawn); the frame pixel is (x, row) exactly as d2c_emit_box_kernel maps it, and the scene
// value s is read from the same frame pixel (the frame stays in L2 / MALL, shared by every hypothesis).  Counts per lane in registers, a wave
// sum, a sum over the four wavefronts in LDS, then one integer atomic per counter and workgroup: the records are exact and reproducible.
// abs_err: a lane sees at most 4 rows x 128 columns (frames <= 8192 wide) of |r - s| <= tau < 2^31, so its sum is < 2^40 and is reduced as a
// 24-bit low part and a high part, each of which stays below 2^32 over the 256 lanes.
template <typename SceneT>
__global__ __launch_bounds__(256) void score_box_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                        const uint32_t *__restrict__ box_off, const SceneT *__restrict__ scene, int32_t tau,
                                                        uint32_t *__restrict__ records)
{
    __shared__ uint32_t part[4][8];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int4 bb = bbox[blockIdx.y];
    const int r_lo = (int)height - 1 - bb.w, r_hi = (int)height - 1 - bb.y;            // image rows of the box (raster rows run flipped)
    const int blk0 = (int)(blockIdx.x * kBoxRowsPerBlock);
    if (bb.x > bb.z || r_lo > r_hi || blk0 > r_hi || blk0 + (int)kBoxRowsPerBlock - 1 < r_lo) return;     // the whole workgroup, before any barrier
    const uint32_t row0 = (uint32_t)blk0 + wave * 4;
    const int64_t t = tau;
    uint32_t vis = 0, inl = 0, occ = 0, vio = 0, mis = 0;
    uint64_t err = 0;
    for (int x0 = bb.x; x0 <= bb.z; x0 += 256) {
        int32_t rv[4][4], sv[4][4];                                 // 32 loads in flight per lane before the first compare
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t row = row0 + r;
            const bool live = row < height && (int)row >= r_lo && (int)row <= r_hi;
            const int32_t *line = live ? box_line(const_cast<int32_t *>(depth), box_off, bb, blockIdx.y, row, width, height) : depth;
            const SceneT *srow = scene + (live ? (size_t)row * width : 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + 64 * j + (int)lane;
                const bool in = live && x <= bb.z;
                rv[r][j] = in ? line[x] : 0;
                sv[r][j] = in ? (int32_t)srow[x] : 0;
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t d = rv[r][j], s = sv[r][j];
                if (!(d > 0 && d != INT_MAX)) continue;             // not rendered
                ++vis;
                if (s <= 0) { ++mis; continue; }
                const int64_t diff = (int64_t)d - (int64_t)s;       // 64 bits: no overflow for any int32 pair
                if (diff > t) ++occ;                                // s < r - tau
                else if (diff < -t) ++vio;                          // s > r + tau
                else { ++inl; err += (uint64_t)(diff < 0 ? -diff : diff); }
            }
    }
    const uint32_t v[7] = { vis, inl, occ, vio, mis, (uint32_t)(err & 0xffffffu), (uint32_t)(err >> 24) };
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const uint32_t w = wave_sum_u32(v[k]);
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const uint32_t k = threadIdx.x;
        uint32_t *rec = records + (size_t)blockIdx.y * 8;
        if (k < 5) {
            const uint32_t sum = part[0][k] + part[1][k] + part[2][k] + part[3][k];
            if (sum) atomicAdd(rec + k, sum);
        } else {
            const unsigned long long lo = (unsigned long long)part[0][5] + part[1][5] + part[2][5] + part[3][5];
            const unsigned long long hi = (unsigned long long)part[0][6] + part[1][6] + part[2][6] + part[3][6];
            const unsigned long long sum = lo + (hi << 24);
            if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(rec + 6), sum);
        }
    }
}

hipError_t launch_score_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height,
                              const void *scene, bool scene_i32, int32_t tau, uint32_t *records, hipStream_t s)
{
    for (uint32_t p0 = 0; p0 < n_poses; p0 += 32768) {                // grid.y is limited to 65535 (launch_render_boxes splits the same way)
        const uint32_t np = (n_poses - p0 < 32768) ? (n_poses - p0) : 32768;
        const int32_t *d = box_off ? depth : depth + (size_t)p0 * width * height;
        const uint32_t *bo = box_off ? box_off + p0 : nullptr;
        const dim3 grid((height + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock, np);
        if (scene_i32)
            hipLaunchKernelGGL(score_box_kernel<int32_t>, grid, dim3(256), 0, s, d, bbox + p0, width, height, bo, static_cast<const int32_t *>(scene), tau,
                               records + (size_t)p0 * 8);
        else
            hipLaunchKernelGGL(score_box_kernel<uint16_t>, grid, dim3(256), 0, s, d, bbox + p0, width, height, bo, static_cast<const uint16_t *>(scene), tau,
                               records + (size_t)p0 * 8);
    }
    return hipGetLastError();
}

}  // namespace prk
