// verify.hip -- render-and-compare scoring: the depth boxes of a rendered batch (launch_render_boxes) against one scene depth frame, integer counts per hypothesis
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "score_walk.h"

namespace prk {

// One workgroup = 16 image rows of one hypothesis' box (count_box_kernel's shape: 4 wavefronts x 4 rows, lanes along a row).  A box pixel holds
// the rendered depth r (INT_MAX where nothing was drawn); the frame pixel is (x, row) exactly as d2c_emit_box_kernel maps it, and the scene
// value s is read from the same frame pixel (the frame stays in L2 / MALL, shared by every hypothesis).  Counts per lane in registers, summed
// over the workgroup (block_totals), then one integer atomic per counter and workgroup: the records are exact and reproducible.
// abs_err: a lane sees at most 4 rows x 128 columns (frames <= 8192 wide) of |r - s| <= tau < 2^31, so its sum is < 2^40 and is reduced as a
// 24-bit low part and a high part, each of which stays below 2^32 over the 256 lanes.
template <typename SceneT>
__global__ __launch_bounds__(256) void score_box_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                        const uint32_t *__restrict__ box_off, const SceneT *__restrict__ scene, int32_t tau,
                                                        uint32_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x & 63;
    BoxBlock blk;
    if (!box_block(bbox, height, blk)) return;
    const auto [bb, r_lo, r_hi, row0] = blk;
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
                if (!rendered(d)) continue;
                const uint32_t c = depth_class(d, s, t);
                const int64_t diff = (int64_t)d - (int64_t)s;       // 64 bits: no overflow for any int32 pair
                ++vis;
                inl += c == 0; occ += c == 1; vio += c == 2; mis += c == 3;
                if (c == 0) err += (uint64_t)(diff < 0 ? -diff : diff);
            }
    }
    const uint32_t v[7] = { vis, inl, occ, vio, mis, (uint32_t)(err & 0xffffffu), (uint32_t)(err >> 24) };
    const uint32_t sum = block_totals(v);
    const uint32_t hi = __shfl_down(sum, 1);                        // thread 5: the low part is its own total, the high part thread 6's
    const uint32_t k = threadIdx.x;
    uint32_t *rec = records + (size_t)blockIdx.y * 8;
    if (k < 5) {
        if (sum) atomicAdd(rec + k, sum);
    } else if (k == 5) {
        const unsigned long long err_sum = (unsigned long long)sum + ((unsigned long long)hi << 24);
        if (err_sum) atomicAdd(reinterpret_cast<unsigned long long *>(rec + 6), err_sum);
    }
}

hipError_t launch_score_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height,
                              const void *scene, bool scene_i32, int32_t tau, uint32_t *records, hipStream_t s)
{
    return for_box_launches(depth, box_off, n_poses, width, height, scene, scene_i32, [&](const BoxLaunch &b, auto *sc) {
        hipLaunchKernelGGL(score_box_kernel, b.grid, dim3(256), 0, s, b.depth, bbox + b.p0, width, height, b.box_off, sc, tau, records + (size_t)b.p0 * 8);
    });
}

}  // namespace prk
