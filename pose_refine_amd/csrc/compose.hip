// compose.hip -- the accepted hypotheses of a frame taken together: which one is in front at every pixel, what each one keeps, what the set explains
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "score_walk.h"

namespace prk {

// A key is (uint64)depth << 32 | caller's index of the hypothesis, kComposeNoKey where nothing is drawn: the minimum over the hypotheses is the
// front depth, ties to the lower index.  The caller's index never exceeds 0xfffe (PR_COMPOSE_MAX_POSES), so the low word of kComposeNoKey is nobody's.
constexpr unsigned long long kComposeNoKey = ~0ull;
constexpr uint32_t kComposeCull = 256;                               // boxes tested against the tile per round: one per lane of the workgroup
constexpr uint32_t kComposeBatch = 4;                                // listed boxes whose pixels a lane requests before the first compare (x 4 rows)

// Key frame.  A GATHER: a workgroup owns a frame tile of 64 columns x 16 rows (4 wavefronts x 4 rows, lanes along a row: score_box_kernel's
// shape turned from a box to the frame) and is the only writer of its pixels, so there are no 64-bit atomics and the bytes do not depend on
// how the batch was cut into depth chunks.  Per round of 256 boxes of the chunk every lane tests one box against the tile and the hits are
// compacted into LDS (ballot, prefix by mbcnt, the four wavefronts' totals through LDS); every lane then takes the minimum key over the listed
// boxes at its own four pixels, kComposeBatch boxes' loads in flight together.  `first` (the call's first chunk): the result is stored as it
// is -- that launch initialises every pixel of the frame, the ones outside the window included; later chunks combine with what is there.
__global__ __launch_bounds__(256) void compose_tile_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, const uint32_t *__restrict__ box_off,
                                                           uint32_t n_boxes, uint32_t width, uint32_t height, int4 window,
                                                           const uint32_t *__restrict__ index_of, uint32_t index0, unsigned long long *__restrict__ keys, uint32_t first)
{
    __shared__ uint32_t list[kComposeCull];
    __shared__ uint32_t wave_hits[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx0 = (int)(blockIdx.x * 64), ty0 = (int)(blockIdx.y * kBoxRowsPerBlock);
    const int tx1 = min(tx0 + 63, (int)width - 1), ty1 = min(ty0 + (int)kBoxRowsPerBlock - 1, (int)height - 1);
    const int x = tx0 + (int)lane;
    const uint32_t row0 = (uint32_t)ty0 + wave * 4;
    unsigned long long best[4] = { kComposeNoKey, kComposeNoKey, kComposeNoKey, kComposeNoKey };
    for (uint32_t base = 0; base < n_boxes; base += kComposeCull) {
        const uint32_t cand = base + threadIdx.x;
        bool hit = false;
        if (cand < n_boxes) {
            const int4 bb = bbox[cand];
            const int r_lo = (int)height - 1 - bb.w, r_hi = (int)height - 1 - bb.y;    // image rows of the box (raster rows run flipped)
            hit = bb.x <= bb.z && r_lo <= r_hi && bb.x <= tx1 && bb.z >= tx0 && r_lo <= ty1 && r_hi >= ty0;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wave_hits[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) { const uint32_t c = wave_hits[w]; before += w < wave ? c : 0; total += c; }
        if (hit) list[before + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0))] = cand;
        __syncthreads();
        for (uint32_t k0 = 0; k0 < total; k0 += kComposeBatch) {
            int32_t d[kComposeBatch][4];
            uint32_t who[kComposeBatch];
#pragma unroll
            for (uint32_t u = 0; u < kComposeBatch; ++u) {
                const bool have = k0 + u < total;                     // the same for every lane of the workgroup
                const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[have ? k0 + u : k0]);
                const int4 bb = bbox[b];
                const int r_lo = (int)height - 1 - bb.w, r_hi = (int)height - 1 - bb.y;
                const bool in_x = have && x >= bb.x && x <= bb.z;
                who[u] = index_of ? index_of[b] : index0 + b;
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) {
                    const uint32_t row = row0 + r;
                    const bool in = in_x && row < height && (int)row >= r_lo && (int)row <= r_hi;
                    d[u][r] = in ? box_line(const_cast<int32_t *>(depth), box_off, bb, b, row, width, height)[x] : INT_MAX;
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kComposeBatch; ++u)
#pragma unroll
                for (uint32_t r = 0; r < 4; ++r) {
                    const int32_t v = d[u][r];
                    const unsigned long long key = rendered(v) ? ((unsigned long long)(uint32_t)v << 32 | who[u]) : kComposeNoKey;
                    best[r] = key < best[r] ? key : best[r];
                }
        }
        __syncthreads();                                              // every wavefront is done with the list before the next round overwrites it
    }
    if (x >= (int)width) return;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t row = row0 + r;
        if (row >= height) continue;
        const bool inside = x >= window.x && x <= window.z && (int)row >= window.y && (int)row <= window.w;
        unsigned long long *cell = keys + (size_t)row * width + (uint32_t)x;
        unsigned long long v = inside ? best[r] : kComposeNoKey;
        if (!first) { const unsigned long long old = *cell; v = old < v ? old : v; }
        *cell = v;
    }
}

// What every hypothesis keeps.  score_box_kernel's grid and shape over the boxes of ALL hypotheses of the call (blockIdx.y = position in the
// grouped batch): the key frame and the scene inside the box, a pixel counts when the key's index is this hypothesis' (the caller's index:
// index_of, or the position itself), by the four tests (depth_class).  Registers, block_totals, one integer atomic per counter
// and workgroup into records[8 * caller's index] (pr_pose_visible words: owned, owned_inlier, owned_occluded, owned_violation, owned_missing).
template <typename SceneT>
__global__ __launch_bounds__(256) void compose_count_kernel(const unsigned long long *__restrict__ keys, const int4 *__restrict__ bbox, const uint32_t *__restrict__ index_of,
                                                            uint32_t width, uint32_t height, const SceneT *__restrict__ scene, int32_t tau, uint32_t *__restrict__ records)
{
    const uint32_t lane = threadIdx.x & 63;
    BoxBlock blk;
    if (!box_block(bbox, height, blk) || blk.bb.x < 0 || blk.bb.z >= (int)width || blk.r_lo < 0) return;   // (this kernel reads the frame, not the box: clipped to it)
    const auto [bb, r_lo, r_hi, row0] = blk;
    const uint32_t me = index_of ? index_of[blockIdx.y] : blockIdx.y;
    const int64_t t = tau;
    uint32_t cnt[5] = { 0, 0, 0, 0, 0 };                              // owned, then its four classes
    for (int x0 = bb.x; x0 <= bb.z; x0 += 128) {
        unsigned long long kv[4][2];
        int32_t sv[4][2];                                           // 16 loads in flight per lane before the first compare
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t row = row0 + r;
            const bool live = row < height && (int)row >= r_lo && (int)row <= r_hi;
            const size_t line = live ? (size_t)row * width : 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int x = x0 + 64 * j + (int)lane;
                const bool in = live && x <= bb.z;
                kv[r][j] = in ? keys[line + (uint32_t)x] : kComposeNoKey;
                sv[r][j] = in ? (int32_t)scene[line + (uint32_t)x] : 0;
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if ((uint32_t)kv[r][j] != me) continue;               // somebody else's pixel, or nobody's
                const uint32_t c = depth_class((int32_t)(kv[r][j] >> 32), sv[r][j], t);
                ++cnt[0];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) cnt[1 + k] += c == k;
            }
    }
    const uint32_t sum = block_totals(cnt);
    if (sum) atomicAdd(records + (size_t)me * 8 + threadIdx.x, sum);      // (threads 0..4: the others' totals are 0)
}

// Labels, front depth and the frame record: one pass over the frame, a workgroup per 256 columns x kEmitRows rows, lanes along a row, the rows'
// loads in flight together.  frame[0..6] = window, measured, covered, explained, in_front, behind, unmeasured (pr_frame_explained), reduced
// like the counts above.
constexpr uint32_t kEmitRows = 4;
template <typename SceneT>
__global__ __launch_bounds__(256) void compose_emit_kernel(const unsigned long long *__restrict__ keys, uint32_t width, uint32_t height, int4 window,
                                                           const SceneT *__restrict__ scene, int32_t tau, uint16_t *__restrict__ labels, int32_t *__restrict__ depth_out,
                                                           uint32_t *__restrict__ frame)
{
    const int64_t t = tau;
    const uint32_t x = blockIdx.x * 256 + threadIdx.x;
    uint32_t cnt[7] = { 0, 0, 0, 0, 0, 0, 0 };
    unsigned long long kv[kEmitRows];
    int32_t sv[kEmitRows];
#pragma unroll
    for (uint32_t r = 0; r < kEmitRows; ++r) {
        const uint32_t row = blockIdx.y * kEmitRows + r;
        const bool in = x < width && row < height;
        const size_t i = in ? (size_t)row * width + x : 0;
        kv[r] = in ? keys[i] : kComposeNoKey;
        sv[r] = in ? (int32_t)scene[i] : 0;
    }
#pragma unroll
    for (uint32_t r = 0; r < kEmitRows; ++r) {
        const uint32_t row = blockIdx.y * kEmitRows + r;
        if (x >= width || row >= height) continue;
        const size_t i = (size_t)row * width + x;
        const unsigned long long key = kv[r];
        const int32_t s = sv[r];
        const bool inside = (int)x >= window.x && (int)x <= window.z && (int)row >= window.y && (int)row <= window.w;
        const bool drawn = key != kComposeNoKey;                      // only ever inside the window
        if (labels) labels[i] = drawn ? (uint16_t)(uint32_t)key : (uint16_t)PR_COMPOSE_NONE;
        if (depth_out) depth_out[i] = drawn ? (int32_t)(key >> 32) : 0;
        cnt[0] += inside;
        cnt[1] += inside && s > 0;
        if (drawn) {
            const uint32_t c = depth_class((int32_t)(key >> 32), s, t);
            cnt[2] += 1;
            cnt[3] += c == 0;                                         // explained
            cnt[4] += c == 2;                                         // in_front: the composite lies before the measurement by more than tau (`violation`)
            cnt[5] += c == 1;                                         // behind: it lies behind it by more than tau (`occluded`)
            cnt[6] += c == 3;                                         // unmeasured
        }
    }
    const uint32_t sum = block_totals(cnt);
    if (sum) atomicAdd(frame + threadIdx.x, sum);                     // (threads 0..6: the others' totals are 0)
}

hipError_t launch_compose_tiles(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height, int4 window,
                                const uint32_t *index_of, uint32_t index0, unsigned long long *keys, bool first, hipStream_t s)
{
    const dim3 grid((width + 63) / 64, (height + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock);
    hipLaunchKernelGGL(compose_tile_kernel, grid, dim3(256), 0, s, depth, bbox, box_off, n_poses, width, height, window, index_of, index0, keys, first ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_compose_counts(const unsigned long long *keys, const int4 *bbox, const uint32_t *index_of, uint32_t n_poses, uint32_t width, uint32_t height,
                                 const void *scene, bool scene_i32, int32_t tau, uint32_t *records, hipStream_t s)
{
    if (n_poses == 0 || n_poses > PR_COMPOSE_MAX_POSES) return n_poses ? hipErrorInvalidValue : hipSuccess;      // grid.y is limited to 65535: one launch
    const dim3 grid((height + kBoxRowsPerBlock - 1) / kBoxRowsPerBlock, n_poses);
    with_scene(scene, scene_i32, [&](auto *sc) { hipLaunchKernelGGL(compose_count_kernel, grid, dim3(256), 0, s, keys, bbox, index_of, width, height, sc, tau, records); });
    return hipGetLastError();
}

hipError_t launch_compose_emit(const unsigned long long *keys, uint32_t width, uint32_t height, int4 window, const void *scene, bool scene_i32, int32_t tau,
                               uint16_t *labels, int32_t *depth_out, uint32_t *frame, hipStream_t s)
{
    const dim3 grid((width + 255) / 256, (height + kEmitRows - 1) / kEmitRows);
    with_scene(scene, scene_i32, [&](auto *sc) { hipLaunchKernelGGL(compose_emit_kernel, grid, dim3(256), 0, s, keys, width, height, window, sc, tau, labels, depth_out, frame); });
    return hipGetLastError();
}

}  // namespace prk
