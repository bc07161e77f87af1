// select.hip -- which hypotheses explain the same scene pixels: one bit plane of inlier pixels per hypothesis, then popcount(a & b) for every pair
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "score_walk.h"

namespace prk {

// Support bits.  score_box_kernel's shape (16 box rows per workgroup, 4 wavefronts x 4 rows, lanes along a row) and its inlier test, but the
// column loop starts at the 64-pixel boundary at or before the box, so one wavefront's ballot is one frame-aligned word: bit b of word w of
// image row y is frame pixel (64 w + b, y).  The plane of a hypothesis is dense (height x words_per_row words); only the words its box
// touches (rows r_lo..r_hi, words bb.x >> 6 .. bb.z >> 6) are written, each exactly once, by a plain store of the lane that owns the row,
// and only those are ever read (pair_overlap_kernel walks box intersections): no clearing pass, no atomics.  Pixels of a written word that
// lie outside the box are 0 in it.
template <typename SceneT>
__global__ __launch_bounds__(256) void support_bits_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                           const uint32_t *__restrict__ box_off, const SceneT *__restrict__ scene, int32_t tau,
                                                           unsigned long long *__restrict__ planes, uint32_t words_per_row)
{
    const uint32_t lane = threadIdx.x & 63;
    BoxBlock blk;
    if (!box_block(bbox, height, blk)) return;
    const auto [bb, r_lo, r_hi, row0] = blk;
    unsigned long long *plane = planes + (size_t)blockIdx.y * height * words_per_row;
    const int64_t t = tau;
    const int32_t *line[4];
    const SceneT *srow[4];
    bool live[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t row = row0 + r;
        live[r] = row < height && (int)row >= r_lo && (int)row <= r_hi;                // the same for every lane of the wavefront
        line[r] = live[r] ? box_line(const_cast<int32_t *>(depth), box_off, bb, blockIdx.y, row, width, height) : depth;
        srow[r] = scene + (live[r] ? (size_t)row * width : 0);
    }
    const bool my_live = lane < 4 && row0 + lane < height && (int)(row0 + lane) >= r_lo && (int)(row0 + lane) <= r_hi;
    for (int x0 = bb.x & ~63; x0 <= bb.z; x0 += 64) {
        const int x = x0 + (int)lane;
        const bool in_x = x >= bb.x && x <= bb.z;
        int32_t rv[4], sv[4];                                       // 8 loads in flight per lane before the first compare
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const bool in = live[r] && in_x;
            rv[r] = in ? line[r][x] : 0;
            sv[r] = in ? (int32_t)srow[r][x] : 0;
        }
        unsigned long long mine = 0;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const unsigned long long m = __ballot(rendered(rv[r]) && depth_class(rv[r], sv[r], t) == 0);
            if (lane == r) mine = m;
        }
        if (my_live)                                                // lane r < 4 stores the word of row r
            plane[(size_t)(row0 + lane) * words_per_row + (uint32_t)(x0 >> 6)] = mine;
    }
}

hipError_t launch_support_bits(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height,
                               const void *scene, bool scene_i32, int32_t tau, unsigned long long *planes, hipStream_t s)
{
    const uint32_t wpr = overlap_words_per_row(width);
    return for_box_launches(depth, box_off, n_poses, width, height, scene, scene_i32, [&](const BoxLaunch &b, auto *sc) {
        hipLaunchKernelGGL(support_bits_kernel, b.grid, dim3(256), 0, s, b.depth, bbox + b.p0, width, height, b.box_off, sc, tau,
                           planes + (size_t)b.p0 * height * wpr, wpr);
    });
}

// Pair counts.  Workgroup i owns hypothesis i and the pairs (i, i + k mod P) for k = 0 .. P / 2 (for even P the distance P / 2 belongs to the
// lower index only): every unordered pair, the diagonal included, has exactly one owner, and every workgroup has the same number of pairs --
// the triangle "j > i" would give workgroup 0 all of P - 1 and the last one none.  The words of i's box go into LDS, in bands of rows when
// the box has more than kPairTileWords; the wavefronts -- 16 per workgroup, of gridDim.y workgroups that share i when the batch is small -- take
// the partners in turn, lanes over the (row, word) cells of the two boxes' intersection inside the band, four cells per lane at a time so that
// the partner's words are in flight together, popcount(a & b), a wave sum, and lane 0 stores [i][j] and [j][i] (first band) or adds to what it stored for
// the band before (the same lane of the same wavefront: program order).  One writer per element and integer sums: reproducible without
// atomics.  Partners whose box does not meet i's cost no plane reads; an empty box gives a row and a column of zeros.
constexpr uint32_t kPairThreads = 1024, kPairWaves = kPairThreads / 64;
constexpr uint32_t kPairCellsPerLane = 4, kPairMinGroups = 1024, kPairMaxSplits = 8;
constexpr uint32_t kPairTileWords = 6144;                             // 48 KB of LDS: a 640 x 480 frame (10 x 480 words) in one band; three workgroups per CU

__global__ __launch_bounds__(kPairThreads) void pair_overlap_kernel(const unsigned long long *__restrict__ planes, const int4 *__restrict__ bbox, uint32_t n_poses,
                                                                    uint32_t height, uint32_t words_per_row, uint32_t *mat)
{
    __shared__ unsigned long long tile[kPairTileWords];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x, P = n_poses;
    const uint32_t n_k = ((P & 1u) || i < P / 2) ? P / 2 + 1 : P / 2;                  // partners i + k, k = 0 .. n_k - 1
    const uint32_t k_first = blockIdx.y * kPairWaves + wave, k_step = gridDim.y * kPairWaves;      // gridDim.y workgroups share i's partners
    const size_t plane_words = (size_t)height * words_per_row;
    const WordBox bi = word_box(bbox[i], height);
    if (bi.r0 > bi.r1 || (uint32_t)bi.w1 >= words_per_row) {                          // nothing rendered into: zeros
        for (uint32_t k = blockIdx.y * kPairThreads + threadIdx.x; k < n_k; k += gridDim.y * kPairThreads) {
            const uint32_t j = (i + k < P) ? i + k : i + k - P;
            mat[(size_t)i * P + j] = 0; mat[(size_t)j * P + i] = 0;
        }
        return;
    }
    const uint32_t nw_i = (uint32_t)(bi.w1 - bi.w0 + 1);                               // <= 128 (frames are at most 8192 wide)
    const uint32_t magic_i = fast_div_magic(nw_i);
    const int band_rows = (int)(kPairTileWords / nw_i);
    const unsigned long long *plane_i = planes + (size_t)i * plane_words;
    for (int band0 = bi.r0; band0 <= bi.r1; band0 += band_rows) {
        const int band1 = min(band0 + band_rows - 1, bi.r1);
        if (band0 != bi.r0) __syncthreads();                                           // every wavefront is done with the band before
        const uint32_t n_tile = (uint32_t)(band1 - band0 + 1) * nw_i;
        for (uint32_t c = threadIdx.x; c < n_tile; c += kPairThreads) {
            const uint32_t r = fast_div(c, magic_i), w = c - r * nw_i;
            tile[c] = plane_i[(size_t)(band0 + (int)r) * words_per_row + (uint32_t)bi.w0 + w];
        }
        __syncthreads();
        for (uint32_t k = k_first; k < n_k; k += k_step) {
            const uint32_t j = (i + k < P) ? i + k : i + k - P;
            const WordBox bj = word_box(bbox[j], height);
            const int r0 = max(band0, bj.r0), r1 = min(band1, bj.r1), w0 = max(bi.w0, bj.w0), w1 = min(bi.w1, bj.w1);
            uint32_t count = 0;
            if (bj.r0 <= bj.r1 && r0 <= r1 && w0 <= w1) {                              // the same for every lane of the wavefront
                const uint32_t nw = (uint32_t)(w1 - w0 + 1), cells = (uint32_t)(r1 - r0 + 1) * nw, magic = fast_div_magic(nw);
                const unsigned long long *pj = planes + (size_t)j * plane_words + (size_t)r0 * words_per_row + (uint32_t)w0;
                const unsigned long long *ti = tile + (uint32_t)(r0 - band0) * nw_i + (uint32_t)(w0 - bi.w0);
                for (uint32_t c0 = lane; c0 < cells; c0 += 64 * kPairCellsPerLane) {
                    unsigned long long a[kPairCellsPerLane], b[kPairCellsPerLane];     // the partner's words in flight before the first popcount
#pragma unroll
                    for (uint32_t u = 0; u < kPairCellsPerLane; ++u) {
                        const uint32_t c = c0 + 64 * u;
                        const bool in = c < cells;
                        const uint32_t r = fast_div(in ? c : 0, magic), w = (in ? c : 0) - r * nw;
                        b[u] = in ? pj[(size_t)r * words_per_row + w] : 0;
                        a[u] = ti[r * nw_i + w];
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kPairCellsPerLane; ++u) count += (uint32_t)__popcll(a[u] & b[u]);
                }
                count = wave_sum_u32(count);
            }
            if (lane == 0) {
                uint32_t *e = mat + (size_t)i * P + j;
                const uint32_t v = (band0 == bi.r0) ? count : *e + count;
                *e = v;
                mat[(size_t)j * P + i] = v;
            }
        }
    }
}

hipError_t launch_pair_overlap(const unsigned long long *planes, const int4 *bbox, uint32_t n_poses, uint32_t width, uint32_t height, uint32_t *mat, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    // small batches: several workgroups per hypothesis, so that the launch still has about kPairMinGroups of them (256 CUs, up to three per CU)
    const uint32_t want = (kPairMinGroups + n_poses - 1) / n_poses, splits = want > kPairMaxSplits ? kPairMaxSplits : want;
    hipLaunchKernelGGL(pair_overlap_kernel, dim3(n_poses, splits), dim3(kPairThreads), 0, s, planes, bbox, n_poses, height, overlap_words_per_row(width), mat);
    return hipGetLastError();
}

}  // namespace prk
