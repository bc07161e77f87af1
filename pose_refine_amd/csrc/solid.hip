// solid.hip -- do two hypotheses claim the same space?  Per pixel a closed mesh occupies the depth interval [near, far] along the ray (the two planes of a
// span render, raster.hip); for every pair of hypotheses the pixels where the two intervals overlap are counted and the overlaps summed (pr_pose_penetration)
// gfx950 (CDNA4, wave64); integers only, differences in 64 bits: every value is bit-identical to the CPU restatement.
#include "score_walk.h"

namespace prk {

// a pixel box in frame columns and image rows (raster rows run flipped); empty: r0 > r1
struct PixBox { int x0, x1, r0, r1; };
constexpr uint32_t kSolidThreads = 1024, kSolidWaves = kSolidThreads / 64;
constexpr uint32_t kSolidCellsPerLane = 4, kSolidMinGroups = 1024, kSolidMaxSplits = 8;
constexpr uint32_t kSolidTilePx = 8192;                               // 64 KB of LDS as {near, far} pairs: at least one row of any box (a frame is at most 8192 wide)
constexpr uint32_t kSolidWords = 6;                                   // pr_pair_solid in 32-bit words: both, inter, max_mm, reserved, sum_mm lo / hi

__device__ __forceinline__ PixBox pix_box(const int4 bb, uint32_t height)
{
    PixBox b{ bb.x, bb.z, (int)height - 1 - bb.w, (int)height - 1 - bb.y };
    if (bb.x > bb.z || bb.y > bb.w || bb.x < 0 || b.r0 < 0 || b.r1 >= (int)height || (uint32_t)(bb.z - bb.x) >= kSolidTilePx) { b.r0 = 1; b.r1 = 0; }   // (boxes are clipped to the frame: only the first two tests ever fire)
    return b;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x)
{
    for (int off = 32; off > 0; off >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, off));
    return x;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x)
{
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// Pair records.  pair_overlap_kernel's shape (select.hip): workgroup i owns hypothesis i and the pairs (i, i + k mod P) for k = 0 .. P / 2 (for even P the
// distance P / 2 belongs to the lower index only), so every unordered pair, the diagonal included, has exactly one owner.  The {near, far} pairs of i's box
// go into LDS, in bands of rows when the box has more than kSolidTilePx pixels (a band is a contiguous run of the packed box); the wavefronts -- 16 per
// workgroup, of gridDim.y workgroups that share i when the batch is small -- take the partners in turn, lanes over the pixels of the two boxes' intersection
// inside the band, four pixels per lane at a time so that the partner's eight words are in flight before the first compare.  Counters per lane, a wave sum
// and a wave maximum, and lane 0 stores [i][j] and [j][i] (first band) or adds to what it stored for the band before (the same lane of the same wavefront:
// program order).  One writer per record, integer sums and maxima: the same bytes on every call, no atomics.  A partner whose box does not meet i's reads
// nothing; an empty box gives a row and a column of zeros.
__global__ __launch_bounds__(kSolidThreads) void pair_solid_kernel(const int32_t *__restrict__ depth, const int32_t *__restrict__ far, const int4 *__restrict__ bbox,
                                                                   const uint32_t *__restrict__ box_off, uint32_t n_poses, uint32_t height, int32_t slack,
                                                                   uint32_t *rec)
{
    __shared__ int2 tile[kSolidTilePx];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x, P = n_poses;
    const uint32_t n_k = ((P & 1u) || i < P / 2) ? P / 2 + 1 : P / 2;                  // partners i + k, k = 0 .. n_k - 1
    const uint32_t k_first = blockIdx.y * kSolidWaves + wave, k_step = gridDim.y * kSolidWaves;
    const PixBox bi = pix_box(bbox[i], height);
    if (bi.r0 > bi.r1) {                                                              // nothing rendered into: zeros
        for (uint32_t k = blockIdx.y * kSolidThreads + threadIdx.x; k < n_k; k += gridDim.y * kSolidThreads) {
            const uint32_t j = (i + k < P) ? i + k : i + k - P;
            uint32_t *a = rec + ((size_t)i * P + j) * kSolidWords, *b = rec + ((size_t)j * P + i) * kSolidWords;
#pragma unroll
            for (uint32_t w = 0; w < kSolidWords; ++w) { a[w] = 0; b[w] = 0; }
        }
        return;
    }
    const uint32_t wi = (uint32_t)(bi.x1 - bi.x0 + 1);
    const int band_rows = (int)(kSolidTilePx / wi);
    const int32_t *near_i = depth + box_off[i], *far_i = far + box_off[i];
    const int64_t sl = slack;
    for (int band0 = bi.r0; band0 <= bi.r1; band0 += band_rows) {
        const int band1 = min(band0 + band_rows - 1, bi.r1);
        if (band0 != bi.r0) __syncthreads();                                           // every wavefront is done with the band before
        const uint32_t n_tile = (uint32_t)(band1 - band0 + 1) * wi, first = (uint32_t)(band0 - bi.r0) * wi;
        for (uint32_t c = threadIdx.x; c < n_tile; c += kSolidThreads) tile[c] = make_int2(near_i[first + c], far_i[first + c]);
        __syncthreads();
        for (uint32_t k = k_first; k < n_k; k += k_step) {
            const uint32_t j = (i + k < P) ? i + k : i + k - P;
            const PixBox bj = pix_box(bbox[j], height);
            const int r0 = max(band0, bj.r0), r1 = min(band1, bj.r1), x0 = max(bi.x0, bj.x0), x1 = min(bi.x1, bj.x1);
            uint32_t both = 0, inter = 0, longest = 0;
            unsigned long long sum = 0;
            if (bj.r0 <= bj.r1 && r0 <= r1 && x0 <= x1) {                              // the same for every lane of the wavefront
                const uint32_t nx = (uint32_t)(x1 - x0 + 1), cells = (uint32_t)(r1 - r0 + 1) * nx, magic = fast_div_magic(nx);   // cells <= kSolidTilePx: cells * nx < 2^32
                const uint32_t wj = (uint32_t)(bj.x1 - bj.x0 + 1);
                const size_t at_j = (size_t)box_off[j] + (size_t)(r0 - bj.r0) * wj + (uint32_t)(x0 - bj.x0);
                const int32_t *near_j = depth + at_j, *far_j = far + at_j;
                const int2 *ti = tile + (uint32_t)(r0 - band0) * wi + (uint32_t)(x0 - bi.x0);
                for (uint32_t c0 = lane; c0 < cells; c0 += 64 * kSolidCellsPerLane) {
                    int32_t an[kSolidCellsPerLane], af[kSolidCellsPerLane], bn[kSolidCellsPerLane], bf[kSolidCellsPerLane];
#pragma unroll
                    for (uint32_t u = 0; u < kSolidCellsPerLane; ++u) {                // the partner's words in flight before the first compare
                        const uint32_t c = c0 + 64 * u;
                        const bool in = c < cells;
                        const uint32_t r = fast_div(in ? c : 0, magic), x = (in ? c : 0) - r * nx;
                        bn[u] = in ? near_j[(size_t)r * wj + x] : 0;
                        bf[u] = in ? far_j[(size_t)r * wj + x] : 0;
                        const int2 a = ti[r * wi + x];
                        an[u] = in ? a.x : 0; af[u] = a.y;
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kSolidCellsPerLane; ++u) {
                        if (!(rendered(an[u]) && rendered(bn[u]))) continue;
                        ++both;
                        const int64_t len = (int64_t)min(af[u], bf[u]) - (int64_t)max(an[u], bn[u]);      // 64 bits: no overflow for any int32 pair
                        if (len > sl) { ++inter; sum += (unsigned long long)len; longest = max(longest, (uint32_t)len); }
                    }
                }
                both = wave_sum_u32(both); inter = wave_sum_u32(inter); longest = wave_max_u32(longest); sum = wave_sum_u64(sum);
            }
            if (lane == 0) {
                uint32_t *a = rec + ((size_t)i * P + j) * kSolidWords, *b = rec + ((size_t)j * P + i) * kSolidWords;
                if (band0 != bi.r0) {
                    both += a[0]; inter += a[1]; longest = max(longest, a[2]);
                    sum += (unsigned long long)a[4] | ((unsigned long long)a[5] << 32);
                }
                const uint32_t v[kSolidWords] = { both, inter, longest, 0u, (uint32_t)sum, (uint32_t)(sum >> 32) };
#pragma unroll
                for (uint32_t w = 0; w < kSolidWords; ++w) { a[w] = v[w]; b[w] = v[w]; }
            }
        }
    }
}

hipError_t launch_pair_solid(const int32_t *depth, const int32_t *far, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t height,
                             int32_t slack, uint32_t *records, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    // small batches: several workgroups per hypothesis, as launch_pair_overlap
    const uint32_t want = (kSolidMinGroups + n_poses - 1) / n_poses, splits = want > kSolidMaxSplits ? kSolidMaxSplits : want;
    hipLaunchKernelGGL(pair_solid_kernel, dim3(n_poses, splits), dim3(kSolidThreads), 0, s, depth, far, bbox, box_off, n_poses, height, slack, records);
    return hipGetLastError();
}

}  // namespace prk
