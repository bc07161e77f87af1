// cover.hip -- detections by cumulative cover: walk a ranking and keep a hypothesis for the inlier pixels it adds to what the better ones already claim
// gfx950 (CDNA4, wave64); integers only: every value is bit-identical to the CPU restatement (pr_select_cover_host).
#include "score_walk.h"

namespace prk {

// The walk of pr_score_cover is sequential by definition -- whether i is accepted depends on everything accepted before it -- but the claimed set C
// only grows, so fresh_i = |S_i \ C| only shrinks: a hypothesis that fails against some C fails against every later one, and the first
// hypothesis of the order that passes against the C of k acceptances is exactly the one the sequential walk accepts next.  So the device goes in
// ROUNDS of two launches: cover_gain_kernel counts fresh for every still-undecided hypothesis at once (one workgroup each) and applies the two integer
// tests; cover_commit_kernel (one workgroup) rejects the ones that failed, for good, accepts the passing one that comes first in the order and ORs its
// plane into C.  K detections take K + 1 rounds whatever the batch size; nothing is a chain of dependent loads through one workgroup but the commit's
// OR of one box.  Between rounds a hypothesis is UNDECIDED (internal; never returned): every hypothesis of the order ends EMPTY, ACCEPTED or REJECTED.
constexpr uint32_t kCoverUndecided = 0x80000000u, kCoverPassed = 0x40000000u;
constexpr uint32_t kCoverCtlFinished = 0, kCoverCtlSelected = 1, kCoverCtlClaimed = 2, kCoverCtlLastPos = 3;      // (words 4 .. 7: reserved, 0)
constexpr uint32_t kGainThreads = 256, kGainCellsPerLane = 4, kCommitThreads = 1024;
static_assert(kCoverCtlWords >= 4, "the control words");

// support, state and position of the hypotheses of a depth chunk, from the score records the chunk's score kernel has just finished
__global__ __launch_bounds__(256) void cover_init_kernel(const uint32_t *__restrict__ records, uint32_t p0, uint32_t np, uint32_t *ctl, uint32_t *rec,
                                                         const uint32_t *__restrict__ pos)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (p0 == 0 && k < kCoverCtlWords) ctl[k] = k == kCoverCtlLastPos ? kCoverNoPos : 0u;
    if (k >= np) return;
    const uint32_t support = records[8 * (size_t)k + 1];                 // pr_pose_score.inlier
    uint32_t *r = rec + 4 * ((size_t)p0 + k);
    r[0] = support; r[1] = 0;
    r[2] = pos[p0 + k] == kCoverNoPos ? (uint32_t)PR_COVER_NOT_IN_ORDER : (support == 0 ? (uint32_t)PR_COVER_EMPTY : kCoverUndecided);
    r[3] = PR_COVER_NO_POSITION;
}

// Gain.  Workgroup i owns hypothesis i: popcount(S_i & ~C) over the words of its box (rows r0 .. r1, words x0 >> 6 .. x1 >> 6 -- the words
// support_bits_kernel wrote, and no others), lanes over the (row, word) cells, kGainCellsPerLane cells of both planes in flight per lane before the
// first popcount; wave sums by DPP, the four wavefronts' through LDS (block_totals), and thread 0 alone stores the count and the verdict: one writer
// per hypothesis, no atomics, integer sums.  During the walk (final == 0) only undecided hypotheses are counted and the launch is a no-op once the
// finished word is set; the pass after the walk (final == 1) counts everything that was not accepted against the final C and touches `fresh` only.
__global__ __launch_bounds__(kGainThreads) void cover_gain_kernel(const unsigned long long *__restrict__ planes, const int4 *__restrict__ bbox, uint32_t height,
                                                                  uint32_t words_per_row, CoverRule rule, const uint32_t *__restrict__ ctl, uint32_t *rec,
                                                                  const unsigned long long *__restrict__ claimed, uint32_t final)
{
    const uint32_t i = blockIdx.x;
    uint32_t *r = rec + 4 * (size_t)i;
    const uint32_t state = r[2];                                          // the same for every thread: the workgroup leaves before any barrier
    if (final) { if (state == PR_COVER_ACCEPTED || state == PR_COVER_EMPTY) return; }
    else if (ctl[kCoverCtlFinished] || !(state & kCoverUndecided)) return;
    const WordBox b = word_box(bbox[i], height);
    uint32_t count[1] = { 0 };
    if (b.r0 <= b.r1 && (uint32_t)b.w1 < words_per_row) {
        const uint32_t nw = (uint32_t)(b.w1 - b.w0 + 1), cells = (uint32_t)(b.r1 - b.r0 + 1) * nw, magic = fast_div_magic(nw);      // cells * nw < 2^32: frames are at most 8192 on a side
        const size_t first = (size_t)b.r0 * words_per_row + (uint32_t)b.w0;
        const unsigned long long *ps = planes + (size_t)i * height * words_per_row + first, *pc = claimed + first;
        for (uint32_t c0 = threadIdx.x; c0 < cells; c0 += kGainThreads * kGainCellsPerLane) {
            unsigned long long a[kGainCellsPerLane], c[kGainCellsPerLane];
#pragma unroll
            for (uint32_t u = 0; u < kGainCellsPerLane; ++u) {
                const uint32_t cell = c0 + kGainThreads * u;
                const bool in = cell < cells;
                const uint32_t row = fast_div(in ? cell : 0, magic), w = (in ? cell : 0) - row * nw;
                const size_t off = (size_t)row * words_per_row + w;
                a[u] = in ? ps[off] : 0;
                c[u] = in ? pc[off] : 0;
            }
#pragma unroll
            for (uint32_t u = 0; u < kGainCellsPerLane; ++u) count[0] += (uint32_t)__popcll(a[u] & ~c[u]);
        }
    }
    const uint32_t fresh = block_totals(count);                           // thread 0: the workgroup's total
    if (threadIdx.x != 0) return;
    r[1] = fresh;
    if (!final) {
        const bool pass = fresh >= rule.min_new && (unsigned long long)fresh * rule.new_den >= (unsigned long long)rule.new_num * r[0];
        r[2] = kCoverUndecided | (pass ? kCoverPassed : 0u);
    }
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, o));
    return x;
}

// every hypothesis of the order at position >= first that has support and was not accepted: the walk never reached it with room left.  Thread t
// visits the hypotheses t, t + kCommitThreads, ... here and in the commit's scan alike, so it meets its own earlier stores in program order.
__device__ __forceinline__ void cover_relabel_cap(uint32_t n_poses, uint32_t first, uint32_t *rec, const uint32_t *__restrict__ pos)
{
    for (uint32_t j = threadIdx.x; j < n_poses; j += kCommitThreads) {
        const uint32_t p = pos[j];
        if (p != kCoverNoPos && p >= first && rec[4 * (size_t)j] != 0) rec[4 * (size_t)j + 2] = PR_COVER_REJECTED | PR_COVER_REASON_CAP;
    }
}

// Commit.  One workgroup.  Every undecided hypothesis that failed is rejected -- final, by the monotonicity above -- and of those that passed the one
// with the smallest order position is accepted: a ballot says whether a wavefront saw a passing one at all, a min-reduction over order
// positions (unique, so the minimum names the hypothesis through `at`) picks it.  Its box words are ORed into C by the whole workgroup (nobody else
// writes C), thread 0 records position, the selected list and the counters.  The walk is over when nothing that passed is left or max_keep
// is reached; then the finished word is set and every later launch of either kernel returns at once.
__global__ __launch_bounds__(kCommitThreads) void cover_commit_kernel(const unsigned long long *__restrict__ planes, const int4 *__restrict__ bbox, uint32_t n_poses,
                                                                      uint32_t height, uint32_t words_per_row, CoverRule rule, uint32_t *ctl, uint32_t *rec,
                                                                      const uint32_t *__restrict__ pos, const uint32_t *__restrict__ at, uint32_t *selected,
                                                                      unsigned long long *claimed)
{
    __shared__ uint32_t wave_best[kCommitThreads / 64], wave_passed[kCommitThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (ctl[kCoverCtlFinished]) return;                                   // the same for every thread
    const uint32_t n_sel = ctl[kCoverCtlSelected];
    if (rule.max_keep == 0) {                                             // nothing may be accepted: everything with support is beyond the cap
        cover_relabel_cap(n_poses, 0, rec, pos);
        if (threadIdx.x == 0) ctl[kCoverCtlFinished] = 1;
        return;
    }
    uint32_t best = kCoverNoPos, passed = 0;
    for (uint32_t j = threadIdx.x; j < n_poses; j += kCommitThreads) {
        const uint32_t st = rec[4 * (size_t)j + 2];
        if (!(st & kCoverUndecided)) continue;
        if (st & kCoverPassed) { best = min(best, pos[j]); ++passed; }
        else rec[4 * (size_t)j + 2] = PR_COVER_REJECTED | PR_COVER_REASON_THRESHOLD;
    }
    const bool any = __ballot(passed != 0) != 0;                          // wave-uniform
    if (any) { best = wave_min_u32(best); passed = wave_sum_u32(passed); }
    if (lane == 0) { wave_best[wave] = best; wave_passed[wave] = passed; }
    __syncthreads();
    best = kCoverNoPos; passed = 0;
#pragma unroll
    for (uint32_t w = 0; w < kCommitThreads / 64; ++w) { best = min(best, wave_best[w]); passed += wave_passed[w]; }
    if (best == kCoverNoPos) {                                            // nothing passed: the walk is over
        if (threadIdx.x == 0) ctl[kCoverCtlFinished] = 1;
        return;
    }
    const uint32_t win = at[best];
    const WordBox b = word_box(bbox[win], height);
    if (b.r0 <= b.r1 && (uint32_t)b.w1 < words_per_row) {
        const uint32_t nw = (uint32_t)(b.w1 - b.w0 + 1), cells = (uint32_t)(b.r1 - b.r0 + 1) * nw, magic = fast_div_magic(nw);
        const size_t first = (size_t)b.r0 * words_per_row + (uint32_t)b.w0;
        const unsigned long long *ps = planes + (size_t)win * height * words_per_row + first;
        unsigned long long *pc = claimed + first;
        for (uint32_t cell = threadIdx.x; cell < cells; cell += kCommitThreads) {
            const uint32_t row = fast_div(cell, magic), w = cell - row * nw;
            const size_t off = (size_t)row * words_per_row + w;
            const unsigned long long s = ps[off];
            if (s) pc[off] |= s;
        }
    }
    const bool full = n_sel + 1 >= rule.max_keep;
    if (threadIdx.x == 0) {
        rec[4 * (size_t)win + 2] = PR_COVER_ACCEPTED;
        rec[4 * (size_t)win + 3] = n_sel;
        selected[n_sel] = win;
        ctl[kCoverCtlSelected] = n_sel + 1;
        ctl[kCoverCtlClaimed] += rec[4 * (size_t)win + 1];                // its fresh, as the gain kernel of this round counted it
        ctl[kCoverCtlLastPos] = best;
        if (full || passed == 1) ctl[kCoverCtlFinished] = 1;
    }
    if (full) cover_relabel_cap(n_poses, best + 1, rec, pos);             // (the accepted one sits at `best`: not touched)
}

hipError_t launch_cover_init(const uint32_t *records, uint32_t p0, uint32_t np, const CoverState &st, hipStream_t s)
{
    const uint32_t n = np > kCoverCtlWords ? np : kCoverCtlWords;
    hipLaunchKernelGGL(cover_init_kernel, dim3((n + 255) / 256), dim3(256), 0, s, records, p0, np, st.ctl, st.rec, st.pos);
    return hipGetLastError();
}

hipError_t launch_cover_round(const unsigned long long *planes, const int4 *bbox, uint32_t n_poses, uint32_t width, uint32_t height, const CoverRule &rule,
                              const CoverState &st, unsigned long long *claimed, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    const uint32_t wpr = overlap_words_per_row(width);
    if (rule.max_keep)
        hipLaunchKernelGGL(cover_gain_kernel, dim3(n_poses), dim3(kGainThreads), 0, s, planes, bbox, height, wpr, rule, st.ctl, st.rec, claimed, 0u);
    hipLaunchKernelGGL(cover_commit_kernel, dim3(1), dim3(kCommitThreads), 0, s, planes, bbox, n_poses, height, wpr, rule, st.ctl, st.rec, st.pos, st.at, st.selected,
                       claimed);
    return hipGetLastError();
}

hipError_t launch_cover_final(const unsigned long long *planes, const int4 *bbox, uint32_t n_poses, uint32_t width, uint32_t height, const CoverState &st,
                              const unsigned long long *claimed, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    hipLaunchKernelGGL(cover_gain_kernel, dim3(n_poses), dim3(kGainThreads), 0, s, planes, bbox, height, overlap_words_per_row(width), CoverRule{}, st.ctl, st.rec,
                       claimed, 1u);
    return hipGetLastError();
}

}  // namespace prk
