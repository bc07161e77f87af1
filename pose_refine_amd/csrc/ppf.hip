// ppf.hip -- point-pair-feature voting: the model's direct-addressed pair table (count, scan, fill), the strided scene sample (count, scan, emit)
// and the voting kernel with its peaks (pr_ppf_*; the definition is in include/pose_refine.h, its one implementation in ppf.h)
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "pr_launch.h"
#include "ppf.h"

namespace prk {

constexpr uint32_t kPpfThreads = 256;
constexpr uint32_t kPpfVoteThreads = 1024;                       // one workgroup per CU (its accumulator fills the LDS): 16 wavefronts to hide the table's latency

__device__ __forceinline__ pr_vec3 ld_vec3(const pr_vec3 *a, uint32_t i) { return a[i]; }

// the descriptor's two edge tables from the kernel arguments into LDS (read with wave-uniform indices afterwards: broadcasts)
__device__ __forceinline__ void stage_tables(const ppf::Tables &tb, float *cos_edge, float *alpha_edge)
{
    for (uint32_t k = threadIdx.x; k <= PR_PPF_MAX_ANGLE_BINS; k += blockDim.x) cos_edge[k] = tb.cos_edge[k];
    for (uint32_t k = threadIdx.x; k <= PR_PPF_MAX_ALPHA_BINS / 2; k += blockDim.x) alpha_edge[k] = tb.alpha_edge[k];
    __syncthreads();
}

__global__ __launch_bounds__(kPpfThreads) void ppf_zero_kernel(uint32_t *w, uint32_t n)
{
    for (uint32_t i = blockIdx.x * kPpfThreads + threadIdx.x; i < n; i += gridDim.x * kPpfThreads) w[i] = 0;
}

// Ordered model pair t = ref * n_model + other.  kFill false: the histogram of the keys; true: the entry goes to its bucket, at the position an
// integer atomic on the bucket's cursor hands out (the order inside a bucket is whatever the hardware makes it: the header leaves it open).
template <bool kFill>
__global__ __launch_bounds__(kPpfThreads) void ppf_model_pairs_kernel(const ppf::Tables tb, const pr_vec3 *__restrict__ points, const pr_vec3 *__restrict__ normals,
                                                                      uint32_t n_model, uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                                      pr_ppf_entry *__restrict__ entries)
{
    __shared__ float cos_edge[PR_PPF_MAX_ANGLE_BINS + 1], alpha_edge[PR_PPF_MAX_ALPHA_BINS / 2 + 1];
    stage_tables(tb, cos_edge, alpha_edge);
    const uint32_t t = blockIdx.x * kPpfThreads + threadIdx.x;
    if (t >= n_model * n_model) return;
    const uint32_t r = t / n_model, i = t - r * n_model;
    if (r == i) return;
    const pr_vec3 pr = ld_vec3(points, r), nr = ld_vec3(normals, r);
    const ppf::Frame fr = ppf::make_frame(nr.x, nr.y, nr.z);
    const ppf::Pair p = ppf::make_pair(fr, tb.inv_dist_step, tb.n_dist, tb.n_angle, cos_edge, pr, nr, ld_vec3(points, i), ld_vec3(normals, i));
    if (!p.ok) return;
    const uint32_t at = atomicAdd(&counts[p.key], 1u);
    if (kFill) {
        const uint32_t slot = offsets[p.key] + at;
        if (slot < offsets[p.key + 1]) entries[slot] = pr_ppf_entry{ (r << 16) | i, p.c, p.s };
    }
}

// ---- the scene sample: one wavefront per sampled row (wave_compact_count / wave_compact_place over its sampled columns) ---------------------
__device__ __forceinline__ bool scene_keep(const float *__restrict__ pcd, const float *__restrict__ normal, size_t px)
{
    const float nx = normal[px * 3], ny = normal[px * 3 + 1], nz = normal[px * 3 + 2];
    return (nx != 0.0f || ny != 0.0f || nz != 0.0f) && pcd[px * 3 + 2] > 0.0f;
}
__global__ __launch_bounds__(64) void ppf_scene_count_kernel(const float *__restrict__ pcd, const float *__restrict__ normal, uint32_t width, uint32_t stride,
                                                             uint32_t *__restrict__ row_count)
{
    const size_t row = (size_t)blockIdx.x * stride * width;
    const uint32_t n = wave_compact_count((width + stride - 1) / stride, threadIdx.x, [&](uint32_t c) { return scene_keep(pcd, normal, row + (size_t)c * stride); });
    if (threadIdx.x == 0) row_count[blockIdx.x] = n;
}
__global__ __launch_bounds__(64) void ppf_scene_emit_kernel(const float *__restrict__ pcd, const float *__restrict__ normal, uint32_t width, uint32_t stride,
                                                            const uint32_t *__restrict__ row_off, pr_vec3 *__restrict__ points, pr_vec3 *__restrict__ normals)
{
    const size_t row = (size_t)blockIdx.x * stride * width;
    wave_compact_place((width + stride - 1) / stride, threadIdx.x, row_off[blockIdx.x], [&](uint32_t c) { return scene_keep(pcd, normal, row + (size_t)c * stride); },
                       [&](uint32_t c, bool kept, uint32_t pos) {
                           if (!kept || pos >= PR_PPF_MAX_SCENE_POINTS) return;
                           const size_t px = row + (size_t)c * stride;
                           points[pos] = pr_vec3{ pcd[px * 3] * 1000.0f, pcd[px * 3 + 1] * 1000.0f, pcd[px * 3 + 2] * 1000.0f };
                           normals[pos] = pr_vec3{ normal[px * 3], normal[px * 3 + 1], normal[px * 3 + 2] };
                       });
}

// ---- voting: one workgroup per scene reference (and model), its accumulator votes[n_model * n_alpha] in LDS -----------------------------------
// Lanes run over the scene's other points; each forms the pair's key and angle and reads its bucket's bounds; every entry of the bucket is one
// integer LDS atomic.  Bucket lengths vary by orders of magnitude, so there are two walks (option "ppf_walk", same votes):
//   kCoop false: a lane walks its own pair's bucket -- a wavefront takes as long as its longest bucket;
//   kCoop true:  the wavefront concatenates the buckets of its 64 pairs (an exclusive scan of their lengths, staged with the pairs' angles in LDS)
//                and lane l takes entries l, l + 64, ... of the concatenation, finding each one's owner by a binary search over the 64 starts
//                (raster.hip's candidate expansion): lanes stay busy whatever the lengths, and neighbouring lanes read neighbouring entries.
// Then n_peaks rounds of a workgroup arg-max in the order (votes descending, cell ascending): the largest count by an LDS atomicMax, the lowest
// cell that holds it by an atomicMin; the winner's cell is zeroed for the next round.
struct PpfWaveStage { uint32_t start[64], lo[64]; float c[64], s[64]; };      // 1 KB per wavefront
// The whole of a workgroup's work, for both kernels below: reference j = blockIdx.x against one model (tb, offsets, entries, n_model); peaks,
// refs and acc_out are that model's (peaks[j * n_peaks + k], acc_out[j * n_cells + c]), the reference is stored when write_ref.
template <bool kCoop>
__device__ __forceinline__ void ppf_vote_workgroup(const ppf::Tables &tb, const uint32_t *__restrict__ offsets, const pr_ppf_entry *__restrict__ entries,
                                                   uint32_t n_model, const pr_vec3 *__restrict__ points, const pr_vec3 *__restrict__ normals,
                                                   uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride, uint32_t n_peaks,
                                                   pr_ppf_peak *__restrict__ peaks, PpfRef *__restrict__ refs, uint32_t *__restrict__ acc_out, bool write_ref)
{
    extern __shared__ uint32_t votes[];                            // n_model * n_alpha
    __shared__ float cos_edge[PR_PPF_MAX_ANGLE_BINS + 1], alpha_edge[PR_PPF_MAX_ALPHA_BINS / 2 + 1];
    __shared__ uint32_t n_pairs_s, best_votes, best_cell;
    const uint32_t n_alpha = tb.n_alpha, n_cells = n_model * n_alpha;
    for (uint32_t c = threadIdx.x; c < n_cells; c += kPpfVoteThreads) votes[c] = 0;
    if (threadIdx.x == 0) n_pairs_s = 0;
    stage_tables(tb, cos_edge, alpha_edge);                        // (ends in a barrier)

    const uint32_t s = ref_first + blockIdx.x * ref_stride;        // < n_scene: the entry point checked the last one
    const pr_vec3 pr = ld_vec3(points, s), nr = ld_vec3(normals, s);
    const ppf::Frame fr = ppf::make_frame(nr.x, nr.y, nr.z);
    uint32_t n_pairs = 0;
    if (kCoop) {
        __shared__ PpfWaveStage stage_all[kPpfVoteThreads / 64];
        PpfWaveStage &st = stage_all[threadIdx.x >> 6];
        const uint32_t lane = threadIdx.x & 63u;
        for (uint32_t base = threadIdx.x - lane; base < n_scene; base += kPpfVoteThreads) {      // wave-uniform: all 64 lanes take every turn
            const uint32_t i = base + lane, ic = i < n_scene ? i : s;
            ppf::Pair p = ppf::make_pair(fr, tb.inv_dist_step, tb.n_dist, tb.n_angle, cos_edge, pr, nr, ld_vec3(points, ic), ld_vec3(normals, ic));
            if (i >= n_scene) p.ok = false;
            uint32_t lo = 0, cnt = 0;
            if (p.ok) { ++n_pairs; lo = offsets[p.key]; cnt = offsets[p.key + 1] - lo; }
            uint32_t incl = cnt;                                   // inclusive scan of the lengths over the wavefront
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d); if (lane >= d) incl += up; }
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            st.start[lane] = incl - cnt; st.lo[lane] = lo; st.c[lane] = p.c; st.s[lane] = p.s;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (uint32_t t = lane; t < total; t += 64) {
                uint32_t j = 0;                                    // the last pair whose bucket starts at or before t (empty buckets share their successor's start and lose to it)
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1) if (st.start[j + step] <= t) j += step;
                const pr_ppf_entry en = entries[st.lo[j] + (t - st.start[j])];
                const uint32_t m = en.pair >> 16;
                const int bin = ppf::alpha_bin(alpha_edge, n_alpha, st.c[j], st.s[j], en.cos_m, en.sin_m);
                if (bin >= 0 && m < n_model) atomicAdd(&votes[m * n_alpha + (uint32_t)bin], 1u);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                       // the stage is rewritten on the next turn
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n_scene; i += kPpfVoteThreads) {
            const ppf::Pair p = ppf::make_pair(fr, tb.inv_dist_step, tb.n_dist, tb.n_angle, cos_edge, pr, nr, ld_vec3(points, i), ld_vec3(normals, i));
            if (!p.ok) continue;
            ++n_pairs;
            const uint32_t lo = offsets[p.key], hi = offsets[p.key + 1];
            for (uint32_t e = lo; e < hi; ++e) {
                const pr_ppf_entry en = entries[e];
                const uint32_t m = en.pair >> 16;
                const int bin = ppf::alpha_bin(alpha_edge, n_alpha, p.c, p.s, en.cos_m, en.sin_m);
                if (bin >= 0 && m < n_model) atomicAdd(&votes[m * n_alpha + (uint32_t)bin], 1u);
            }
        }
    }
    n_pairs = wave_sum_u32(n_pairs);
    if ((threadIdx.x & 63u) == 0) atomicAdd(&n_pairs_s, n_pairs);
    __syncthreads();
    if (acc_out) for (uint32_t c = threadIdx.x; c < n_cells; c += kPpfVoteThreads) acc_out[(size_t)blockIdx.x * n_cells + c] = votes[c];
    if (write_ref && threadIdx.x == 0) refs[blockIdx.x] = PpfRef{ pr, nr };

    for (uint32_t k = 0; k < n_peaks; ++k) {
        if (threadIdx.x == 0) { best_votes = 0; best_cell = 0xFFFFFFFFu; }
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t c = threadIdx.x; c < n_cells; c += kPpfVoteThreads) mine = max(mine, votes[c]);
        if (mine) atomicMax(&best_votes, mine);
        __syncthreads();
        const uint32_t top = best_votes;
        if (top && mine == top)
            for (uint32_t c = threadIdx.x; c < n_cells; c += kPpfVoteThreads) if (votes[c] == top) { atomicMin(&best_cell, c); break; }
        __syncthreads();
        if (threadIdx.x == 0) {
            pr_ppf_peak pk{ 0, 0, 0, s, n_pairs_s };
            if (top) { pk.votes = top; pk.model_ref = (uint16_t)(best_cell / n_alpha); pk.alpha_bin = (uint16_t)(best_cell % n_alpha); votes[best_cell] = 0; }
            peaks[blockIdx.x * n_peaks + k] = pk;
        }
        __syncthreads();
    }
}
template <bool kCoop>
__global__ __launch_bounds__(kPpfVoteThreads) void ppf_vote_kernel(const ppf::Tables tb, const uint32_t *__restrict__ offsets, const pr_ppf_entry *__restrict__ entries,
                                                               uint32_t n_model, const pr_vec3 *__restrict__ points, const pr_vec3 *__restrict__ normals,
                                                               uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride, uint32_t n_peaks,
                                                               pr_ppf_peak *__restrict__ peaks, PpfRef *__restrict__ refs, uint32_t *__restrict__ acc_out)
{
    ppf_vote_workgroup<kCoop>(tb, offsets, entries, n_model, points, normals, n_scene, ref_first, ref_stride, n_peaks, peaks, refs, acc_out, true);
}
// A table of models over one scene sample: workgroup (x, y) = (reference, model).  The model's record comes from the device table the entry point
// staged (a wave-uniform address: scalar loads), its edge tables go from there into LDS as above; the dynamic LDS of the launch is the largest
// model's accumulator, a workgroup uses its own model's n_model * n_alpha words of it.  The references are the same for every model: row 0 stores them.
template <bool kCoop>
__global__ __launch_bounds__(kPpfVoteThreads) void ppf_vote_multi_kernel(const PpfModelRec *__restrict__ models, const pr_vec3 *__restrict__ points,
                                                                     const pr_vec3 *__restrict__ normals, uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride,
                                                                     uint32_t n_peaks, pr_ppf_peak *__restrict__ peaks, PpfRef *__restrict__ refs, uint32_t *__restrict__ acc_out)
{
    const PpfModelRec &m = models[blockIdx.y];
    ppf_vote_workgroup<kCoop>(m.tb, m.offsets, m.entries, m.n_model, points, normals, n_scene, ref_first, ref_stride, n_peaks, peaks + m.peak_base, refs,
                              acc_out ? acc_out + m.acc_base : nullptr, blockIdx.y == 0);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
hipError_t launch_ppf_model_build(const ppf::Tables &tb, const pr_vec3 *points, const pr_vec3 *normals, uint32_t n_model, uint32_t *counts,
                                  uint32_t *offsets, pr_ppf_entry *entries, hipStream_t s)
{
    const uint32_t n_pairs = n_model * n_model, grid = (n_pairs + kPpfThreads - 1) / kPpfThreads;
    hipLaunchKernelGGL(ppf_zero_kernel, dim3(cap_grid((tb.n_keys + kPpfThreads - 1) / kPpfThreads)), dim3(kPpfThreads), 0, s, counts, tb.n_keys);
    hipLaunchKernelGGL(ppf_model_pairs_kernel<false>, dim3(grid), dim3(kPpfThreads), 0, s, tb, points, normals, n_model, counts, (const uint32_t *)nullptr, (pr_ppf_entry *)nullptr);
    { hipError_t e = launch_scan_counts(counts, tb.n_keys, offsets, nullptr, true, s); if (e != hipSuccess) return e; }      // the counts become the fill's cursors
    hipLaunchKernelGGL(ppf_model_pairs_kernel<true>, dim3(grid), dim3(kPpfThreads), 0, s, tb, points, normals, n_model, counts, (const uint32_t *)offsets, entries);
    return hipGetLastError();
}

hipError_t launch_ppf_scene_count(const float *pcd, const float *normal, uint32_t width, uint32_t height, uint32_t stride, uint32_t *row_count,
                                  uint32_t *row_off, hipStream_t s)
{
    const uint32_t gh = (height + stride - 1) / stride;
    hipLaunchKernelGGL(ppf_scene_count_kernel, dim3(gh), dim3(64), 0, s, pcd, normal, width, stride, row_count);
    return launch_scan_counts(row_count, gh, row_off, nullptr, false, s);      // row_off[gh] = the total
}

hipError_t launch_ppf_scene_emit(const float *pcd, const float *normal, uint32_t width, uint32_t height, uint32_t stride, const uint32_t *row_off,
                                 pr_vec3 *points, pr_vec3 *normals, hipStream_t s)
{
    const uint32_t gh = (height + stride - 1) / stride;
    hipLaunchKernelGGL(ppf_scene_emit_kernel, dim3(gh), dim3(64), 0, s, pcd, normal, width, stride, row_off, points, normals);
    return hipGetLastError();
}

hipError_t launch_ppf_vote(const ppf::Tables &tb, const uint32_t *offsets, const pr_ppf_entry *entries, uint32_t n_model, const pr_vec3 *points,
                           const pr_vec3 *normals, uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks,
                           pr_ppf_peak *peaks, PpfRef *refs, uint32_t *acc_out, bool cooperative, hipStream_t s)
{
    // the accumulator may take 128 KiB: beyond 64 KiB dynamic LDS is an opt-in per device and kernel, asked once for the cap
    auto *fn = cooperative ? ppf_vote_kernel<true> : ppf_vote_kernel<false>;
    if (!lds_opt_in(reinterpret_cast<const void *>(fn), cooperative ? 1 : 0, PR_PPF_MAX_CELLS * sizeof(uint32_t))) return hipErrorInvalidValue;
    const uint32_t lds = n_model * tb.n_alpha * (uint32_t)sizeof(uint32_t);
    hipLaunchKernelGGL(fn, dim3(n_refs), dim3(kPpfVoteThreads), lds, s, tb, offsets, entries, n_model, points, normals, n_scene, ref_first,
                       ref_stride, n_peaks, peaks, refs, acc_out);
    return hipGetLastError();
}

hipError_t launch_ppf_vote_multi(const PpfModelRec *models, uint32_t n_models, uint32_t max_cells, const pr_vec3 *points, const pr_vec3 *normals, uint32_t n_scene,
                                 uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks, pr_ppf_peak *peaks, PpfRef *refs, uint32_t *acc_out,
                                 bool cooperative, hipStream_t s)
{
    auto *fn = cooperative ? ppf_vote_multi_kernel<true> : ppf_vote_multi_kernel<false>;
    if (!lds_opt_in(reinterpret_cast<const void *>(fn), cooperative ? 3 : 2, PR_PPF_MAX_CELLS * sizeof(uint32_t))) return hipErrorInvalidValue;
    // dynamic LDS is one size per launch: the largest model's accumulator (a small model next to a large one reserves the large one's)
    hipLaunchKernelGGL(fn, dim3(n_refs, n_models), dim3(kPpfVoteThreads), max_cells * (uint32_t)sizeof(uint32_t), s, models, points, normals, n_scene, ref_first,
                       ref_stride, n_peaks, peaks, refs, acc_out);
    return hipGetLastError();
}

}  // namespace prk
