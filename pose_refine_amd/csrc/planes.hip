// planes.hip -- the dominant planes of a depth frame, peeled one after another: the strided sample (count, scan, emit), the support count of
// every one-point candidate, the winner, the integer moments of its inliers and the label pass (pr_scene_planes_dev; the definition is in
// include/pose_refine.h, its one implementation in planes.h)
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "pr_launch.h"
#include "planes.h"

namespace prk {

constexpr uint32_t kPlaneThreads = 256;
constexpr uint32_t kPlaneTile = 256;                             // samples staged per turn: one per thread
static_assert(kPlaneTile == kPlaneThreads, "plane_support_kernel: one staged sample per thread");

// ---- the sample: one wavefront per sampled row (wave_compact_count / wave_compact_place over its sampled columns) ---------------------------
__global__ __launch_bounds__(64) void plane_sample_count_kernel(const float *__restrict__ pcd, const float *__restrict__ normal, uint32_t width, uint32_t stride,
                                                                uint32_t *__restrict__ row_count)
{
    const size_t row = (size_t)blockIdx.x * stride * width;
    const uint32_t n = wave_compact_count((width + stride - 1) / stride, threadIdx.x, [&](uint32_t c) { return planes::sample_keep(pcd, normal, row + (size_t)c * stride); });
    if (threadIdx.x == 0) row_count[blockIdx.x] = n;
}
__global__ __launch_bounds__(64) void plane_sample_emit_kernel(const float *__restrict__ pcd, const float *__restrict__ normal, uint32_t width, uint32_t stride,
                                                               const uint32_t *__restrict__ row_off, PlaneSample *__restrict__ points, pr_vec3 *__restrict__ normals)
{
    const size_t row = (size_t)blockIdx.x * stride * width;
    wave_compact_place((width + stride - 1) / stride, threadIdx.x, row_off[blockIdx.x], [&](uint32_t c) { return planes::sample_keep(pcd, normal, row + (size_t)c * stride); },
                       [&](uint32_t c, bool kept, uint32_t pos) {
                           if (!kept || pos >= PR_PLANE_MAX_SAMPLES) return;
                           const size_t px = row + (size_t)c * stride;
                           points[pos] = PlaneSample{ pcd[px * 3] * 1000.0f, pcd[px * 3 + 1] * 1000.0f, pcd[px * 3 + 2] * 1000.0f, (uint32_t)px };
                           normals[pos] = pr_vec3{ normal[px * 3], normal[px * 3 + 1], normal[px * 3 + 2] };
                       });
}

__global__ __launch_bounds__(kPlaneThreads) void plane_init_kernel(const float *__restrict__ pcd, uint32_t n_px, uint8_t *__restrict__ labels, uint32_t *__restrict__ round_words,
                                                                   uint32_t n_round_words, uint32_t *__restrict__ support, uint32_t n_support)
{
    const uint32_t t = blockIdx.x * kPlaneThreads + threadIdx.x, step = gridDim.x * kPlaneThreads;
    for (uint32_t i = t; i < n_px; i += step) labels[i] = pcd[(size_t)i * 3 + 2] > 0.0f ? (uint8_t)0 : (uint8_t)PR_PLANE_NO_DEPTH;
    for (uint32_t i = t; i < n_round_words; i += step) round_words[i] = 0;
    for (uint32_t i = t; i < n_support; i += step) support[i] = 0;
}

// ---- support: lanes on candidates, samples through LDS -----------------------------------------------------------------------------------------
// Candidate c = sample c * cand_stride; its lane holds (p_c, n_c) and a counter in registers for the whole sample range of its workgroup row
// (blockIdx.y: tiles_per_row tiles of kPlaneTile samples).  A tile is staged once per workgroup, dead samples as "not alive" in the point's
// fourth word, and read back with a wave-uniform index (a broadcast: no bank conflict).  Counts are integers: one atomicAdd per (candidate, row)
// whatever the split.  A row that starts at or behind n (the launcher makes none) would stage nothing and add nothing.
__global__ __launch_bounds__(kPlaneThreads) void plane_support_kernel(const pr_plane_params pp, const PlaneSample *__restrict__ points, const pr_vec3 *__restrict__ normals,
                                                                      uint32_t n, uint32_t n_cand, const uint8_t *__restrict__ labels,
                                                                      uint32_t tiles_per_row, uint32_t *__restrict__ support)
{
    __shared__ float4 tile_p[kPlaneTile], tile_n[kPlaneTile];      // p.w: 1 = alive (as bits)
    const uint32_t c = blockIdx.x * kPlaneThreads + threadIdx.x;
    bool active = c < n_cand;                                      // (a lane without a candidate still stages samples and meets the barriers)
    float pcx = 0.0f, pcy = 0.0f, pcz = 0.0f, ncx = 0.0f, ncy = 0.0f, ncz = 0.0f;
    if (active) {
        const PlaneSample p = points[c * pp.cand_stride];          // < n: n_cand = ceil(n / cand_stride)
        const pr_vec3 m = normals[c * pp.cand_stride];
        pcx = p.x; pcy = p.y; pcz = p.z; ncx = m.x; ncy = m.y; ncz = m.z;
        active = labels[p.px] == 0;                 // a dead candidate keeps support 0
    }
    const uint32_t span = tiles_per_row * kPlaneTile;
    const uint32_t first = blockIdx.y * span;
    const uint32_t last = (first >= n) ? first : ((n - first < span) ? n : first + span);
    uint32_t count = 0;
    for (uint32_t base = first; base < last; base += kPlaneTile) {
        if (base != first) __syncthreads();                        // every lane is done with the tile before
        const uint32_t nt = (last - base < kPlaneTile) ? last - base : kPlaneTile;
        if (threadIdx.x < nt) {
            const PlaneSample p = points[base + threadIdx.x];
            const pr_vec3 m = normals[base + threadIdx.x];
            const uint32_t alive = labels[p.px] == 0 ? 1u : 0u;
            tile_p[threadIdx.x] = make_float4(p.x, p.y, p.z, __uint_as_float(alive));
            tile_n[threadIdx.x] = make_float4(m.x, m.y, m.z, 0.0f);
        }
        __syncthreads();
        if (!active) continue;
        for (uint32_t i = 0; i < nt; ++i) {
            const float4 p = tile_p[i], m = tile_n[i];
            const bool in = planes::supports(pp.tau_mm, pp.cos_min, pcx, pcy, pcz, ncx, ncy, ncz, p.x, p.y, p.z, m.x, m.y, m.z);
            count += (in && __float_as_uint(p.w) != 0u) ? 1u : 0u;
        }
    }
    if (active && count) atomicAdd(&support[c], count);
}

// one workgroup: the largest key over the candidates (support, then the lowest index); no candidate with support: the key stays 0
__global__ __launch_bounds__(kPlaneThreads) void plane_winner_kernel(const uint32_t *__restrict__ support, uint32_t n_cand, PlaneRound *__restrict__ round)
{
    unsigned long long best = 0;
    for (uint32_t c = threadIdx.x; c < n_cand; c += kPlaneThreads) {
        const uint32_t s = support[c];
        const unsigned long long key = s ? planes::winner_key(s, c) : 0ull;
        best = key > best ? key : best;
    }
    if (best) atomicMax(reinterpret_cast<unsigned long long *>(&round->key), best);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
    return v;
}
// The winner (read from the round's record, not through the host) against every alive sample: the ten moments of its inliers.  Integer sums:
// per wavefront by shuffles, per workgroup by LDS atomics, one global atomic per moment and workgroup -- exact in any order.
__global__ __launch_bounds__(kPlaneThreads) void plane_moments_kernel(const pr_plane_params pp, const PlaneSample *__restrict__ points, const pr_vec3 *__restrict__ normals,
                                                                      uint32_t n, const uint8_t *__restrict__ labels, PlaneRound *__restrict__ round)
{
    __shared__ unsigned long long sums[10];
    const unsigned long long key = round->key;
    if (key == 0) return;                                          // wave-uniform (one address): no winner, no moments
    if (threadIdx.x < 10) sums[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t w = (0xFFFFFFFFu - (uint32_t)key) * pp.cand_stride;
    const PlaneSample pc = points[w];
    const pr_vec3 nc = normals[w];
    const uint32_t j = blockIdx.x * kPlaneThreads + threadIdx.x;
    uint64_t m[10];
#pragma unroll
    for (int e = 0; e < 10; ++e) m[e] = 0;
    if (j < n) {
        const PlaneSample p = points[j];
        const pr_vec3 mj = normals[j];
        if (labels[p.px] == 0 && planes::supports(pp.tau_mm, pp.cos_min, pc.x, pc.y, pc.z, nc.x, nc.y, nc.z, p.x, p.y, p.z, mj.x, mj.y, mj.z))
            planes::point_moments(p.x, p.y, p.z, m);
    }
#pragma unroll
    for (int e = 0; e < 10; ++e) {
        const unsigned long long v = wave_sum_u64(m[e]);
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&sums[e], v);
    }
    __syncthreads();
    if (threadIdx.x < 10 && sums[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long *>(&round->m[threadIdx.x]), sums[threadIdx.x]);
}

// ---- labels: full resolution, one pixel per thread; a sample dies with its pixel's label (the next round reads the label image) -----------------
__global__ __launch_bounds__(kPlaneThreads) void plane_label_kernel(const pr_plane_params pp, uint32_t k, float nx, float ny, float nz, float offset,
                                                                    const float *__restrict__ pcd, const float *__restrict__ normal, uint32_t n_px,
                                                                    uint8_t *__restrict__ labels, PlaneRound *__restrict__ round)
{
    const uint32_t i = blockIdx.x * kPlaneThreads + threadIdx.x;
    uint8_t lab = 0;
    if (i < n_px && labels[i] == 0) {
        lab = planes::pixel_label(pp, k, nx, ny, nz, offset, pcd[(size_t)i * 3], pcd[(size_t)i * 3 + 1], pcd[(size_t)i * 3 + 2], normal[(size_t)i * 3],
                                  normal[(size_t)i * 3 + 1], normal[(size_t)i * 3 + 2]);
        if (lab) labels[i] = lab;
    }
    const uint32_t n_lab = wave_sum_u32(lab == (uint8_t)k ? 1u : 0u), n_behind = wave_sum_u32(lab == (uint8_t)PR_PLANE_BEHIND ? 1u : 0u);
    if ((threadIdx.x & 63u) == 0) {
        if (n_lab) atomicAdd(&round->labelled, n_lab);
        if (n_behind) atomicAdd(&round->behind, n_behind);
    }
}

template <class T>
__global__ __launch_bounds__(kPlaneThreads) void plane_clear_depth_kernel(const uint8_t *__restrict__ labels, const T *depth_in, T *depth_out, uint32_t n_px)
{
    const uint32_t i = blockIdx.x * kPlaneThreads + threadIdx.x;   // (depth_out may be depth_in: a thread reads and writes its own pixel only)
    if (i < n_px) depth_out[i] = labels[i] == 0 ? depth_in[i] : (T)0;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
hipError_t launch_plane_sample_count(const float *pcd, const float *normal, uint32_t width, uint32_t height, uint32_t stride, uint32_t *row_count,
                                     uint32_t *row_off, hipStream_t s)
{
    const uint32_t gh = (height + stride - 1) / stride;
    hipLaunchKernelGGL(plane_sample_count_kernel, dim3(gh), dim3(64), 0, s, pcd, normal, width, stride, row_count);
    return launch_scan_counts(row_count, gh, row_off, nullptr, false, s);      // row_off[gh] = the total
}

hipError_t launch_plane_sample_emit(const float *pcd, const float *normal, uint32_t width, uint32_t height, uint32_t stride, const uint32_t *row_off,
                                    PlaneSample *points, pr_vec3 *normals, hipStream_t s)
{
    const uint32_t gh = (height + stride - 1) / stride;
    hipLaunchKernelGGL(plane_sample_emit_kernel, dim3(gh), dim3(64), 0, s, pcd, normal, width, stride, row_off, points, normals);
    return hipGetLastError();
}

hipError_t launch_plane_init(const float *pcd, uint32_t n_px, uint8_t *labels, PlaneRound *rounds, uint32_t n_rounds, uint32_t *support, uint32_t n_support,
                             hipStream_t s)
{
    hipLaunchKernelGGL(plane_init_kernel, dim3(cap_grid((n_px + kPlaneThreads - 1) / kPlaneThreads)), dim3(kPlaneThreads), 0, s, pcd, n_px, labels,
                       reinterpret_cast<uint32_t *>(rounds), n_rounds * (uint32_t)(sizeof(PlaneRound) / sizeof(uint32_t)), support, n_support);
    return hipGetLastError();
}

hipError_t launch_plane_round(const pr_plane_params &pp, const PlaneSample *points, const pr_vec3 *normals, uint32_t n, uint32_t n_cand, const uint8_t *labels,
                              uint32_t n_cus, uint32_t *support, PlaneRound *round, hipStream_t s)
{
    if (n == 0 || n_cand == 0) return hipSuccess;
    // about four workgroups per CU: the candidates fill grid.x, the sample range is split over grid.y in whole tiles
    const uint32_t gx = (n_cand + kPlaneThreads - 1) / kPlaneThreads, n_tiles = (n + kPlaneTile - 1) / kPlaneTile;
    const uint32_t want = (4 * (n_cus ? n_cus : 256u) + gx - 1) / gx, tiles_per_row = (n_tiles + want - 1) / want;
    const uint32_t rows = (n_tiles + tiles_per_row - 1) / tiles_per_row;      // every row starts inside the sample; the last may be short
    hipLaunchKernelGGL(plane_support_kernel, dim3(gx, rows), dim3(kPlaneThreads), 0, s, pp, points, normals, n, n_cand, labels, tiles_per_row, support);
    hipLaunchKernelGGL(plane_winner_kernel, dim3(1), dim3(kPlaneThreads), 0, s, (const uint32_t *)support, n_cand, round);
    hipLaunchKernelGGL(plane_moments_kernel, dim3((n + kPlaneThreads - 1) / kPlaneThreads), dim3(kPlaneThreads), 0, s, pp, points, normals, n, labels, round);
    return hipGetLastError();
}

hipError_t launch_plane_label(const pr_plane_params &pp, uint32_t k, const float plane[4], const float *pcd, const float *normal, uint32_t n_px, uint8_t *labels,
                              PlaneRound *round, hipStream_t s)
{
    hipLaunchKernelGGL(plane_label_kernel, dim3((n_px + kPlaneThreads - 1) / kPlaneThreads), dim3(kPlaneThreads), 0, s, pp, k, plane[0], plane[1], plane[2], plane[3], pcd,
                       normal, n_px, labels, round);
    return hipGetLastError();
}

hipError_t launch_plane_clear_depth(const uint8_t *labels, const void *depth_in, void *depth_out, bool depth_i32, uint32_t n_px, hipStream_t s)
{
    const dim3 grid((n_px + kPlaneThreads - 1) / kPlaneThreads);
    for_depth_type(depth_i32, [&](auto *tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(plane_clear_depth_kernel<T>, grid, dim3(kPlaneThreads), 0, s, labels, static_cast<const T *>(depth_in), static_cast<T *>(depth_out), n_px);
    });
    return hipGetLastError();
}

}  // namespace prk
