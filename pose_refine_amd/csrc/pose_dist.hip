// pose_dist.hip -- how far apart two poses are: the displacement of the model's points between them (mean, maximum, maximum in the image), each
// minimised over a set of symmetry transforms (pr_pose_distance; the definition is in include/pose_refine.h)
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "pr_launch.h"

namespace prk {

constexpr uint32_t kPoseDistThreads = 256;
static_assert(kPoseDistChunk == kPoseDistThreads, "pose_dist_kernel: one staged point per thread");

// what one workgroup row (blockIdx.y: a run of point chunks) leaves for one candidate: 16 bytes, [row][candidate]
struct alignas(16) PoseDistPartial { unsigned long long sum; float maxd, maxp; };
static_assert(sizeof(PoseDistPartial) == 16, "PoseDistPartial: one 16-byte word");

// rows 0..2 of a 4x4 applied to a point, the header's three-term form: ((m0*x + m1*y) + m2*z) + m3
__device__ __forceinline__ float row_apply(const float *m, float x, float y, float z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }

// Lanes on candidates.  Candidate c of a launch = (pair pair0 + c / n_k, symmetry c % n_k); its lane holds the 12 coefficients of D = A S_k - B
// (and, kProj, of A S_k and B) in registers for the whole point range of its workgroup row.  The points go through LDS, kPoseDistChunk at a
// time, and every lane reads the same address in the same instruction (a broadcast: no bank conflict); the accumulators are per lane -- an
// exact integer sum and two maxima -- so nothing crosses lanes and the result does not depend on how grid.y splits the points.
// as_rows: rows 0..2 of A_i S_k in DOUBLE, [i * n_k + k][12]; b_rows: rows 0..2 of B_j in float, [j][12].  D and the float32 A S_k are rounded
// from the doubles here, once.  all_pairs: pair p = (p / n_b, p % n_b), else (p, p).
template <bool kProj>
__global__ __launch_bounds__(kPoseDistThreads) void pose_dist_kernel(const pr_vec3 *__restrict__ points, uint32_t n_points, uint32_t chunks_per_row,
                                                                     const double *__restrict__ as_rows, const float *__restrict__ b_rows, uint32_t n_b,
                                                                     uint32_t n_k, uint32_t pair0, uint32_t n_cand, uint32_t all_pairs, PoseDistCamera cam,
                                                                     PoseDistPartial *__restrict__ part)
{
    __shared__ float4 tile[kPoseDistChunk];
    const uint32_t c = blockIdx.x * kPoseDistThreads + threadIdx.x;
    const bool active = c < n_cand;                              // (a lane without a candidate still stages points and meets the barriers)
    float D[12], As[12], B[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) D[e] = As[e] = B[e] = 0.0f;
    if (active) {
        const uint32_t pl = c / n_k, k = c - pl * n_k, p = pair0 + pl;
        const uint32_t ia = all_pairs ? p / n_b : p, ib = all_pairs ? p - ia * n_b : p;
        const double *as = as_rows + ((size_t)ia * n_k + k) * 12;
        const float *b = b_rows + (size_t)ib * 12;
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            const double a = as[e];
            B[e] = b[e];
            As[e] = (float)a;
            D[e] = (float)(a - (double)B[e]);
        }
    }
    unsigned long long sum = 0;
    float maxd = 0.0f, maxp = 0.0f;
    bool behind = false;
    const uint32_t first = blockIdx.y * chunks_per_row * kPoseDistChunk;
    const uint32_t span = chunks_per_row * kPoseDistChunk;
    const uint32_t last = (n_points - first < span) ? n_points : first + span;          // first < n_points: the launcher makes no empty row
    for (uint32_t base = first; base < last; base += kPoseDistChunk) {
        if (base != first) __syncthreads();                        // every lane is done with the chunk before
        const uint32_t n = (last - base < kPoseDistChunk) ? last - base : kPoseDistChunk;
        if (threadIdx.x < n) {
            const pr_vec3 v = points[base + threadIdx.x];
            tile[threadIdx.x] = make_float4(v.x, v.y, v.z, 0.0f);
        }
        __syncthreads();
        if (!active) continue;
        for (uint32_t i = 0; i < n; ++i) {
            const float4 v = tile[i];
            const float d0 = row_apply(D, v.x, v.y, v.z), d1 = row_apply(D + 4, v.x, v.y, v.z), d2 = row_apply(D + 8, v.x, v.y, v.z);
            const float sq = (d0 * d0 + d1 * d1) + d2 * d2;
            const float q = rintf(sqrtf(sq) * 65536.0f);
            sum += (q < 1099511627776.0f) ? (unsigned long long)q : (1ull << 40);       // (a NaN counts as saturated)
            maxd = (sq > maxd) ? sq : maxd;
            if (kProj) {
                const float ax = row_apply(As, v.x, v.y, v.z), ay = row_apply(As + 4, v.x, v.y, v.z), az = row_apply(As + 8, v.x, v.y, v.z);
                const float bx = row_apply(B, v.x, v.y, v.z), by = row_apply(B + 4, v.x, v.y, v.z), bz = row_apply(B + 8, v.x, v.y, v.z);
                const bool out = az <= 0.0f || bz <= 0.0f;
                behind = behind || out;
                const float ua = cam.fx * ax / az + cam.cx, wa = cam.fy * ay / az + cam.cy;
                const float ub = cam.fx * bx / bz + cam.cx, wb = cam.fy * by / bz + cam.cy;
                const float du = ua - ub, dw = wa - wb;
                const float pp = out ? 0.0f : du * du + dw * dw;
                maxp = (pp > maxp) ? pp : maxp;
            }
        }
    }
    if (active) {
        PoseDistPartial r;
        r.sum = sum; r.maxd = maxd; r.maxp = behind ? __int_as_float(0x7f800000) : maxp;
        part[(size_t)blockIdx.y * n_cand + c] = r;
    }
}

hipError_t launch_pose_dist(const pr_vec3 *points, uint32_t n_points, const double *as_rows, const float *b_rows, uint32_t n_b, uint32_t n_k,
                            uint32_t pair0, uint32_t n_pairs, bool all_pairs, const PoseDistCamera *cam, uint32_t n_rows, uint32_t chunks_per_row,
                            void *partials, hipStream_t s)
{
    const uint32_t n_cand = n_pairs * n_k;
    if (n_cand == 0 || n_points == 0) return hipSuccess;
    // every row starts inside the point range, and the rows cover it
    if (n_rows == 0 || chunks_per_row == 0 || (uint64_t)(n_rows - 1) * chunks_per_row * kPoseDistChunk >= n_points ||
        (uint64_t)n_rows * chunks_per_row * kPoseDistChunk < n_points) return hipErrorInvalidValue;
    const dim3 grid((n_cand + kPoseDistThreads - 1) / kPoseDistThreads, n_rows);
    const PoseDistCamera none{ 0.0f, 0.0f, 0.0f, 0.0f };
    if (cam)
        hipLaunchKernelGGL(pose_dist_kernel<true>, grid, dim3(kPoseDistThreads), 0, s, points, n_points, chunks_per_row, as_rows, b_rows, n_b, n_k, pair0, n_cand,
                           all_pairs ? 1u : 0u, *cam, static_cast<PoseDistPartial *>(partials));
    else
        hipLaunchKernelGGL(pose_dist_kernel<false>, grid, dim3(kPoseDistThreads), 0, s, points, n_points, chunks_per_row, as_rows, b_rows, n_b, n_k, pair0, n_cand,
                           all_pairs ? 1u : 0u, none, static_cast<PoseDistPartial *>(partials));
    return hipGetLastError();
}

// One lane per pair: the rows of every candidate folded (sums added, maxima taken), then the three minima over the candidates, each with the
// lowest k that attains it.  One writer per record, no atomics; the record leaves as two 16-byte words.
__global__ __launch_bounds__(256) void pose_dist_combine_kernel(const PoseDistPartial *__restrict__ part, uint32_t n_rows, uint32_t n_pairs, uint32_t n_k,
                                                                uint32_t n_points, uint32_t with_proj, uint4 *__restrict__ records)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const size_t n_cand = (size_t)n_pairs * n_k;
    unsigned long long best_sum = 0;
    float best_d = 0.0f, best_p = 0.0f;
    uint32_t k_sum = 0, k_d = 0, k_p = 0;
    for (uint32_t k = 0; k < n_k; ++k) {
        unsigned long long sum = 0;
        float maxd = 0.0f, maxp = 0.0f;
        for (uint32_t r = 0; r < n_rows; ++r) {
            const PoseDistPartial v = part[(size_t)r * n_cand + (size_t)p * n_k + k];
            sum += v.sum;
            maxd = (v.maxd > maxd) ? v.maxd : maxd;
            maxp = (v.maxp > maxp) ? v.maxp : maxp;
        }
        if (k == 0 || sum < best_sum) { best_sum = sum; k_sum = k; }
        if (k == 0 || maxd < best_d) { best_d = maxd; k_d = k; }
        if (k == 0 || maxp < best_p) { best_p = maxp; k_p = k; }
    }
    if (!with_proj) { best_p = 0.0f; k_p = 0; }
    records[2 * (size_t)p] = make_uint4((uint32_t)best_sum, (uint32_t)(best_sum >> 32), __float_as_uint(best_d), __float_as_uint(best_p));
    records[2 * (size_t)p + 1] = make_uint4(k_sum | (k_d << 16), k_p, n_points, 0u);
}

hipError_t launch_pose_dist_combine(const void *partials, uint32_t n_rows, uint32_t n_pairs, uint32_t n_k, uint32_t n_points, bool with_proj,
                                    pr_pose_dist *records, hipStream_t s)
{
    static_assert(sizeof(pr_pose_dist) == 32 && offsetof(pr_pose_dist, max_disp_sq) == 8 && offsetof(pr_pose_dist, sym_sum) == 16 &&
                  offsetof(pr_pose_dist, sym_proj) == 20 && offsetof(pr_pose_dist, n_points) == 24, "pr_pose_dist: two 16-byte words");
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(pose_dist_combine_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, s, static_cast<const PoseDistPartial *>(partials), n_rows, n_pairs, n_k,
                       n_points, with_proj ? 1u : 0u, reinterpret_cast<uint4 *>(records));
    return hipGetLastError();
}

}  // namespace prk
