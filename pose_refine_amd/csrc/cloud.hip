// cloud.hip -- scenes from point clouds (pr_cloud_*, include/pose_refine.h; no counterpart in the reference): the exact k nearest neighbours of every
// scene point over the scene's own kd-tree, the PCA normal formed from them, and the strided scene sample of the PPF vote
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the host twin (cloud.h is both).
//
// One lane per scene point runs the ordered stackless walk (cloud::knn_walk) that nn_walk_stackless and grid_build_kernel run at build time, with a
// bounded candidate list in place of the single best.  The list -- up to PR_KNN_MAX_K (d2, j) pairs per lane -- lives in LDS as [entry][lane]: the
// lanes of a wavefront address consecutive words of an entry (no bank conflict in either half), an insertion is a few ds_read / ds_write, and
// nothing is indexed by a variable in registers, so nothing goes to scratch.  k KiB per workgroup of 128 lanes.  The normal is formed in the SAME
// kernel from the list while it is still in LDS (no n x k round trip through global memory, no second launch); the walk dominates either way.
#include "pr_launch.h"
#include "cloud.h"

namespace prk {

namespace {

// the derived traversal arrays of a kd-tree scene (make_scene) as cloud::knn_walk's tree
struct DevTree {
    const int4 *__restrict__ topo;
    const float4 *__restrict__ bmin, *__restrict__ bmax, *__restrict__ pts;
    __device__ __forceinline__ cloud::Topo node(int c) const { const int4 t = topo[c]; return cloud::Topo{ t.x, t.y, t.z, t.w }; }
    __device__ __forceinline__ cloud::Box box(int c) const { const float4 a = bmin[c], b = bmax[c]; return cloud::Box{ { a.x, a.y, a.z }, { b.x, b.y, b.z } }; }
    __device__ __forceinline__ cloud::Point point(int i) const { const float4 p = pts[i]; return cloud::Point{ p.x, p.y, p.z }; }
};
// a lane's list in LDS: entry t at [t * kCloudThreads + lane]
struct LdsList {
    float *d2;
    uint32_t *idx;
    __device__ __forceinline__ float d(uint32_t t) const { return d2[t * kCloudThreads]; }
    __device__ __forceinline__ uint32_t j(uint32_t t) const { return idx[t * kCloudThreads]; }
    __device__ __forceinline__ void set(uint32_t t, float v, uint32_t i) { d2[t * kCloudThreads] = v; idx[t * kCloudThreads] = i; }
};

}  // namespace

// kNormals: the normal, the variation and the tally instead of the lists
template <bool kNormals>
__global__ __launch_bounds__(kCloudThreads) void cloud_knn_kernel(SceneNNDev tree, uint32_t n, pr_cloud_params cp, uint32_t *__restrict__ idx, float *__restrict__ d2,
                                                                  uint32_t *__restrict__ count, pr_vec3 *normal, float *__restrict__ variation,
                                                                  uint32_t *__restrict__ tally)
{
    extern __shared__ __align__(16) unsigned char cloud_lds[];   // k * kCloudThreads distances, then as many indices
    const uint32_t k = cp.k;
    LdsList list{ reinterpret_cast<float *>(cloud_lds) + threadIdx.x, reinterpret_cast<uint32_t *>(cloud_lds) + (size_t)k * kCloudThreads + threadIdx.x };
    const DevTree t{ tree.topo, tree.bmin, tree.bmax, tree.pts };
    const uint32_t i = blockIdx.x * kCloudThreads + threadIdx.x;
    const bool live = i < n;
    uint32_t m = 0;
    cloud::Point p{ 0.0f, 0.0f, 0.0f };
    if (live) {
        p = t.point((int)i);
        m = cloud::knn_walk(t, list, k, cp.r2, p.x, p.y, p.z);
    }
    if constexpr (!kNormals) {
        if (!live) return;
        for (uint32_t e = 0; e < k; ++e) {
            idx[(size_t)i * k + e] = e < m ? list.j(e) : (uint32_t)PR_KNN_NONE;
            if (d2) d2[(size_t)i * k + e] = e < m ? list.d(e) : 0.0f;
        }
        if (count) count[i] = m;
    } else {
        uint32_t status = 0xffffffffu;
        if (live) {
            const cloud::Normal r = cloud::normal_from_list(t, list, m, cp, p.x, p.y, p.z);
            normal[i] = pr_vec3{ r.n[0], r.n[1], r.n[2] };
            if (variation) variation[i] = r.variation;
            status = r.status;
        }
        if (tally) {                                             // one integer atomic per wavefront and status (exact in any order)
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) {
                const uint32_t cnt = (uint32_t)__popcll(__ballot(status == c));
                if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(tally + c, cnt);
            }
        }
    }
}

// ---- the scene sample of the PPF vote: one wavefront per chunk of kCloudChunk samples (wave_compact_count / wave_compact_place) ---------------
__device__ __forceinline__ bool cloud_sample_keep(const pr_vec3 *__restrict__ normal, size_t i)
{
    const pr_vec3 q = normal[i];
    return q.x != 0.0f || q.y != 0.0f || q.z != 0.0f;
}
__device__ __forceinline__ uint32_t cloud_chunk_samples(uint32_t n, uint32_t stride, uint32_t first)
{
    const uint32_t n_samples = (n - 1) / stride + 1, left = n_samples - first;
    return left < kCloudChunk ? left : kCloudChunk;
}
__global__ __launch_bounds__(64) void cloud_sample_count_kernel(const pr_vec3 *__restrict__ normal, uint32_t n, uint32_t stride, uint32_t *__restrict__ chunk_count)
{
    const uint32_t first = blockIdx.x * kCloudChunk;
    const uint32_t kept = wave_compact_count(cloud_chunk_samples(n, stride, first), threadIdx.x, [&](uint32_t c) { return cloud_sample_keep(normal, (size_t)(first + c) * stride); });
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = kept;
}
__global__ __launch_bounds__(64) void cloud_sample_emit_kernel(const pr_vec3 *__restrict__ pcd, const pr_vec3 *__restrict__ normal, uint32_t n, uint32_t stride,
                                                               const uint32_t *__restrict__ chunk_off, pr_vec3 *__restrict__ points, pr_vec3 *__restrict__ normals)
{
    const uint32_t first = blockIdx.x * kCloudChunk;
    wave_compact_place(cloud_chunk_samples(n, stride, first), threadIdx.x, chunk_off[blockIdx.x], [&](uint32_t c) { return cloud_sample_keep(normal, (size_t)(first + c) * stride); },
                       [&](uint32_t c, bool kept, uint32_t pos) {
                           if (!kept || pos >= PR_PPF_MAX_SCENE_POINTS) return;
                           const size_t i = (size_t)(first + c) * stride;
                           const pr_vec3 p = pcd[i];
                           points[pos] = pr_vec3{ p.x * 1000.0f, p.y * 1000.0f, p.z * 1000.0f };
                           normals[pos] = normal[i];
                       });
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
hipError_t launch_cloud_knn(const SceneNNDev &tree, uint32_t n, const pr_cloud_params &cp, uint32_t *idx, float *d2, uint32_t *count, pr_vec3 *normal,
                            float *variation, uint32_t *tally, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t grid = (n + kCloudThreads - 1) / kCloudThreads, lds = cp.k * kCloudThreads * (uint32_t)(sizeof(float) + sizeof(uint32_t));      // <= 32 KiB
    if (normal) hipLaunchKernelGGL(cloud_knn_kernel<true>, dim3(grid), dim3(kCloudThreads), lds, s, tree, n, cp, idx, d2, count, normal, variation, tally);
    else hipLaunchKernelGGL(cloud_knn_kernel<false>, dim3(grid), dim3(kCloudThreads), lds, s, tree, n, cp, idx, d2, count, normal, variation, tally);
    return hipGetLastError();
}

static uint32_t cloud_chunks(uint32_t n, uint32_t stride) { return ((n - 1) / stride + 1 + kCloudChunk - 1) / kCloudChunk; }

hipError_t launch_cloud_sample_count(const pr_vec3 *normal, uint32_t n, uint32_t stride, uint32_t *chunk_count, uint32_t *chunk_off, hipStream_t s)
{
    const uint32_t n_chunks = cloud_chunks(n, stride);
    hipLaunchKernelGGL(cloud_sample_count_kernel, dim3(n_chunks), dim3(64), 0, s, normal, n, stride, chunk_count);
    return launch_scan_counts(chunk_count, n_chunks, chunk_off, nullptr, false, s);      // chunk_off[n_chunks] = the total
}

hipError_t launch_cloud_sample_emit(const pr_vec3 *pcd, const pr_vec3 *normal, uint32_t n, uint32_t stride, const uint32_t *chunk_off, pr_vec3 *points,
                                    pr_vec3 *normals, hipStream_t s)
{
    hipLaunchKernelGGL(cloud_sample_emit_kernel, dim3(cloud_chunks(n, stride)), dim3(64), 0, s, pcd, normal, n, stride, chunk_off, points, normals);
    return hipGetLastError();
}

}  // namespace prk
