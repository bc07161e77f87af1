// pose_info.h -- what pose_info.hip (the information pass and the eigen kernel) shares with its host driver (pr_pose_info.cpp)
#pragma once
#include "pr_internal.h"

namespace prk {

constexpr uint32_t kInfoSums           = 30;                      // H[21], g[6], sum_w, sum_wr2, sum_r2 (pr_pose_info's order)
constexpr uint32_t kInfoStride         = 32;                      // doubles per partial: the sums, then one slot holding the two uint32 counters, then a spare
constexpr uint32_t kInfoSteps          = 2;                       // 1024-point steps per workgroup
constexpr uint32_t kInfoPointsPerBlock = kInfoSteps * kPointsPerStep;
constexpr uint32_t kInfoMaxSweeps      = 16;                      // PR_INFO_MAX_SWEEPS

// one hypothesis of an information launch: its cloud (points relative to the launch's cloud base), centre and radius
struct alignas(32) InfoMeta { uint32_t start, count; float c[3], rho; uint32_t pad[2]; };
static_assert(sizeof(InfoMeta) == 32, "InfoMeta: two 16-byte words");
static_assert(kInfoMaxSweeps == PR_INFO_MAX_SWEEPS, "the header states the sweep cap");

// partial: [n_poses][nblk][kInfoStride] doubles; nblk = blocks of kInfoPointsPerBlock points the largest cloud has (at least 1)
hipError_t launch_info_pass_proj_aos(const pr_vec3 *cloud, const InfoMeta *meta, const SceneProjAoS &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s);
hipError_t launch_info_pass_proj_packed(const pr_vec3 *cloud, const InfoMeta *meta, const SceneProjPacked &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s);
hipError_t launch_info_pass_nn(const pr_vec3 *cloud, const InfoMeta *meta, const SceneNNDev &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s);
// ... after launch_nn_search has left the winners of every cloud point in sc.winner (indexed like the cloud)
hipError_t launch_info_pass_nn_winners(const pr_vec3 *cloud, const InfoMeta *meta, const SceneNNWinners &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s);
hipError_t launch_info_pass_grid(const pr_vec3 *cloud, const InfoMeta *meta, const SceneGridDev &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s);
// the partials added in block order into info[n_poses]; eig (or null): the Jacobi decomposition of each
hipError_t launch_info_eigen(const double *partial, const InfoMeta *meta, uint32_t nblk, uint32_t n_poses, pr_pose_info *info, pr_pose_eig *eig, hipStream_t s);

}  // namespace prk
