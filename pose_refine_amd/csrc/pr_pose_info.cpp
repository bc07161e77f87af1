// pr_pose_info.cpp -- pose observability: the driver of pose_info.hip's two launches (info_drive), pr_icp_information and its audit form, and the
// host-only covariance pr_info_covariance.  The fused entry points (pr_pose_information, _multi) live in pr_refine.cpp beside refine_core.
#include "pr_runtime.h"
#include "pose_info.h"

namespace prr {

// The hypotheses' records go in through the context's pinned block, pulled by a kernel; the eigen kernel stores its records straight into another:
// no copy or memset command on this path (see refine_core).  Everything runs on the context's own stream and workspaces.
int info_drive(const pr_vec3 *cloud_base, const uint32_t *start_h, const uint32_t *count_h, uint32_t P, const SceneSel &sc, const pr_robust &robust,
               const float *centers, const float *radii, pr_pose_info *info_host, pr_pose_eig *eig_host)
{
    constexpr uint32_t kMaxPerLaunch = 32768;                     // the hypothesis index is the y dimension of the pass' grid
    for (uint32_t p0 = 0; p0 < P; p0 += kMaxPerLaunch) {
        const uint32_t np = std::min(kMaxPerLaunch, P - p0);
        uint32_t max_n = 0;
        for (uint32_t i = 0; i < np; ++i) max_n = std::max(max_n, count_h[p0 + i]);
        const uint32_t nblk = std::max(1u, (max_n + prk::kInfoPointsPerBlock - 1) / prk::kInfoPointsPerBlock);
        const size_t b_info = sizeof(pr_pose_info) * (size_t)np, b_eig = eig_host ? sizeof(pr_pose_eig) * (size_t)np : 0;
        // kd-tree scenes with compact records: the product's search kernels (one PoseMeta per hypothesis behind the InfoMeta records, state kRun: no pending
        // update, so the search neither moves nor writes the cloud), then the pass over their winners.  Without such records: the per-lane walk.
        const bool nn_search = sc.kind == PR_SCENE_NN && sc.nn.rec32 && (sc.nn.stack_depth == 16 || sc.nn.stack_depth == 24) && max_n > 0 && max_n < (1u << 30);
        const size_t b_meta = (sizeof(prk::InfoMeta) * (size_t)np + 63) & ~(size_t)63, b_pose = nn_search ? sizeof(prk::PoseMeta) * (size_t)np : 0;
        PR_TRY(g->h_info_meta.ensure(b_meta + b_pose));
        PR_TRY(g->info_meta.ensure(b_meta + b_pose));
        PR_TRY(g->info_part.ensure(sizeof(double) * prk::kInfoStride * (size_t)nblk * np));
        PR_TRY(g->h_info_out.ensure(b_info + b_eig));
        prk::InfoMeta *hm = g->h_info_meta.as<prk::InfoMeta>();
        for (uint32_t i = 0; i < np; ++i) {
            prk::InfoMeta m{};
            m.start = start_h[p0 + i]; m.count = count_h[p0 + i];
            for (int a = 0; a < 3; ++a) m.c[a] = centers[3 * (size_t)(p0 + i) + a];
            m.rho = radii[p0 + i];
            hm[i] = m;
        }
        if (nn_search) {
            prk::PoseMeta *hp = reinterpret_cast<prk::PoseMeta *>(g->h_info_meta.as<unsigned char>() + b_meta);
            for (uint32_t i = 0; i < np; ++i) {
                std::memset(static_cast<void *>(&hp[i]), 0, sizeof(prk::PoseMeta));
                hp[i].start = start_h[p0 + i]; hp[i].count = count_h[p0 + i]; hp[i].state = count_h[p0 + i] ? prk::kRun : prk::kSkip;
            }
        }
        HIP_TRY(prk::launch_stage_words(g->h_info_meta.dev, g->info_meta.p, b_meta + b_pose, g->stream));
        const prk::InfoMeta *meta = g->info_meta.as<prk::InfoMeta>();
        double *part = g->info_part.as<double>();
        if (max_n > 0) {
            hipError_t e;
            if (nn_search) {
                size_t span = 0;
                for (uint32_t i = 0; i < np; ++i) span = std::max(span, (size_t)start_h[p0 + i] + count_h[p0 + i]);
                const NNLayout nl = nn_layout(span, np);
                PR_TRY(g->nn_prev.ensure(nl.bytes));
                prk::IcpBatch b{};
                b.cloud = const_cast<pr_vec3 *>(cloud_base);           // (kRun: read only)
                b.meta = reinterpret_cast<const prk::PoseMeta *>(g->info_meta.as<unsigned char>() + b_meta);
                nn_carve(b, g->nn_prev.as<uint32_t>(), nl);
                HIP_TRY(prk::launch_fill_i32(reinterpret_cast<int32_t *>(b.nn_qcount), (size_t)prk::kQCountStride * np, 0, g->stream));
                HIP_TRY(prk::launch_nn_search(b, sc.nn, np, max_n, (uint32_t)std::max(1, opt.nn_run), g->stream));
                const prk::SceneNNWinners w{ sc.nn.max_dist_diff, sc.nn.pts, sc.nn.normal, b.nn_prev };
                e = prk::launch_info_pass_nn_winners(cloud_base, meta, w, robust, nblk, np, part, g->stream);
            }
            else if (sc.kind == PR_SCENE_GRID) e = prk::launch_info_pass_grid(cloud_base, meta, sc.grid, robust, nblk, np, part, g->stream);
            else if (sc.kind == PR_SCENE_NN) e = prk::launch_info_pass_nn(cloud_base, meta, sc.nn, robust, nblk, np, part, g->stream);
            else if (sc.packed) e = prk::launch_info_pass_proj_packed(cloud_base, meta, sc.pk, robust, nblk, np, part, g->stream);
            else e = prk::launch_info_pass_proj_aos(cloud_base, meta, sc.aos, robust, nblk, np, part, g->stream);
            HIP_TRY(e);
        }
        pr_pose_info *d_info = g->h_info_out.dev_as<pr_pose_info>();
        pr_pose_eig *d_eig = eig_host ? reinterpret_cast<pr_pose_eig *>(g->h_info_out.dev_as<unsigned char>() + b_info) : nullptr;
        HIP_TRY(prk::launch_info_eigen(part, meta, nblk, np, d_info, d_eig, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        std::memcpy(info_host + p0, g->h_info_out.p, b_info);
        if (eig_host) std::memcpy(eig_host + p0, g->h_info_out.as<unsigned char>() + b_info, b_eig);
    }
    return PR_OK;
}

static const pr_robust kPlain{ PR_ROBUST_NONE, 0.0f, 0.0f, 0 };

static int icp_information_impl(const char *fn, const pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind, const void *scene,
                                bool want_packed, const pr_robust *robust, const float *centers, const float *radii, pr_pose_info *info_host, pr_pose_eig *eig_host)
{
    // every argument check before any device is touched
    if (robust) PR_TRY(robust_desc_ok(fn, robust));
    if (!offsets_host || (n_clouds && !info_host)) { set_error("%s: bad arguments", fn); return PR_ERR_INVALID; }
    if (n_clouds == 0) return PR_OK;
    PR_TRY(info_scene_ok(fn, scene_kind, scene));
    PR_TRY(info_center_radius_ok(fn, centers, radii, n_clouds));
    for (uint32_t i = 0; i < n_clouds; ++i)
        if (offsets_host[i + 1] < offsets_host[i]) { set_error("%s: offsets must be non-decreasing", fn); return PR_ERR_INVALID; }
    if (!clouds_dev && offsets_host[n_clouds] != offsets_host[0]) { set_error("%s: null cloud array", fn); return PR_ERR_INVALID; }
    PR_ENTER();
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    PR_TRY(make_scene(scene_kind, scene, want_packed, sc));
    std::vector<uint32_t> start(n_clouds), count(n_clouds);
    for (uint32_t i = 0; i < n_clouds; ++i) { start[i] = offsets_host[i]; count[i] = offsets_host[i + 1] - offsets_host[i]; }
    return info_drive(clouds_dev, start.data(), count.data(), n_clouds, sc, robust ? *robust : kPlain, centers, radii, info_host, eig_host);
}

}  // namespace prr

using namespace prr;

extern "C" {

int pr_icp_information(const pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind, const void *scene,
                       const pr_robust *robust_or_null, const float *centers_host, const float *radii_host, pr_pose_info *info_host,
                       pr_pose_eig *eig_host_or_null)
{
    return icp_information_impl("pr_icp_information", clouds_dev, offsets_host, n_clouds, scene_kind, scene, false, robust_or_null, centers_host, radii_host,
                                info_host, eig_host_or_null);
}

int pr_debug_icp_information(const pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind, const void *scene,
                             int want_packed, const pr_robust *robust_or_null, const float *centers_host, const float *radii_host,
                             pr_pose_info *info_host, pr_pose_eig *eig_host_or_null)
{
    return icp_information_impl("pr_debug_icp_information", clouds_dev, offsets_host, n_clouds, scene_kind, scene, want_packed != 0, robust_or_null, centers_host,
                                radii_host, info_host, eig_host_or_null);
}

int pr_info_covariance(const pr_pose_info *info, const pr_pose_eig *eig, double sigma, double min_ratio, double *cov21_out, uint32_t *rank_out,
                       double *sigma2_out)
{
    return info_covariance(info, eig, sigma, min_ratio, cov21_out, rank_out, sigma2_out);
}

}  // extern "C"
