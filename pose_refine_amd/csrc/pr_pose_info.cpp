// pr_pose_info.cpp -- pose observability: the driver of pose_info.hip's two launches (info_drive), pr_icp_information and its audit form, and the
// host-only covariance pr_info_covariance, and the host-only float64 pieces of a combined pose step: pr_info_combine, pr_info_eig (the eigen kernel's
// Jacobi, restated) and pr_info_step.  The fused entry points (pr_pose_information, _multi) live in pr_refine.cpp beside refine_core.
#include "pr_runtime.h"
#include "pose_info.h"
#include "jacobi.h"

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

// ---- host only: combine two records, decompose one, step a pose along its observable directions ---------------------------------------------------
static int info_combine(const pr_pose_info *a, double wa, const pr_pose_info *b, double wb, pr_pose_info *out)
{
    const char *fn = "pr_info_combine";
    if (!a || !b || !out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(wa) || !std::isfinite(wb) || wa < 0.0 || wb < 0.0) { set_error("%s: the weights must be finite and >= 0", fn); return PR_ERR_INVALID; }
    if (std::memcmp(a->c, b->c, sizeof a->c) != 0 || std::memcmp(&a->rho, &b->rho, sizeof a->rho) != 0) {
        set_error("%s: the records are about different centres or radii", fn); return PR_ERR_INVALID;
    }
    pr_pose_info o = *a;
    o.n_points = a->n_points + b->n_points; o.n_valid = a->n_valid + b->n_valid; o.n_zero_weight = a->n_zero_weight + b->n_zero_weight; o.reserved = 0;
    for (int i = 0; i < 21; ++i) o.H[i] = wa * a->H[i] + wb * b->H[i];
    for (int i = 0; i < 6; ++i) o.g[i] = wa * a->g[i] + wb * b->g[i];
    o.sum_w = wa * a->sum_w + wb * b->sum_w;
    o.sum_wr2 = wa * a->sum_wr2 + wb * b->sum_wr2;
    o.sum_r2 = a->sum_r2 + b->sum_r2;
    *out = o;
    return PR_OK;
}

// pose_info_eigen_kernel's decomposition (pose_info.hip): the solve is jacobi.h's, the ordering and the signs are below
static int info_eig(const pr_pose_info *info, pr_pose_eig *eig_out)
{
    if (!info || !eig_out) { set_error("pr_info_eig: bad arguments (info or eig_out is null)"); return PR_ERR_INVALID; }
    double A[6][6], V[6][6];
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { A[i][j] = info->H[k]; A[j][i] = info->H[k]; ++k; }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    const uint32_t sweeps = jacobi_eigen(A, V, PR_INFO_MAX_SWEEPS);
    double lam[6];
    for (int i = 0; i < 6; ++i) lam[i] = A[i][i];
    // ascending order by the kernel's fixed 12-comparator network (strict: equal eigenvalues keep their places)
    static const int net[12][2] = { { 1, 2 }, { 4, 5 }, { 0, 2 }, { 3, 5 }, { 0, 1 }, { 3, 4 }, { 2, 5 }, { 0, 3 }, { 1, 4 }, { 2, 4 }, { 1, 3 }, { 2, 3 } };
    for (const auto &ij : net) {
        const int i = ij[0], j = ij[1];
        if (!(lam[i] > lam[j])) continue;
        std::swap(lam[i], lam[j]);
        for (int r = 0; r < 6; ++r) std::swap(V[r][i], V[r][j]);
    }
    pr_pose_eig e;
    for (int c = 0; c < 6; ++c) {
        double big = V[0][c];
        for (int i = 1; i < 6; ++i) if (std::fabs(V[i][c]) > std::fabs(big)) big = V[i][c];
        const double sg = (big < 0.0) ? -1.0 : 1.0;
        e.lambda[c] = lam[c];
        for (int i = 0; i < 6; ++i) e.V[i * 6 + c] = sg * V[i][c];
    }
    e.sweeps = sweeps; e.reserved = 0;
    *eig_out = e;
    return PR_OK;
}

static int info_step(const pr_pose_info *info, const pr_pose_eig *eig, double min_ratio, const pr_mat4 *pose_in, pr_mat4 *pose_out, double *delta6_out,
                     uint32_t *rank_out)
{
    const char *fn = "pr_info_step";
    if (!info || !eig || !pose_in || !pose_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(min_ratio) || min_ratio < 0.0) { set_error("%s: min_ratio must be finite and >= 0", fn); return PR_ERR_INVALID; }
    uint32_t rank = 0;
    double delta[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int k = 0; k < 6; ++k) {
        const double l = eig->lambda[k];
        if (!(l > 0.0) || !(l > min_ratio * eig->lambda[5])) continue;
        ++rank;
        double dot = 0.0;
        for (int i = 0; i < 6; ++i) dot += eig->V[6 * i + k] * info->g[i];
        const double coef = dot / l;
        for (int i = 0; i < 6; ++i) delta[i] += eig->V[6 * i + k] * coef;
    }
    pr_mat4 out = *pose_in;
    if (rank > 0) {
        const double rho = (double)info->rho, c[3] = { (double)info->c[0], (double)info->c[1], (double)info->c[2] };
        const double th[3] = { delta[0] / rho, delta[1] / rho, delta[2] / rho };
        const double a2 = (th[0] * th[0] + th[1] * th[1]) + th[2] * th[2], a = std::sqrt(a2);
        double R[3][3] = { { 1.0, 0.0, 0.0 }, { 0.0, 1.0, 0.0 }, { 0.0, 0.0, 1.0 } };
        if (a > 0.0) {
            const double Kx[3][3] = { { 0.0, -th[2], th[1] }, { th[2], 0.0, -th[0] }, { -th[1], th[0], 0.0 } };
            const double A = std::sin(a) / a, B = (1.0 - std::cos(a)) / a2;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    const double k2 = (Kx[i][0] * Kx[0][j] + Kx[i][1] * Kx[1][j]) + Kx[i][2] * Kx[2][j];
                    R[i][j] += A * Kx[i][j] + B * k2;
                }
        }
        double tr[3];                                               // 1000 * (c - R c + t): metres about c to the pose's millimetres
        for (int i = 0; i < 3; ++i) tr[i] = 1000.0 * ((c[i] - ((R[i][0] * c[0] + R[i][1] * c[1]) + R[i][2] * c[2])) + delta[3 + i]);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) {
                double v = (R[i][0] * (double)pose_in->m[j] + R[i][1] * (double)pose_in->m[4 + j]) + R[i][2] * (double)pose_in->m[8 + j];
                if (j == 3) v += tr[i];
                out.m[4 * i + j] = (float)v;
            }
    }
    *pose_out = out;
    if (delta6_out) for (int i = 0; i < 6; ++i) delta6_out[i] = delta[i];
    if (rank_out) *rank_out = rank;
    return PR_OK;
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

int pr_info_combine(const pr_pose_info *a, double wa, const pr_pose_info *b, double wb, pr_pose_info *out) { return info_combine(a, wa, b, wb, out); }

int pr_info_eig(const pr_pose_info *info, pr_pose_eig *eig_out) { return info_eig(info, eig_out); }

int pr_info_step(const pr_pose_info *info, const pr_pose_eig *eig, double min_ratio, const pr_mat4 *pose_in, pr_mat4 *pose_out, double *delta6_out,
                 uint32_t *rank_out)
{
    return info_step(info, eig, min_ratio, pose_in, pose_out, delta6_out, rank_out);
}

}  // extern "C"
