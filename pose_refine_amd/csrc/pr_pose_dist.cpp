// pr_pose_dist.cpp -- pr_pose_distance: the candidates' matrices in double on the host, the launches of pose_dist.hip, the records back
#include "pr_runtime.h"

namespace prr {

// rows 0..2 of A * S in double, every entry summed in mat4_mul_impl's order (pr_solver.inl): acc = 0, += a3 s3, += a2 s2, += a1 s1, += a0 s0.
// The products of two float32 are exact in double; only the sums round.
static void mat_rows_d(const float *A, const float *S, double *out12)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double acc = 0.0;
            acc += (double)A[i * 4 + 3] * (double)S[12 + j];
            acc += (double)A[i * 4 + 2] * (double)S[8 + j];
            acc += (double)A[i * 4 + 1] * (double)S[4 + j];
            acc += (double)A[i * 4 + 0] * (double)S[j];
            out12[i * 4 + j] = acc;
        }
}

// One checked call with n_pairs > 0.  The matrices go in through the context's pinned block, pulled by a kernel; the records come back through
// another, stored by a kernel: no copy or memset command on this path (see refine_core).  Everything runs on the context's own stream and
// workspaces, which no asynchronous slot owns.
int pose_distance_core(const pr_vec3 *points_dev, uint32_t n_points, const pr_mat4 *a, uint32_t n_a, const pr_mat4 *b, uint32_t n_b, bool all_pairs,
                       const pr_mat4 *syms, uint32_t n_syms, const float *K, uint32_t n_pairs, pr_pose_dist *out)
{
    const uint32_t n_k = n_syms ? n_syms : 1;
    pr_mat4 eye;
    identity16(eye.m);
    if (!n_syms) syms = &eye;
    const size_t as_bytes = sizeof(double) * 12 * (size_t)n_a * n_k, b_bytes = sizeof(float) * 12 * (size_t)n_b;      // multiples of 16 both
    PR_TRY(g->h_pd_mats.ensure(as_bytes + b_bytes));
    PR_TRY(g->pd_mats.ensure(as_bytes + b_bytes));
    double *as_h = g->h_pd_mats.as<double>();
    float *b_h = reinterpret_cast<float *>(g->h_pd_mats.as<unsigned char>() + as_bytes);
    for (uint32_t i = 0; i < n_a; ++i)
        for (uint32_t k = 0; k < n_k; ++k) mat_rows_d(a[i].m, syms[k].m, as_h + ((size_t)i * n_k + k) * 12);
    for (uint32_t j = 0; j < n_b; ++j) std::memcpy(b_h + (size_t)j * 12, b[j].m, sizeof(float) * 12);
    HIP_TRY(prk::launch_stage_words(g->h_pd_mats.dev, g->pd_mats.p, as_bytes + b_bytes, g->stream));
    const double *as_d = g->pd_mats.as<double>();
    const float *b_d = reinterpret_cast<const float *>(g->pd_mats.as<unsigned char>() + as_bytes);
    const prk::PoseDistCamera cam{ K ? K[0] : 0.0f, K ? K[2] : 0.0f, K ? K[4] : 0.0f, K ? K[5] : 0.0f };

    const uint32_t n_chunks = (n_points + prk::kPoseDistChunk - 1) / prk::kPoseDistChunk;
    const uint32_t batch = std::max<uint32_t>(1, PR_POSE_DIST_BATCH / n_k);
    for (uint32_t p0 = 0; p0 < n_pairs; p0 += batch) {
        const uint32_t np = std::min(batch, n_pairs - p0), n_cand = np * n_k;
        // few candidates: the point range is split over workgroup rows until the launch has about PR_POSE_DIST_GROUPS workgroups
        const uint32_t wg_x = (n_cand + 255) / 256;
        const uint32_t want_rows = std::min(n_chunks, std::max<uint32_t>(1, (PR_POSE_DIST_GROUPS + wg_x - 1) / wg_x));
        const uint32_t per_row = (n_chunks + want_rows - 1) / want_rows, n_rows = (n_chunks + per_row - 1) / per_row;
        PR_TRY(g->pd_part.ensure((size_t)16 * n_rows * n_cand));
        PR_TRY(g->pd_rec.ensure(sizeof(pr_pose_dist) * np));
        PR_TRY(g->h_pd_rec.ensure(sizeof(pr_pose_dist) * np));
        HIP_TRY(prk::launch_pose_dist(points_dev, n_points, as_d, b_d, n_b, n_k, p0, np, all_pairs, K ? &cam : nullptr, n_rows, per_row, g->pd_part.p, g->stream));
        HIP_TRY(prk::launch_pose_dist_combine(g->pd_part.p, n_rows, np, n_k, n_points, K != nullptr, g->pd_rec.as<pr_pose_dist>(), g->stream));
        HIP_TRY(prk::launch_copy_words32(g->pd_rec.p, g->h_pd_rec.dev, (uint32_t)(sizeof(pr_pose_dist) / sizeof(uint32_t)) * np, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        std::memcpy(out + p0, g->h_pd_rec.p, sizeof(pr_pose_dist) * np);
    }
    return PR_OK;
}

}  // namespace prr

using namespace prr;

extern "C" {

int pr_pose_distance(const pr_vec3 *points_dev, uint32_t n_points, const pr_mat4 *a_host, uint32_t n_a, const pr_mat4 *b_host, uint32_t n_b,
                     int all_pairs, const pr_mat4 *syms_host, uint32_t n_syms, const float K[9], pr_pose_dist *out_host)
{
    uint64_t n_pairs = 0;
    PR_TRY(pose_dist_args_ok(points_dev, n_points, a_host, n_a, b_host, n_b, all_pairs, syms_host, n_syms, K, out_host, &n_pairs));      // before any device use
    if (n_pairs == 0) return PR_OK;
    PR_ENTER();
    return pose_distance_core(points_dev, n_points, a_host, n_a, b_host, n_b, all_pairs != 0, syms_host, n_syms, K, (uint32_t)n_pairs, out_host);
}

}  // extern "C"
