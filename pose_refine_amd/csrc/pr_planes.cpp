// pr_planes.cpp -- pr_plane_* / pr_scene_planes_*: the parameters, the refit from the integer moments (128-bit scatter matrix, 3 x 3 Jacobi), the
// host twin of the peel and the launches of planes.hip
#include <vector>

#include "pr_runtime.h"
#include "frame_stage.h"
#include "planes.h"
#include "jacobi.h"

namespace prr {

// a parameter block as a caller hands it over: pr_plane_describe's rules.  No HIP call in here.
static int plane_params_ok(const char *fn, const pr_plane_params *pp)
{
    if (!pp) { set_error("%s: null pr_plane_params", fn); return PR_ERR_INVALID; }
    if (pp->stride == 0 || pp->stride > PR_PPF_MAX_STRIDE) { set_error("%s: pr_plane_params: stride must be 1 .. PR_PPF_MAX_STRIDE = %d (got %u)", fn, PR_PPF_MAX_STRIDE, pp->stride); return PR_ERR_INVALID; }
    if (pp->cand_stride == 0) { set_error("%s: pr_plane_params: cand_stride must not be 0", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(pp->tau_mm) || pp->tau_mm < 0.0f || !std::isfinite(pp->label_tau_mm) || pp->label_tau_mm < 0.0f) {
        set_error("%s: pr_plane_params: tau_mm and label_tau_mm must be finite and >= 0 (got %g, %g)", fn, (double)pp->tau_mm, (double)pp->label_tau_mm); return PR_ERR_INVALID;
    }
    if (!(pp->cos_min == -2.0f || (pp->cos_min >= -1.0f && pp->cos_min <= 1.0f))) { set_error("%s: pr_plane_params: cos_min must be -2 (off) or in [-1, 1] (got %g)", fn, (double)pp->cos_min); return PR_ERR_INVALID; }
    if (pp->min_support < 3) { set_error("%s: pr_plane_params: min_support must be at least 3 (got %u)", fn, pp->min_support); return PR_ERR_INVALID; }
    if (pp->n_planes == 0 || pp->n_planes > PR_PLANE_MAX_PLANES) { set_error("%s: pr_plane_params: n_planes must be 1 .. PR_PLANE_MAX_PLANES = %d (got %u)", fn, PR_PLANE_MAX_PLANES, pp->n_planes); return PR_ERR_INVALID; }
    if (pp->drop_behind > 1) { set_error("%s: pr_plane_params: drop_behind must be 0 or 1", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
// the two caps, with the entry point's name in the message
static int sample_caps_ok(const char *fn, const pr_plane_params *pp, uint32_t n, uint32_t *n_cand)
{
    if (n > PR_PLANE_MAX_SAMPLES) { set_error("%s: %u samples at stride %u, at most PR_PLANE_MAX_SAMPLES = %d (raise the stride)", fn, n, pp->stride, PR_PLANE_MAX_SAMPLES); return PR_ERR_INVALID; }
    *n_cand = n ? (n - 1) / pp->cand_stride + 1 : 0;
    if (*n_cand > PR_PLANE_MAX_CANDIDATES) { set_error("%s: %u candidates at cand_stride %u, at most PR_PLANE_MAX_CANDIDATES = %d (raise cand_stride)", fn, *n_cand, pp->cand_stride, PR_PLANE_MAX_CANDIDATES); return PR_ERR_INVALID; }
    return PR_OK;
}

struct PlaneFit { double n[3], offset, rms, eig[3]; };
// false: fewer than 3 points, an all-zero scatter matrix or an eigenvector without a length (the reason in *why)
static bool plane_fit(const int64_t m[10], PlaneFit *out, const char **why)
{
    if (m[0] < 3) { *why = "fewer than 3 points"; return false; }
    const __int128 n = m[0], S[3] = { m[1], m[2], m[3] };
    const __int128 SS[3][3] = { { m[4], m[5], m[6] }, { m[5], m[7], m[8] }, { m[6], m[8], m[9] } };
    double A[3][3], V[3][3];
    bool any = false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const __int128 c = n * SS[i][j] - S[i] * S[j];
            any = any || c != 0;
            A[i][j] = (double)c;
            V[i][j] = (i == j) ? 1.0 : 0.0;
        }
    if (!any) { *why = "an all-zero scatter matrix (the points coincide)"; return false; }
    (void)jacobi_eigen(A, V, PR_PLANE_MAX_SWEEPS);
    int lo = 0;
    for (int i = 1; i < 3; ++i) if (A[i][i] < A[lo][lo]) lo = i;
    const double vx = V[0][lo], vy = V[1][lo], vz = V[2][lo];
    const double len = std::sqrt((vx * vx + vy * vy) + vz * vz);
    if (!(len > 0.0) || !std::isfinite(len)) { *why = "an eigenvector without a length"; return false; }
    double nu[3] = { vx / len, vy / len, vz / len };
    const double nd = (double)m[0];
    double offset = ((nu[0] * (double)m[1] + nu[1] * (double)m[2]) + nu[2] * (double)m[3]) / nd / 16.0;
    const double first = nu[0] != 0.0 ? nu[0] : (nu[1] != 0.0 ? nu[1] : nu[2]);
    if (offset > 0.0 || (offset == 0.0 && first > 0.0)) { nu[0] = -nu[0]; nu[1] = -nu[1]; nu[2] = -nu[2]; offset = -offset; }
    out->n[0] = nu[0]; out->n[1] = nu[1]; out->n[2] = nu[2]; out->offset = offset;
    out->rms = std::sqrt(std::fmax(A[lo][lo], 0.0)) / nd / 16.0;
    out->eig[0] = A[lo][lo]; out->eig[1] = A[lo == 0 ? 1 : 0][lo == 0 ? 1 : 0]; out->eig[2] = A[lo == 2 ? 1 : 2][lo == 2 ? 1 : 2];
    return true;
}
// a round's record to the caller's plane (labelled / behind follow once the label pass has run); false: the peel ends here
static bool round_plane(const pr_plane_params *pp, uint64_t key, const uint64_t moments[10], pr_plane *out, int64_t *moments_out)
{
    const uint32_t support = (uint32_t)(key >> 32);
    if (key == 0 || support < pp->min_support) return false;
    int64_t m[10];
    for (int e = 0; e < 10; ++e) m[e] = (int64_t)moments[e];
    PlaneFit f;
    const char *why = "";
    if (!plane_fit(m, &f, &why)) return false;
    std::memset(out, 0, sizeof *out);
    out->normal[0] = (float)f.n[0]; out->normal[1] = (float)f.n[1]; out->normal[2] = (float)f.n[2]; out->offset_mm = (float)f.offset;
    out->candidate = 0xFFFFFFFFu - (uint32_t)key; out->support = support; out->rms_mm = (float)f.rms;
    if (moments_out) std::memcpy(moments_out, m, sizeof m);
    return true;
}

}  // namespace prr

using namespace prr;

extern "C" {

int pr_plane_describe(uint32_t stride, uint32_t cand_stride, float tau_mm, float label_tau_mm, float cos_min, uint32_t min_support, uint32_t n_planes,
                      int drop_behind, pr_plane_params *out)
{
    const char *fn = "pr_plane_describe";
    if (!out) { set_error("%s: null out", fn); return PR_ERR_INVALID; }
    const pr_plane_params pp = { stride, cand_stride, tau_mm, label_tau_mm, cos_min, min_support, n_planes, drop_behind ? 1u : 0u };
    PR_TRY(plane_params_ok(fn, &pp));
    *out = pp;
    return PR_OK;
}

int pr_plane_from_moments(const int64_t moments[10], double normal_out[3], double *offset_mm_out, double *rms_mm_out, double eig_out[3])
{
    const char *fn = "pr_plane_from_moments";
    if (!moments || !normal_out || !offset_mm_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PlaneFit f;
    const char *why = "";
    if (!plane_fit(moments, &f, &why)) { set_error("%s: %s", fn, why); return PR_ERR_INVALID; }
    for (int i = 0; i < 3; ++i) { normal_out[i] = f.n[i]; if (eig_out) eig_out[i] = f.eig[i]; }
    *offset_mm_out = f.offset;
    if (rms_mm_out) *rms_mm_out = f.rms;
    return PR_OK;
}

int pr_scene_planes_host(const float *pcd, const float *normal, const void *depth, int depth_is_i32, size_t width, size_t height,
                         const pr_plane_params *params, uint8_t *labels_out, void *depth_out, pr_plane *planes_out, int64_t *moments_out,
                         uint32_t *support_out, uint32_t *n_found)
{
    const char *fn = "pr_scene_planes_host";
    PR_TRY(plane_params_ok(fn, params));
    if (!pcd || !normal || !labels_out || !planes_out || !n_found || (depth_out && !depth)) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(frame_ok(fn, width, height));
    const pr_plane_params pp = *params;
    const size_t n_px = width * height;
    std::vector<prk::PlaneSample> pts;
    std::vector<pr_vec3> nrm;
    for (size_t y = 0; y < height; y += pp.stride)
        for (size_t x = 0; x < width; x += pp.stride) {
            const size_t px = y * width + x;
            if (!planes::sample_keep(pcd, normal, px)) continue;
            pts.push_back(prk::PlaneSample{ pcd[px * 3] * 1000.0f, pcd[px * 3 + 1] * 1000.0f, pcd[px * 3 + 2] * 1000.0f, (uint32_t)px });
            nrm.push_back(pr_vec3{ normal[px * 3], normal[px * 3 + 1], normal[px * 3 + 2] });
        }
    const uint32_t n = (uint32_t)pts.size();
    uint32_t n_cand = 0;
    PR_TRY(sample_caps_ok(fn, &pp, n, &n_cand));
    *n_found = 0;
    for (size_t i = 0; i < n_px; ++i) labels_out[i] = pcd[i * 3 + 2] > 0.0f ? (uint8_t)0 : (uint8_t)PR_PLANE_NO_DEPTH;
    if (support_out) std::memset(support_out, 0, sizeof(uint32_t) * (size_t)pp.n_planes * PR_PLANE_MAX_CANDIDATES);
    std::vector<uint32_t> support_row(n_cand);
    for (uint32_t k = 0; k < pp.n_planes && n > 0; ++k) {
        uint64_t key = 0;
        for (uint32_t c = 0; c < n_cand; ++c) {
            const prk::PlaneSample &pc = pts[(size_t)c * pp.cand_stride];
            const pr_vec3 &nc = nrm[(size_t)c * pp.cand_stride];
            uint32_t count = 0;
            if (labels_out[pc.px] == 0)
                for (uint32_t j = 0; j < n; ++j)
                    count += (labels_out[pts[j].px] == 0 && planes::supports(pp.tau_mm, pp.cos_min, pc.x, pc.y, pc.z, nc.x, nc.y, nc.z, pts[j].x, pts[j].y, pts[j].z,
                                                                              nrm[j].x, nrm[j].y, nrm[j].z)) ? 1u : 0u;
            support_row[c] = count;
            if (count) key = std::max(key, planes::winner_key(count, c));
        }
        if (support_out) std::memcpy(support_out + (size_t)k * PR_PLANE_MAX_CANDIDATES, support_row.data(), sizeof(uint32_t) * n_cand);
        uint64_t m[10] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        if (key) {
            const uint32_t w = (0xFFFFFFFFu - (uint32_t)key) * pp.cand_stride;
            for (uint32_t j = 0; j < n; ++j) {
                if (labels_out[pts[j].px] != 0 || !planes::supports(pp.tau_mm, pp.cos_min, pts[w].x, pts[w].y, pts[w].z, nrm[w].x, nrm[w].y, nrm[w].z, pts[j].x, pts[j].y,
                                                                    pts[j].z, nrm[j].x, nrm[j].y, nrm[j].z)) continue;
                uint64_t pm[10];
                planes::point_moments(pts[j].x, pts[j].y, pts[j].z, pm);
                for (int e = 0; e < 10; ++e) m[e] += pm[e];
            }
        }
        pr_plane &pl = planes_out[k];
        if (!round_plane(&pp, key, m, &pl, moments_out ? moments_out + 10 * (size_t)k : nullptr)) break;
        for (size_t i = 0; i < n_px; ++i) {
            if (labels_out[i] != 0) continue;
            const uint8_t lab = planes::pixel_label(pp, k + 1, pl.normal[0], pl.normal[1], pl.normal[2], pl.offset_mm, pcd[i * 3], pcd[i * 3 + 1], pcd[i * 3 + 2],
                                                    normal[i * 3], normal[i * 3 + 1], normal[i * 3 + 2]);
            if (!lab) continue;
            labels_out[i] = lab;
            if (lab == (uint8_t)PR_PLANE_BEHIND) ++pl.behind; else ++pl.labelled;
        }
        *n_found = k + 1;
    }
    if (depth_out)
        with_depth(depth_out, depth_is_i32 != 0, [&](auto *out) {
            using T = std::remove_pointer_t<decltype(out)>;
            for (size_t i = 0; i < n_px; ++i) out[i] = labels_out[i] == 0 ? static_cast<const T *>(depth)[i] : (T)0;
        });
    return PR_OK;
}

int pr_scene_planes_dev(const pr_scene_proj *scene, const void *depth_dev, int depth_is_i32, const pr_plane_params *params, uint8_t *labels_dev_out,
                        void *depth_dev_out, pr_plane *planes_host, int64_t *moments_host, uint32_t *support_dev_out, uint32_t *n_found)
{
    const char *fn = "pr_scene_planes_dev";
    PR_TRY(plane_params_ok(fn, params));                            // every check before any device use
    if (!scene || !scene->pcd || !scene->normal || !labels_dev_out || !planes_host || !n_found || (depth_dev_out && !depth_dev)) {
        set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID;
    }
    PR_TRY(frame_ok(fn, scene->width, scene->height));
    PR_ENTER();
    const pr_plane_params pp = *params;
    const uint32_t W = (uint32_t)scene->width, H = (uint32_t)scene->height, n_px = W * H, gh = (H + pp.stride - 1) / pp.stride;
    const float *pcd = reinterpret_cast<const float *>(scene->pcd), *normal = reinterpret_cast<const float *>(scene->normal);
    const PlaneBlock l(pp.n_planes, gh, !support_dev_out);
    PR_TRY(g->plane_tmp.ensure(l.b.bytes()));
    PR_TRY(g->h_plane.ensure(sizeof(prk::PlaneRound) * pp.n_planes));
    void *d = g->plane_tmp.p;
    prk::PlaneRound *rounds = at<prk::PlaneRound>(d, l.rounds);
    const ScanRows rows(d, l.rows, gh);
    prk::PlaneSample *pts = at<prk::PlaneSample>(d, l.pts);
    pr_vec3 *nrm = at<pr_vec3>(d, l.nrm);
    uint32_t *support = support_dev_out ? support_dev_out : at<uint32_t>(d, l.support);

    HIP_TRY(prk::launch_plane_sample_count(pcd, normal, W, H, pp.stride, rows.count, rows.off, g->stream));
    uint32_t n = 0, n_cand = 0;
    PR_TRY(read_back_words(rows.total, &n, 1, g->stream));
    PR_TRY(sample_caps_ok(fn, &pp, n, &n_cand));                    // the last check that refuses: nothing of the caller's is written before
    *n_found = 0;
    note_write(labels_dev_out, n_px);
    if (support_dev_out) note_write(support_dev_out, sizeof(uint32_t) * (size_t)pp.n_planes * PR_PLANE_MAX_CANDIDATES);
    if (depth_dev_out) note_write(depth_dev_out, (size_t)n_px * depth_bytes(depth_is_i32 != 0));
    HIP_TRY(prk::launch_plane_init(pcd, n_px, labels_dev_out, rounds, pp.n_planes, support, pp.n_planes * PR_PLANE_MAX_CANDIDATES, g->stream));
    if (n > 0) HIP_TRY(prk::launch_plane_sample_emit(pcd, normal, W, H, pp.stride, rows.off, pts, nrm, g->stream));
    const uint32_t round_words = (uint32_t)(sizeof(prk::PlaneRound) / sizeof(uint32_t));
    uint32_t found = 0;
    for (uint32_t k = 0; k < pp.n_planes && n > 0; ++k) {
        HIP_TRY(prk::launch_plane_round(pp, pts, nrm, n, n_cand, labels_dev_out, (uint32_t)g->n_cus, support + (size_t)k * PR_PLANE_MAX_CANDIDATES, rounds + k, g->stream));
        HIP_TRY(prk::launch_copy_words32(rounds + k, g->h_plane.dev_as<prk::PlaneRound>() + k, round_words, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        const prk::PlaneRound r = g->h_plane.as<prk::PlaneRound>()[k];
        if (!round_plane(&pp, r.key, r.m, &planes_host[k], moments_host ? moments_host + 10 * (size_t)k : nullptr)) break;
        const float plane[4] = { planes_host[k].normal[0], planes_host[k].normal[1], planes_host[k].normal[2], planes_host[k].offset_mm };
        HIP_TRY(prk::launch_plane_label(pp, k + 1, plane, pcd, normal, n_px, labels_dev_out, rounds + k, g->stream));
        found = k + 1;
    }
    if (depth_dev_out) HIP_TRY(prk::launch_plane_clear_depth(labels_dev_out, depth_dev, depth_dev_out, depth_is_i32 != 0, n_px, g->stream));
    if (found) HIP_TRY(prk::launch_copy_words32(rounds, g->h_plane.dev, found * round_words, g->stream));      // the label passes' counts
    HIP_TRY(hipStreamSynchronize(g->stream));
    for (uint32_t k = 0; k < found; ++k) {
        const prk::PlaneRound &r = g->h_plane.as<prk::PlaneRound>()[k];
        planes_host[k].labelled = r.labelled; planes_host[k].behind = r.behind;
    }
    *n_found = found;
    return PR_OK;
}

}  // extern "C"
