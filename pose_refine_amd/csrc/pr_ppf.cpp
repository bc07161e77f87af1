// pr_ppf.cpp -- pr_ppf_*: the descriptor and its tables, the model sampler and the pose formula on the host, the launches of ppf.hip
#include <unordered_set>

#include "pr_runtime.h"
#include "frame_stage.h"
#include "ppf.h"

namespace prr {

// a descriptor as a caller hands it over: pr_ppf_describe's rules (not the tables' values).  No HIP call in here.
static int ppf_params_ok(const char *fn, const pr_ppf_params *pp)
{
    if (!pp) { set_error("%s: null pr_ppf_params", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(pp->dist_step) || !(pp->dist_step > 0.0f) || !std::isfinite(pp->diameter) || !(pp->diameter > 0.0f)) {
        set_error("%s: pr_ppf_params: diameter and dist_step must be finite and positive (got %g, %g)", fn, (double)pp->diameter, (double)pp->dist_step); return PR_ERR_INVALID;
    }
    if (!(pp->inv_dist_step == 1.0f / pp->dist_step)) { set_error("%s: pr_ppf_params: inv_dist_step is not 1.0f / dist_step (pr_ppf_describe computes it)", fn); return PR_ERR_INVALID; }
    if (pp->n_dist == 0 || pp->n_dist > PR_PPF_MAX_DIST_BINS) { set_error("%s: pr_ppf_params: n_dist must be 1 .. PR_PPF_MAX_DIST_BINS = %d (got %u)", fn, PR_PPF_MAX_DIST_BINS, pp->n_dist); return PR_ERR_INVALID; }
    if (pp->n_angle < 2 || pp->n_angle > PR_PPF_MAX_ANGLE_BINS) { set_error("%s: pr_ppf_params: n_angle must be 2 .. PR_PPF_MAX_ANGLE_BINS = %d (got %u)", fn, PR_PPF_MAX_ANGLE_BINS, pp->n_angle); return PR_ERR_INVALID; }
    if (pp->n_alpha < 2 || pp->n_alpha > PR_PPF_MAX_ALPHA_BINS || (pp->n_alpha & 1u)) { set_error("%s: pr_ppf_params: n_alpha must be even, 2 .. PR_PPF_MAX_ALPHA_BINS = %d (got %u)", fn, PR_PPF_MAX_ALPHA_BINS, pp->n_alpha); return PR_ERR_INVALID; }
    if (pp->n_keys != pp->n_dist * pp->n_angle * pp->n_angle * pp->n_angle || pp->n_keys > PR_PPF_MAX_KEYS) { set_error("%s: pr_ppf_params: n_keys is not n_dist * n_angle^3 <= PR_PPF_MAX_KEYS (got %u)", fn, pp->n_keys); return PR_ERR_INVALID; }
    return PR_OK;
}
static ppf::Tables tables_of(const pr_ppf_params *pp) { ppf::Tables t; std::memcpy(&t, pp, sizeof t); return t; }
// what pr_ppf_vote and pr_ppf_vote_multi ask of a model (fn: the entry point, for the table's models with the model's index behind it) ...
static int vote_model_ok(const char *fn, const pr_ppf_params *pp, uint32_t n_model)
{
    PR_TRY(ppf_params_ok(fn, pp));
    if (n_model == 0 || n_model > PR_PPF_MAX_MODEL_POINTS) { set_error("%s: n_model must be 1 .. PR_PPF_MAX_MODEL_POINTS = %d (got %u)", fn, PR_PPF_MAX_MODEL_POINTS, n_model); return PR_ERR_INVALID; }
    if (n_model * pp->n_alpha > PR_PPF_MAX_CELLS) { set_error("%s: n_model * n_alpha = %u, at most PR_PPF_MAX_CELLS = %d (one workgroup's LDS)", fn, n_model * pp->n_alpha, PR_PPF_MAX_CELLS); return PR_ERR_INVALID; }
    return PR_OK;
}
// ... and of the scene sample, the peaks and the references.  No HIP call in either.
static int vote_refs_ok(const char *fn, uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks)
{
    if (n_scene == 0 || n_scene > PR_PPF_MAX_SCENE_POINTS) { set_error("%s: n_scene must be 1 .. PR_PPF_MAX_SCENE_POINTS = %d (got %u)", fn, PR_PPF_MAX_SCENE_POINTS, n_scene); return PR_ERR_INVALID; }
    if (n_peaks == 0 || n_peaks > PR_PPF_MAX_PEAKS) { set_error("%s: n_peaks must be 1 .. PR_PPF_MAX_PEAKS = %d (got %u)", fn, PR_PPF_MAX_PEAKS, n_peaks); return PR_ERR_INVALID; }
    if (ref_stride == 0) { set_error("%s: ref_stride must not be 0", fn); return PR_ERR_INVALID; }
    if (ref_first >= n_scene || (n_refs > 0 && (uint64_t)ref_first + (uint64_t)(n_refs - 1) * ref_stride >= n_scene)) {
        set_error("%s: references %u + j * %u, j < %u, but there are %u scene points", fn, ref_first, ref_stride, n_refs, n_scene); return PR_ERR_INVALID;
    }
    return PR_OK;
}

// the pose formula's frame, in double from the float32 normal: rows (nh, u, v)
static bool frame_d(const pr_vec3 &n, double B[3][3])
{
    const double nx = n.x, ny = n.y, nz = n.z;
    const double ln = std::sqrt((nx * nx + ny * ny) + nz * nz);
    if (!(ln > 0.0) || !std::isfinite(ln)) return false;
    const double hx = nx / ln, hy = ny / ln, hz = nz / ln;
    const float ax = std::fabs(n.x), ay = std::fabs(n.y), az = std::fabs(n.z);
    double wx, wy, wz;
    if (ax <= ay && ax <= az) { wx = 0.0; wy = -hz; wz = hy; }
    else if (ay <= az)        { wx = hz; wy = 0.0; wz = -hx; }
    else                      { wx = -hy; wy = hx; wz = 0.0; }
    const double lw = std::sqrt((wx * wx + wy * wy) + wz * wz);
    if (!(lw > 0.0) || !std::isfinite(lw)) return false;
    const double ux = wx / lw, uy = wy / lw, uz = wz / lw;
    B[0][0] = hx; B[0][1] = hy; B[0][2] = hz;
    B[1][0] = ux; B[1][1] = uy; B[1][2] = uz;
    B[2][0] = hy * uz - hz * uy; B[2][1] = hz * ux - hx * uz; B[2][2] = hx * uy - hy * ux;
    return true;
}
static bool peak_pose(const pr_ppf_params *pp, const pr_vec3 &pm, const pr_vec3 &nm, const pr_vec3 &ps, const pr_vec3 &ns, uint32_t bin, pr_mat4 *out)
{
    double Bm[3][3], Bs[3][3], M[3][3];
    if (!frame_d(nm, Bm) || !frame_d(ns, Bs)) return false;
    const double c = pp->alpha_cos[bin], s = pp->alpha_sin[bin];
    for (int j = 0; j < 3; ++j) { M[0][j] = Bm[0][j]; M[1][j] = c * Bm[1][j] - s * Bm[2][j]; M[2][j] = s * Bm[1][j] + c * Bm[2][j]; }
    const double p[3] = { pm.x, pm.y, pm.z }, q[3] = { ps.x, ps.y, ps.z };
    std::memset(out, 0, sizeof *out);
    for (int i = 0; i < 3; ++i) {
        double R[3];
        for (int j = 0; j < 3; ++j) { R[j] = (Bs[0][i] * M[0][j] + Bs[1][i] * M[1][j]) + Bs[2][i] * M[2][j]; out->m[i * 4 + j] = (float)R[j]; }
        out->m[i * 4 + 3] = (float)(q[i] - ((R[0] * p[0] + R[1] * p[1]) + R[2] * p[2]));
    }
    out->m[15] = 1.0f;
    return true;
}

// one model's n_pk = n_refs * n_peaks peaks as read back (pk, with the references rf) to the caller, each with its pose (an unused slot: all zero)
static void peaks_out(const pr_ppf_params *pp, const pr_vec3 *model_points, const pr_vec3 *model_normals, uint32_t n_model, const pr_ppf_peak *pk,
                      const prk::PpfRef *rf, size_t n_pk, uint32_t n_peaks, pr_ppf_peak *peaks_host, pr_mat4 *poses_host)
{
    for (size_t i = 0; i < n_pk; ++i) {
        peaks_host[i] = pk[i];
        std::memset(&poses_host[i], 0, sizeof(pr_mat4));
        const prk::PpfRef &r = rf[i / n_peaks];
        if (pk[i].votes && pk[i].model_ref < n_model)
            (void)peak_pose(pp, model_points[pk[i].model_ref], model_normals[pk[i].model_ref], r.p, r.n, pk[i].alpha_bin, &poses_host[i]);
    }
}

}  // namespace prr

using namespace prr;

extern "C" {

int pr_ppf_describe(float diameter_mm, float dist_step_mm, uint32_t n_angle, uint32_t n_alpha, int flip_model_normals, pr_ppf_params *out)
{
    const char *fn = "pr_ppf_describe";
    pr_ppf_params pp;
    std::memset(&pp, 0, sizeof pp);
    pp.diameter = diameter_mm; pp.dist_step = dist_step_mm; pp.inv_dist_step = 1.0f / dist_step_mm;
    pp.n_angle = n_angle; pp.n_alpha = n_alpha; pp.flip_model_normals = flip_model_normals ? 1u : 0u;
    if (!out) { set_error("%s: null out", fn); return PR_ERR_INVALID; }
    if (std::isfinite(diameter_mm) && std::isfinite(dist_step_mm) && diameter_mm > 0.0f && dist_step_mm > 0.0f) {
        const double nd = std::ceil((double)diameter_mm / (double)dist_step_mm);
        pp.n_dist = nd <= (double)PR_PPF_MAX_DIST_BINS ? (uint32_t)nd : PR_PPF_MAX_DIST_BINS + 1u;
    }
    if (pp.n_angle <= PR_PPF_MAX_ANGLE_BINS) pp.n_keys = pp.n_dist * n_angle * n_angle * n_angle;
    PR_TRY(ppf_params_ok(fn, &pp));
    const double pi = 3.14159265358979323846;
    for (uint32_t k = 0; k <= n_angle; ++k) pp.cos_edge[k] = (float)std::cos((double)k * pi / (double)n_angle);
    for (uint32_t k = 0; k <= n_alpha / 2; ++k) pp.alpha_edge[k] = (float)std::cos((double)k * (2.0 * pi) / (double)n_alpha);
    for (uint32_t b = 0; b < n_alpha; ++b) {
        const double a = ((double)b + 0.5) * (2.0 * pi) / (double)n_alpha;
        pp.alpha_cos[b] = std::cos(a); pp.alpha_sin[b] = std::sin(a);
    }
    *out = pp;
    return PR_OK;
}

int pr_ppf_model_sample(const pr_triangle *tris_host, size_t n_tris, float step_mm, int flip_normals, pr_vec3 *points_out, pr_vec3 *normals_out, uint32_t *n_out)
{
    const char *fn = "pr_ppf_model_sample";
    if ((!tris_host && n_tris > 0) || !points_out || !normals_out || !n_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(step_mm) || !(step_mm > 0.0f)) { set_error("%s: step_mm must be finite and positive (got %g)", fn, (double)step_mm); return PR_ERR_INVALID; }
    const double step = step_mm;
    struct Key { int64_t x, y, z; bool operator==(const Key &o) const { return x == o.x && y == o.y && z == o.z; } };
    struct KeyHash { size_t operator()(const Key &k) const { return (size_t)((uint64_t)k.x * 0x9e3779b97f4a7c15ull ^ (uint64_t)k.y * 0xc2b2ae3d27d4eb4full ^ (uint64_t)k.z * 0x165667b19e3779f9ull); } };
    std::unordered_set<Key, KeyHash> seen;
    uint32_t n = 0;
    for (size_t t = 0; t < n_tris; ++t) {
        const pr_triangle &tr = tris_host[t];
        const double a[3] = { tr.v0.x, tr.v0.y, tr.v0.z }, e1[3] = { (double)tr.v1.x - a[0], (double)tr.v1.y - a[1], (double)tr.v1.z - a[2] },
                     e2[3] = { (double)tr.v2.x - a[0], (double)tr.v2.y - a[1], (double)tr.v2.z - a[2] }, e3[3] = { e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2] };
        double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const double ln = std::sqrt((nx * nx + ny * ny) + nz * nz);
        if (!(ln > 0.0) || !std::isfinite(ln)) continue;             // degenerate
        nx /= ln; ny /= ln; nz /= ln;
        if (flip_normals) { nx = -nx; ny = -ny; nz = -nz; }
        const double l1 = std::sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]), l2 = std::sqrt((e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]),
                     l3 = std::sqrt((e3[0] * e3[0] + e3[1] * e3[1]) + e3[2] * e3[2]);
        const double nsub = std::ceil(std::max(l1, std::max(l2, l3)) / step);
        if (!(nsub <= 1e6)) { set_error("%s: triangle %zu needs more than 10^6 subdivisions at step %g", fn, t, step); return PR_ERR_INVALID; }
        const int64_t N = std::max<int64_t>(1, (int64_t)nsub);
        for (int64_t i = 0; i <= N; ++i)
            for (int64_t j = 0; j <= N - i; ++j) {
                const double fi = (double)i / (double)N, fj = (double)j / (double)N;
                const pr_vec3 p = { (float)((a[0] + fi * e1[0]) + fj * e2[0]), (float)((a[1] + fi * e1[1]) + fj * e2[1]), (float)((a[2] + fi * e1[2]) + fj * e2[2]) };
                const Key k = { (int64_t)std::floor((double)p.x / step), (int64_t)std::floor((double)p.y / step), (int64_t)std::floor((double)p.z / step) };
                if (!seen.insert(k).second) continue;
                if (n == PR_PPF_MAX_MODEL_POINTS) {                   // (the walk ends here: a fine step on a large mesh would go on for a long time)
                    *n_out = n + 1;
                    set_error("%s: more than PR_PPF_MAX_MODEL_POINTS = %d points at step %g (coarsen the step)", fn, PR_PPF_MAX_MODEL_POINTS, step); return PR_ERR_INVALID;
                }
                points_out[n] = p; normals_out[n] = pr_vec3{ (float)nx, (float)ny, (float)nz };
                ++n;
            }
    }
    *n_out = n;
    return PR_OK;
}

int pr_ppf_peak_pose(const pr_ppf_params *params, const pr_vec3 *model_point, const pr_vec3 *model_normal, const pr_vec3 *scene_point,
                     const pr_vec3 *scene_normal, uint32_t alpha_bin, pr_mat4 *pose_out)
{
    const char *fn = "pr_ppf_peak_pose";
    PR_TRY(ppf_params_ok(fn, params));
    if (!model_point || !model_normal || !scene_point || !scene_normal || !pose_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (alpha_bin >= params->n_alpha) { set_error("%s: alpha_bin %u, but n_alpha = %u", fn, alpha_bin, params->n_alpha); return PR_ERR_INVALID; }
    pr_mat4 m;
    if (!peak_pose(params, *model_point, *model_normal, *scene_point, *scene_normal, alpha_bin, &m)) { set_error("%s: a normal without a frame", fn); return PR_ERR_INVALID; }
    *pose_out = m;
    return PR_OK;
}

int pr_ppf_model_build_dev(const pr_ppf_params *params, const pr_vec3 *points_dev, const pr_vec3 *normals_dev, uint32_t n_model,
                           uint32_t *offsets_dev_out, pr_ppf_entry *entries_dev_out, uint32_t *n_entries_out)
{
    const char *fn = "pr_ppf_model_build_dev";
    PR_TRY(ppf_params_ok(fn, params));                              // before any device use
    if (n_model == 0 || n_model > PR_PPF_MAX_MODEL_POINTS) { set_error("%s: n_model must be 1 .. PR_PPF_MAX_MODEL_POINTS = %d (got %u)", fn, PR_PPF_MAX_MODEL_POINTS, n_model); return PR_ERR_INVALID; }
    if (!points_dev || !normals_dev || !offsets_dev_out || !n_entries_out || (!entries_dev_out && n_model > 1)) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_ENTER();
    const ppf::Tables tb = tables_of(params);
    PR_TRY(g->ppf_tmp.ensure(sizeof(uint32_t) * tb.n_keys));
    note_write(offsets_dev_out, sizeof(uint32_t) * ((size_t)tb.n_keys + 1));
    note_write(entries_dev_out, sizeof(pr_ppf_entry) * (size_t)n_model * (n_model - 1));
    HIP_TRY(prk::launch_ppf_model_build(tb, points_dev, normals_dev, n_model, g->ppf_tmp.as<uint32_t>(), offsets_dev_out, entries_dev_out, g->stream));
    return read_back_words(offsets_dev_out + tb.n_keys, n_entries_out, 1, g->stream);
}

int pr_ppf_scene_points_dev(const pr_scene_proj *scene, uint32_t stride, pr_vec3 *points_dev_out, pr_vec3 *normals_dev_out, uint32_t *n_out)
{
    const char *fn = "pr_ppf_scene_points_dev";
    if (!scene || !scene->pcd || !scene->normal || !points_dev_out || !normals_dev_out || !n_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (stride == 0 || stride > PR_PPF_MAX_STRIDE) { set_error("%s: stride must be 1 .. PR_PPF_MAX_STRIDE = %d (got %u)", fn, PR_PPF_MAX_STRIDE, stride); return PR_ERR_INVALID; }
    PR_TRY(frame_ok(fn, scene->width, scene->height));
    PR_ENTER();
    const uint32_t W = (uint32_t)scene->width, H = (uint32_t)scene->height, gh = (H + stride - 1) / stride;
    PR_TRY(g->ppf_tmp.ensure(sizeof(uint32_t) * ScanRows::words(gh)));
    const ScanRows rows(g->ppf_tmp.p, 0, gh);
    const float *pcd = reinterpret_cast<const float *>(scene->pcd), *normal = reinterpret_cast<const float *>(scene->normal);
    HIP_TRY(prk::launch_ppf_scene_count(pcd, normal, W, H, stride, rows.count, rows.off, g->stream));
    uint32_t n = 0;
    PR_TRY(read_back_words(rows.total, &n, 1, g->stream));
    *n_out = n;
    if (n > PR_PPF_MAX_SCENE_POINTS) { set_error("%s: %u points at stride %u, at most PR_PPF_MAX_SCENE_POINTS = %d (raise the stride)", fn, n, stride, PR_PPF_MAX_SCENE_POINTS); return PR_ERR_INVALID; }
    if (n == 0) return PR_OK;
    note_write(points_dev_out, sizeof(pr_vec3) * n);
    note_write(normals_dev_out, sizeof(pr_vec3) * n);
    HIP_TRY(prk::launch_ppf_scene_emit(pcd, normal, W, H, stride, rows.off, points_dev_out, normals_dev_out, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

int pr_ppf_vote(const pr_ppf_params *params, const uint32_t *offsets_dev, const pr_ppf_entry *entries_dev, const pr_vec3 *model_points_host,
                const pr_vec3 *model_normals_host, uint32_t n_model, const pr_vec3 *scene_points_dev, const pr_vec3 *scene_normals_dev,
                uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks, pr_ppf_peak *peaks_host,
                pr_mat4 *poses_host, uint32_t *acc_dev_out)
{
    const char *fn = "pr_ppf_vote";
    PR_TRY(vote_model_ok(fn, params, n_model));                     // every check before any device use
    PR_TRY(vote_refs_ok(fn, n_scene, ref_first, ref_stride, n_refs, n_peaks));
    if (n_refs == 0) return PR_OK;
    if (!offsets_dev || !entries_dev || !model_points_host || !model_normals_host || !scene_points_dev || !scene_normals_dev || !peaks_host || !poses_host) {
        set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID;
    }
    PR_ENTER();
    const ppf::Tables tb = tables_of(params);
    const VoteBlock l(0, n_refs, n_peaks);            // the device block and its pinned twin
    PR_TRY(g->ppf_out.ensure(l.b.bytes()));
    PR_TRY(g->h_ppf.ensure(l.b.bytes()));
    void *d = g->ppf_out.p, *h = g->h_ppf.p;
    if (acc_dev_out) note_write(acc_dev_out, sizeof(uint32_t) * (size_t)n_refs * n_model * tb.n_alpha);
    HIP_TRY(prk::launch_ppf_vote(tb, offsets_dev, entries_dev, n_model, scene_points_dev, scene_normals_dev, n_scene, ref_first, ref_stride, n_refs, n_peaks,
                                 at<pr_ppf_peak>(d, l.peaks), at<prk::PpfRef>(d, l.refs), acc_dev_out, opt.ppf_walk != 0, g->stream));
    HIP_TRY(prk::launch_copy_words32(at<pr_ppf_peak>(d, l.peaks), at<pr_ppf_peak>(g->h_ppf.dev, l.peaks), l.back_words(), g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    peaks_out(params, model_points_host, model_normals_host, n_model, at<pr_ppf_peak>(h, l.peaks), at<prk::PpfRef>(h, l.refs), (size_t)n_refs * n_peaks, n_peaks, peaks_host,
              poses_host);
    return PR_OK;
}

int pr_ppf_vote_multi(const pr_ppf_model *models, uint32_t n_models, const pr_vec3 *scene_points_dev, const pr_vec3 *scene_normals_dev, uint32_t n_scene,
                      uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks, pr_ppf_peak *peaks_host, pr_mat4 *poses_host,
                      uint32_t *acc_dev_out)
{
    const char *fn = "pr_ppf_vote_multi";
    if (n_models > PR_PPF_MAX_MODELS) { set_error("%s: %u models, at most PR_PPF_MAX_MODELS = %d", fn, n_models, PR_PPF_MAX_MODELS); return PR_ERR_INVALID; }      // every check before any device use
    if (n_models && !models) { set_error("%s: bad arguments (a null model table)", fn); return PR_ERR_INVALID; }
    uint32_t max_cells = 0;
    for (uint32_t k = 0; k < n_models; ++k) {
        char who[64];
        std::snprintf(who, sizeof who, "%s: model %u", fn, k);
        PR_TRY(vote_model_ok(who, models[k].params, models[k].n_model));
        if (models[k].reserved != 0) { set_error("%s: reserved must be 0", who); return PR_ERR_INVALID; }
        max_cells = std::max(max_cells, models[k].n_model * models[k].params->n_alpha);
    }
    PR_TRY(vote_refs_ok(fn, n_scene, ref_first, ref_stride, n_refs, n_peaks));
    if (n_models == 0 || n_refs == 0) return PR_OK;
    for (uint32_t k = 0; k < n_models; ++k)
        if (!models[k].offsets_dev || (!models[k].entries_dev && models[k].n_model > 1) || !models[k].points_host || !models[k].normals_host) {
            set_error("%s: model %u: bad arguments (a null pointer)", fn, k); return PR_ERR_INVALID;
        }
    if (!scene_points_dev || !scene_normals_dev || !peaks_host || !poses_host) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_ENTER();
    const VoteBlock l(n_models, n_refs, n_peaks);     // the device block and its pinned twin
    const size_t n_pk = (size_t)n_refs * n_peaks;
    PR_TRY(g->ppf_out.ensure(l.b.bytes()));
    PR_TRY(g->h_ppf.ensure(l.b.bytes()));
    // The rows of the launch are the models by n_model, largest first: a model's pair table, and with it a workgroup's walk, grows with n_model^2, and
    // a launch that ends with its longest workgroups has a long tail (profiles/ppf_multi/README.md: the same table takes 1.48 ms in the caller's
    // order, 1.19 ms largest first, 1.54 ms largest last).  A record carries its model's place in the outputs, so the row order is free.
    uint32_t row[PR_PPF_MAX_MODELS];
    uint64_t acc_base[PR_PPF_MAX_MODELS], acc_words = 0;
    for (uint32_t k = 0; k < n_models; ++k) {
        row[k] = k; acc_base[k] = acc_words;
        acc_words += (uint64_t)n_refs * models[k].n_model * models[k].params->n_alpha;
    }
    std::stable_sort(row, row + n_models, [&](uint32_t a, uint32_t b) { return models[a].n_model > models[b].n_model; });
    void *d = g->ppf_out.p, *h = g->h_ppf.p, *hm = g->h_ppf.dev;
    prk::PpfModelRec *rec = at<prk::PpfModelRec>(h, l.models);
    for (uint32_t r = 0; r < n_models; ++r) {
        const pr_ppf_model &m = models[row[r]];
        rec[r] = prk::PpfModelRec{ tables_of(m.params), m.offsets_dev, m.entries_dev, m.n_model, (uint32_t)(row[r] * n_pk), acc_base[row[r]], 0 };
    }
    if (acc_dev_out) note_write(acc_dev_out, sizeof(uint32_t) * acc_words);
    HIP_TRY(prk::launch_stage_words(at<prk::PpfModelRec>(hm, l.models), at<prk::PpfModelRec>(d, l.models), l.peaks - l.models, g->stream));
    HIP_TRY(prk::launch_ppf_vote_multi(at<prk::PpfModelRec>(d, l.models), n_models, max_cells, scene_points_dev, scene_normals_dev, n_scene, ref_first, ref_stride, n_refs,
                                       n_peaks, at<pr_ppf_peak>(d, l.peaks), at<prk::PpfRef>(d, l.refs), acc_dev_out, opt.ppf_walk != 0, g->stream));
    HIP_TRY(prk::launch_copy_words32(at<pr_ppf_peak>(d, l.peaks), at<pr_ppf_peak>(hm, l.peaks), l.back_words(), g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    const pr_ppf_peak *pk = at<pr_ppf_peak>(h, l.peaks);
    const prk::PpfRef *rf = at<prk::PpfRef>(h, l.refs);
    for (uint32_t k = 0; k < n_models; ++k)
        peaks_out(models[k].params, models[k].points_host, models[k].normals_host, models[k].n_model, pk + k * n_pk, rf, n_pk, n_peaks, peaks_host + k * n_pk,
                  poses_host + k * n_pk);
    return PR_OK;
}

}  // extern "C"
