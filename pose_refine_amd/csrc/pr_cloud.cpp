// pr_cloud.cpp -- pr_cloud_* / pr_scene_nn_from_cloud_dev / pr_ppf_cloud_points_dev: the parameters, the host twins of the k-NN walk and the PCA
// normal (cloud.h is their source and the kernels') and the launches of cloud.hip
#include <vector>

#include "pr_runtime.h"
#include "frame_stage.h"
#include "cloud.h"

namespace prr {

// a parameter block as a caller hands it over: pr_cloud_describe's rules.  No HIP call in here.
static int cloud_params_ok(const char *fn, const pr_cloud_params *cp)
{
    if (!cp) { set_error("%s: null pr_cloud_params", fn); return PR_ERR_INVALID; }
    if (cp->k == 0 || cp->k > PR_KNN_MAX_K) { set_error("%s: pr_cloud_params: k must be 1 .. PR_KNN_MAX_K = %d (got %u)", fn, PR_KNN_MAX_K, cp->k); return PR_ERR_INVALID; }
    if (!(cp->max_radius > 0.0f)) { set_error("%s: pr_cloud_params: max_radius must be positive or INFINITY (got %g)", fn, (double)cp->max_radius); return PR_ERR_INVALID; }
    if (!(cp->r2 >= 0.0f)) { set_error("%s: pr_cloud_params: r2 is not max_radius squared (got %g): fill the block with pr_cloud_describe", fn, (double)cp->r2); return PR_ERR_INVALID; }
    if (cp->min_neighbours < 3) { set_error("%s: pr_cloud_params: min_neighbours must be at least 3 (got %u)", fn, cp->min_neighbours); return PR_ERR_INVALID; }
    if (!(cp->line_ratio >= 0.0f && cp->line_ratio < 1.0f)) { set_error("%s: pr_cloud_params: line_ratio must be in [0, 1) (got %g)", fn, (double)cp->line_ratio); return PR_ERR_INVALID; }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(cp->viewpoint[a])) { set_error("%s: pr_cloud_params: viewpoint[%d] is not finite", fn, a); return PR_ERR_INVALID; }
    return PR_OK;
}
static int cloud_size_ok(const char *fn, size_t n_points)
{
    if (n_points == 0) { set_error("%s: no points", fn); return PR_ERR_INVALID; }
    if (n_points >= 0x7fffffffu) { set_error("%s: %zu points are more than the node records' int ranges hold", fn, n_points); return PR_ERR_INVALID; }
    return PR_OK;
}

// ---- the host twins' tree and list ------------------------------------------------------------------------------------------------------
// the caller's pr_kdnode array as cloud::knn_walk's tree: the links re-encoded as build_nn_accel encodes them, a leaf's box taken over its points
struct HostTree {
    const pr_vec3 *pcd;
    const pr_kdnode *nodes;
    cloud::Topo node(int c) const
    {
        const pr_kdnode &nd = nodes[c];
        const int pw = ((nd.parent + 1) & 0x3fffffff) | (int)((uint32_t)(nd.split_dim & 3) << 30);
        if (nd.child1 < 0 || nd.child2 < 0) return cloud::Topo{ nd.left, nd.right, -1, pw };
        int bits;
        std::memcpy(&bits, &nd.split_v, sizeof bits);
        return cloud::Topo{ bits, nd.child1, nd.child2, pw };
    }
    cloud::Box box(int c) const
    {
        const pr_kdnode &nd = nodes[c];
        if (!(nd.child1 < 0 || nd.child2 < 0)) return cloud::Box{ { nd.bbox[0], nd.bbox[2], nd.bbox[4] }, { nd.bbox[1], nd.bbox[3], nd.bbox[5] } };
        cloud::Box b{ { FLT_MAX, FLT_MAX, FLT_MAX }, { -FLT_MAX, -FLT_MAX, -FLT_MAX } };
        for (int k = nd.left; k < nd.right; ++k) {
            const float c3[3] = { pcd[k].x, pcd[k].y, pcd[k].z };
            for (int d = 0; d < 3; ++d) { b.lo[d] = std::fmin(b.lo[d], c3[d]); b.hi[d] = std::fmax(b.hi[d], c3[d]); }
        }
        return b;
    }
    cloud::Point point(int i) const { return cloud::Point{ pcd[i].x, pcd[i].y, pcd[i].z }; }
};
struct HostList {
    float d2[PR_KNN_MAX_K];
    uint32_t idx[PR_KNN_MAX_K];
    float d(uint32_t t) const { return d2[t]; }
    uint32_t j(uint32_t t) const { return idx[t]; }
    void set(uint32_t t, float v, uint32_t i) { d2[t] = v; idx[t] = i; }
};
// the walk follows child AND parent links: both are the caller's, so they are cross-checked before it runs (as nn_records_kernel does on the device)
static int host_tree_ok(const char *fn, const pr_vec3 *pcd, size_t n_points, const pr_kdnode *nodes, size_t n_nodes)
{
    if (!pcd || !nodes) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(cloud_size_ok(fn, n_points));
    if (n_nodes == 0 || n_nodes >= 0x3fffffffu) { set_error("%s: %zu nodes", fn, n_nodes); return PR_ERR_INVALID; }
    bool ok = nodes[0].parent == -1;
    for (size_t i = 0; i < n_nodes && ok; ++i) {
        const pr_kdnode &nd = nodes[i];
        if (nd.child1 < 0 || nd.child2 < 0) ok = nd.left >= 0 && nd.left <= nd.right && (size_t)nd.right <= n_points;
        else ok = (size_t)nd.child1 > i && (size_t)nd.child1 < n_nodes && (size_t)nd.child2 > i && (size_t)nd.child2 < n_nodes && nd.child1 != nd.child2 &&
                  nodes[nd.child1].parent == (int)i && nodes[nd.child2].parent == (int)i;
    }
    if (!ok) { set_error("%s: the nodes do not form a consistent tree (child / parent links disagree or point outside the arrays)", fn); return PR_ERR_INVALID; }
    return PR_OK;
}

static void counts_from_tally(uint32_t n, const uint32_t tally[3], pr_cloud_counts *out)
{
    if (out) *out = pr_cloud_counts{ n, tally[cloud::kWithNormal], tally[cloud::kTooFew], tally[cloud::kDegenerate] };
}

// ---- the device side (the context's lock is held) ---------------------------------------------------------------------------------------
// the scene's traversal arrays come from make_scene, as pr_scene_grid_build_dev gets them; the kernel reads those and never scene->normal
static int cloud_normals_dev(const char *fn, const pr_scene_nn *scene, const pr_cloud_params &cp, pr_vec3 *normal_out, float *variation_out, pr_cloud_counts *counts_out)
{
    PR_TRY(cloud_size_ok(fn, scene->n_points));
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    PR_TRY(make_scene(PR_SCENE_NN, scene, false, sc));
    // announced like every write through the library: a batch in flight that reads the range finishes first, and every cached form derived from
    // it (a packed projective scene over the same array) is dropped; the kd-tree records hold no normals and stay
    note_write(normal_out, (size_t)scene->n_points * sizeof(pr_vec3));
    if (variation_out) note_write(variation_out, (size_t)scene->n_points * sizeof(float));
    PR_TRY(g->cloud_tmp.ensure(4 * sizeof(uint32_t)));
    uint32_t *tally = g->cloud_tmp.as<uint32_t>();
    HIP_TRY(hipMemsetAsync(tally, 0, 4 * sizeof(uint32_t), g->stream));
    HIP_TRY(prk::launch_cloud_knn(sc.nn, scene->n_points, cp, nullptr, nullptr, nullptr, normal_out, variation_out, tally, g->stream));
    uint32_t t[3] = { 0, 0, 0 };
    PR_TRY(read_back_words(tally, t, 3, g->stream));                // (waits for the stream)
    counts_from_tally(scene->n_points, t, counts_out);
    return PR_OK;
}

}  // namespace prr

using namespace prr;

extern "C" {

int pr_cloud_describe(uint32_t k, float max_radius, uint32_t min_neighbours, float line_ratio, const float viewpoint[3], pr_cloud_params *out)
{
    const char *fn = "pr_cloud_describe";
    if (!out || !viewpoint) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    const volatile float r2 = max_radius * max_radius;             // (volatile: rounded to float32 once, whatever the host compiler's excess precision)
    const pr_cloud_params cp = { k, min_neighbours, max_radius, (float)r2, line_ratio, { viewpoint[0], viewpoint[1], viewpoint[2] } };
    PR_TRY(cloud_params_ok(fn, &cp));
    *out = cp;
    return PR_OK;
}

int pr_cloud_knn_dev(const pr_scene_nn *scene, const pr_cloud_params *params, uint32_t *idx_dev, float *d2_dev, uint32_t *count_dev)
{
    const char *fn = "pr_cloud_knn_dev";
    PR_TRY(cloud_params_ok(fn, params));
    if (!scene || !idx_dev) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(cloud_size_ok(fn, scene->n_points));
    PR_ENTER();
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    PR_TRY(make_scene(PR_SCENE_NN, scene, false, sc));
    const size_t n = scene->n_points;
    note_write(idx_dev, n * params->k * sizeof(uint32_t));
    if (d2_dev) note_write(d2_dev, n * params->k * sizeof(float));
    if (count_dev) note_write(count_dev, n * sizeof(uint32_t));
    HIP_TRY(prk::launch_cloud_knn(sc.nn, scene->n_points, *params, idx_dev, d2_dev, count_dev, nullptr, nullptr, nullptr, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

int pr_cloud_normals_dev(const pr_scene_nn *scene, const pr_cloud_params *params, pr_vec3 *normal_dev_out, float *variation_dev_out, pr_cloud_counts *counts_out)
{
    const char *fn = "pr_cloud_normals_dev";
    PR_TRY(cloud_params_ok(fn, params));
    if (!scene || !normal_dev_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_ENTER();
    return cloud_normals_dev(fn, scene, *params, normal_dev_out, variation_dev_out, counts_out);
}

int pr_scene_nn_from_cloud_dev(pr_vec3 *pcd_dev, size_t n_points, int max_leaf, const pr_cloud_params *params, pr_vec3 *normal_dev_out,
                               pr_kdnode *nodes_dev_out, size_t cap_nodes, uint32_t *n_nodes, pr_cloud_counts *counts_out)
{
    const char *fn = "pr_scene_nn_from_cloud_dev";
    PR_TRY(cloud_params_ok(fn, params));
    if (!pcd_dev || !normal_dev_out || !nodes_dev_out || !n_nodes) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(cloud_size_ok(fn, n_points));
    PR_ENTER();
    note_write(pcd_dev, n_points * sizeof(pr_vec3)); note_write(normal_dev_out, n_points * sizeof(pr_vec3)); note_write(nodes_dev_out, cap_nodes * sizeof(pr_kdnode));
    // the builder moves a normal with its point: the array is cleared first so that it moves zeros, not whatever the buffer held
    HIP_TRY(hipMemsetAsync(normal_dev_out, 0, n_points * sizeof(pr_vec3), g->stream));
    PR_TRY(kd_build_dev(pcd_dev, normal_dev_out, (uint32_t)n_points, max_leaf, nodes_dev_out, cap_nodes, n_nodes));
    // the traversal records are derived for the reference's default radius (pcd_scene.h:52): a later ICP call with max_dist_diff <= 0.1 finds them derived
    pr_scene_nn scene;
    std::memset(&scene, 0, sizeof scene);
    scene.max_dist_diff = 0.1f; scene.pcd = pcd_dev; scene.normal = normal_dev_out; scene.nodes = nodes_dev_out;
    scene.n_points = (uint32_t)n_points; scene.n_nodes = *n_nodes;
    return cloud_normals_dev(fn, &scene, *params, normal_dev_out, nullptr, counts_out);
}

int pr_cloud_knn_host(const pr_vec3 *pcd, size_t n_points, const pr_kdnode *nodes, size_t n_nodes, const pr_cloud_params *params, uint32_t *idx_out,
                      float *d2_out, uint32_t *count_out)
{
    const char *fn = "pr_cloud_knn_host";
    PR_TRY(cloud_params_ok(fn, params));
    if (!idx_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(host_tree_ok(fn, pcd, n_points, nodes, n_nodes));
    const HostTree tree{ pcd, nodes };
    const uint32_t k = params->k;
    for (size_t i = 0; i < n_points; ++i) {
        HostList list;
        const uint32_t m = cloud::knn_walk(tree, list, k, params->r2, pcd[i].x, pcd[i].y, pcd[i].z);
        for (uint32_t e = 0; e < k; ++e) {
            idx_out[i * k + e] = e < m ? list.j(e) : (uint32_t)PR_KNN_NONE;
            if (d2_out) d2_out[i * k + e] = e < m ? list.d(e) : 0.0f;
        }
        if (count_out) count_out[i] = m;
    }
    return PR_OK;
}

int pr_cloud_normals_host(const pr_vec3 *pcd, size_t n_points, const pr_kdnode *nodes, size_t n_nodes, const pr_cloud_params *params, pr_vec3 *normal_out,
                          float *variation_out, pr_cloud_counts *counts_out)
{
    const char *fn = "pr_cloud_normals_host";
    PR_TRY(cloud_params_ok(fn, params));
    if (!normal_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(host_tree_ok(fn, pcd, n_points, nodes, n_nodes));
    const HostTree tree{ pcd, nodes };
    uint32_t tally[3] = { 0, 0, 0 };
    for (size_t i = 0; i < n_points; ++i) {
        HostList list;
        const pr_vec3 p = pcd[i];
        const uint32_t m = cloud::knn_walk(tree, list, params->k, params->r2, p.x, p.y, p.z);
        const cloud::Normal r = cloud::normal_from_list(tree, list, m, *params, p.x, p.y, p.z);
        normal_out[i] = pr_vec3{ r.n[0], r.n[1], r.n[2] };
        if (variation_out) variation_out[i] = r.variation;
        ++tally[r.status];
    }
    counts_from_tally((uint32_t)n_points, tally, counts_out);
    return PR_OK;
}

int pr_ppf_cloud_points_dev(const pr_scene_nn *scene, uint32_t stride, pr_vec3 *points_dev_out, pr_vec3 *normals_dev_out, uint32_t *n_out)
{
    const char *fn = "pr_ppf_cloud_points_dev";
    if (!scene || !scene->pcd || !scene->normal || !points_dev_out || !normals_dev_out || !n_out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (stride == 0) { set_error("%s: stride must be at least 1", fn); return PR_ERR_INVALID; }
    PR_TRY(cloud_size_ok(fn, scene->n_points));
    PR_ENTER();
    const uint32_t n_pts = scene->n_points, n_chunks = ((n_pts - 1) / stride + 1 + prk::kCloudChunk - 1) / prk::kCloudChunk;
    PR_TRY(g->ppf_tmp.ensure(sizeof(uint32_t) * ScanRows::words(n_chunks)));
    const ScanRows chunks(g->ppf_tmp.p, 0, n_chunks);
    HIP_TRY(prk::launch_cloud_sample_count(scene->normal, n_pts, stride, chunks.count, chunks.off, g->stream));
    uint32_t n = 0;
    PR_TRY(read_back_words(chunks.total, &n, 1, g->stream));
    *n_out = n;
    if (n > PR_PPF_MAX_SCENE_POINTS) { set_error("%s: %u points at stride %u, at most PR_PPF_MAX_SCENE_POINTS = %d (raise the stride)", fn, n, stride, PR_PPF_MAX_SCENE_POINTS); return PR_ERR_INVALID; }
    if (n == 0) return PR_OK;
    note_write(points_dev_out, sizeof(pr_vec3) * n);
    note_write(normals_dev_out, sizeof(pr_vec3) * n);
    HIP_TRY(prk::launch_cloud_sample_emit(scene->pcd, scene->normal, n_pts, stride, chunks.off, points_dev_out, normals_dev_out, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

}  // extern "C"
