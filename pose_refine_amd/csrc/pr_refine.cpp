// pr_refine.cpp -- render, depth -> cloud, and the fused batch path render -> cloud -> ICP: synchronous form, two asynchronous slots, helper threads
#include "pr_runtime.h"
#include "pose_box.h"

namespace prr {

// the hypotheses' poses into g->poses: through the context's pinned staging array, pulled by a kernel (as the asynchronous path stages its inputs) --
// a copy command from the caller's pageable array goes through the runtime's bounce buffers and its copy-engine path (see drive_host's
// result block: that path is where the host-solve pipeline's one-off multi-millisecond stalls came from)
int stage_poses(const pr_mat4 *poses_host, size_t n)
{
    PR_TRY(g->poses.ensure(sizeof(pr_mat4) * n));
    PR_TRY(g->h_poses.ensure(sizeof(pr_mat4) * n));
    std::memcpy(g->h_poses.p, poses_host, sizeof(pr_mat4) * n);
    HIP_TRY(prk::launch_stage_words(g->h_poses.dev, g->poses.p, sizeof(pr_mat4) * n, g->stream));
    return PR_OK;
}

// hypotheses per chunk of a synchronous batch: bound the depth workspace to ~4 GiB per chunk (288 GB of HBM would allow far more; this keeps
// first-touch cost and the 2^32 element index space comfortable)
uint32_t depth_chunk(size_t img, uint32_t P)
{
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(P, ((size_t)4 << 30) / (img * sizeof(int32_t))));
}

// {width, height} of one rendered image: the ROI when one is given, the full frame otherwise
std::pair<size_t, size_t> image_extent(pr_roi roi, size_t W, size_t H)
{
    if (roi.width > 0 && roi.height > 0) return { (size_t)roi.width, (size_t)roi.height };
    return { W, H };
}

template <typename T>
int depth2cloud_impl(const T *depth_dev, uint32_t W, uint32_t H, const float K[9], uint32_t stride, uint32_t tl_x, uint32_t tl_y,
                     pr_vec3 **cloud_out, uint32_t *n_out)
{
    if (!depth_dev || !K || !cloud_out || !n_out || W == 0 || H == 0 || stride == 0) { set_error("pr_depth2cloud: bad arguments"); return PR_ERR_INVALID; }
    const uint32_t gh = H / stride;
    PR_TRY(g->row_count.ensure(sizeof(uint32_t) * std::max(1u, gh)));
    PR_TRY(g->row_off.ensure(sizeof(uint32_t) * std::max(1u, gh)));
    PR_TRY(g->counts.ensure(sizeof(uint32_t)));
    HIP_TRY(prk::launch_depth2cloud<T>(depth_dev, 1, 0, W, H, stride, tl_x, tl_y, K[0], K[4], K[2], K[5], false, g->row_count.as<uint32_t>(),
                                       g->row_off.as<uint32_t>(), g->counts.as<uint32_t>(), nullptr, 0, false, g->stream));
    uint32_t n = 0;
    PR_TRY(read_back_words(g->counts.p, &n, 1, g->stream));
    pr_vec3 *cloud = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&cloud), sizeof(pr_vec3) * std::max(1u, n)));
    if (n > 0) {
        hipError_t e = prk::launch_depth2cloud<T>(depth_dev, 1, 0, W, H, stride, tl_x, tl_y, K[0], K[4], K[2], K[5], false, g->row_count.as<uint32_t>(),
                                                  g->row_off.as<uint32_t>(), g->counts.as<uint32_t>(), cloud, 0, true, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) { hipFree(cloud); set_error("depth2cloud emit failed: %s", hipGetErrorString(e)); return PR_ERR_HIP; }
    }
    *cloud_out = cloud; *n_out = n;
    return PR_OK;
}

// ---- mixed batches (pr_*_multi): MeshPlan, MeshArg and Batch are pr_runtime.h's; here, what puts a plan on the device --------------------------
// the device (g->multi) and pinned (g->h_multi) layout of a mixed batch's tables: [meshes: 16 B per group][box index: 4 B per hypothesis of
// a chunk][raster groups: one per group at most].  Staged through pinned memory by kernels, like the poses (stage_poses): no copy commands.
struct MultiLayout { size_t box, groups, bytes; };
MultiLayout multi_layout(size_t n_groups, size_t chunk)
{
    MultiLayout l;
    l.box = n_groups * sizeof(pr_mesh_ref);
    l.groups = l.box + ((chunk * sizeof(uint32_t) + 15) & ~(size_t)15);
    l.bytes = l.groups + n_groups * sizeof(prk::RasterGroup);
    return l;
}
// the model box(es) into g->aabb: 6 floats, or 6 per group of a mixed batch
int model_boxes(const MeshSource &src, uint32_t chunk)
{
    if (!src.plan) {
        PR_TRY(g->aabb.ensure(6 * sizeof(float)));
        PR_TRY(g->aabb_keys.ensure(6 * sizeof(uint32_t)));
        HIP_TRY(prk::launch_model_aabb(src.tris, (uint32_t)src.n_tris, g->aabb_keys.as<uint32_t>(), g->aabb.as<float>(), nullptr, nullptr, g->stream));
        return PR_OK;
    }
    const MeshPlan &pl = *src.plan;
    const uint32_t G = (uint32_t)pl.mesh.size();
    const MultiLayout l = multi_layout(G, chunk);
    PR_TRY(g->aabb.ensure(6 * sizeof(float) * G));
    PR_TRY(g->aabb_keys.ensure(6 * sizeof(uint32_t) * G));
    PR_TRY(g->multi.ensure(l.bytes));
    PR_TRY(g->h_multi.ensure(l.bytes));
    std::memcpy(g->h_multi.p, pl.mesh.data(), sizeof(pr_mesh_ref) * G);
    HIP_TRY(prk::launch_stage_words(g->h_multi.dev, g->multi.p, sizeof(pr_mesh_ref) * G, g->stream));
    HIP_TRY(prk::launch_model_aabb_multi(g->multi.as<pr_mesh_ref>(), pl.mesh.data(), G, g->aabb_keys.as<uint32_t>(), g->aabb.as<float>(), g->stream));
    return PR_OK;
}
// the raster groups of positions [p0, p0 + np) of a mixed batch into `out` (positions relative to p0); returns how many
uint32_t chunk_groups(const MeshPlan &pl, uint32_t p0, uint32_t np, prk::RasterGroup *out)
{
    uint32_t n = 0;
    for (size_t k = 0; k + 1 < pl.start.size(); ++k) {
        const uint32_t a = std::max(pl.start[k], p0), b = std::min(pl.start[k + 1], p0 + np);
        if (a >= b) continue;
        prk::RasterGroup gr{};
        gr.tris = pl.mesh[k].tris_dev; gr.n_tris = (uint32_t)pl.mesh[k].n_tris; gr.first = a - p0; gr.count = b - a;
        out[n++] = gr;
    }
    return n;
}
// Positions [p0, p0 + np) of a mixed batch as launch_raster and launch_render_boxes take them, through the tables multi_layout lays out for chunks of
// `chunk` (g->multi, g->h_multi: sized by the caller): `index`, one word per position, is staged into the index slot (mesh.box_index: the box every
// hypothesis takes, or whatever else the caller keeps per position) and the groups are left in the pinned block for launch_raster to complete and stage.
int stage_groups(const MeshPlan &pl, uint32_t p0, uint32_t np, uint32_t chunk, const uint32_t *index, prk::RasterMesh &mesh)
{
    const MultiLayout l = multi_layout(pl.mesh.size(), chunk);
    unsigned char *h = g->h_multi.as<unsigned char>(), *hm = g->h_multi.dev_as<unsigned char>(), *d = g->multi.as<unsigned char>();
    std::memcpy(h + l.box, index, sizeof(uint32_t) * np);
    HIP_TRY(prk::launch_stage_words(hm + l.box, d + l.box, sizeof(uint32_t) * np, g->stream));
    mesh = prk::RasterMesh{};
    mesh.groups_host = reinterpret_cast<prk::RasterGroup *>(h + l.groups); mesh.groups_mapped = hm + l.groups;
    mesh.groups_dev = reinterpret_cast<prk::RasterGroup *>(d + l.groups);
    mesh.n_groups = chunk_groups(pl, p0, np, mesh.groups_host);
    mesh.box_index = reinterpret_cast<const uint32_t *>(d + l.box);
    return PR_OK;
}
// The workspaces of a chunk of np renders of img = W x H pixels: the depth boxes (packed: kBoxPack), the pixel boxes with the offsets of the packed boxes
// behind them (box_pack_offsets_kernel) -- returned in box_off -- and (rows) row counts, row offsets and cloud sizes.
int chunk_workspaces(size_t img, uint32_t H, uint32_t np, uint32_t *&box_off, bool rows = true)
{
    PR_TRY(g->depth.ensure(sizeof(int32_t) * (img + prk::kBoxPack) * np));
    if (rows) {
        PR_TRY(g->row_count.ensure(sizeof(uint32_t) * (size_t)H * np));
        PR_TRY(g->row_off.ensure(sizeof(uint32_t) * (size_t)H * np));
        PR_TRY(g->counts.ensure(sizeof(uint32_t) * np));
    }
    PR_TRY(g->bbox.ensure(sizeof(int4) * np + sizeof(uint32_t) * np));
    box_off = reinterpret_cast<uint32_t *>(g->bbox.as<int4>() + np);
    return PR_OK;
}
// chunk [p0, p0 + np) of a batch rendered into per-pose pixel boxes (raster + row counts + row scan), poses staged first.  box_off: the boxes
// packed (kBoxPack) or null.  bands: the LDS-band raster (option raster_mode 1) -- single mesh only; a mixed batch always uses the box raster.
// far: a second plane at the same box_off as g->depth that takes the farthest fragment of every pixel (span render) -- then no row outputs:
// nothing makes clouds of these renders.
int render_chunk(const MeshSource &src, const pr_mat4 *poses_host, uint32_t p0, uint32_t np, uint32_t chunk, uint32_t W, uint32_t H,
                 const pr_mat4 *proj, pr_roi roi, uint32_t *box_off, bool bands, int32_t *far = nullptr)
{
    PR_TRY(stage_poses(poses_host + p0, np));
    if (!src.plan && bands) {
        HIP_TRY(prk::launch_render_bands(src.tris, (uint32_t)src.n_tris, g->poses.as<pr_mat4>(), np, g->aabb.as<float>(), g->bbox.as<int4>(),
                                         g->depth.as<int32_t>(), g->row_count.as<uint32_t>(), g->row_off.as<uint32_t>(),
                                         g->counts.as<uint32_t>(), W, H, *proj, roi, (uint32_t)g->n_cus, g->stream));
        return PR_OK;
    }
    prk::RasterMesh mesh{};
    if (src.plan) PR_TRY(stage_groups(*src.plan, p0, np, chunk, src.plan->box.data() + p0, mesh));
    else { mesh.tris = src.tris; mesh.n_tris = (uint32_t)src.n_tris; }
    mesh.aabb = g->aabb.as<float>();
    prk::RasterTarget t{};
    t.depth = g->depth.as<int32_t>(); t.far = far; t.box_off = box_off; t.roi = roi; t.width = W; t.height = H; t.proj = proj;
    const prk::BoxRows rows = far ? prk::BoxRows{} : prk::BoxRows{ g->row_count.as<uint32_t>(), g->row_off.as<uint32_t>(), g->counts.as<uint32_t>(), nullptr, nullptr, nullptr };
    HIP_TRY(prk::launch_render_boxes(mesh, g->poses.as<pr_mat4>(), np, g->bbox.as<int4>(), t, rows, g->stream));
    return PR_OK;
}

// ---- coarse-to-fine refinement (pr_refine_pyramid): the levels of one rendered chunk -------------------------------------------------------
// What a pyramid call adds to refine_core: the level table and where the per-level outputs go ([n_levels][P], either may be null).
struct PyramidPlan { const pr_pyramid_level *levels; uint32_t n_levels; uint32_t P; pr_result *level_results; uint32_t *level_sizes; };
// the level table's own conditions, checked before any device is touched (a box without a GPU reports a bad table as such)
int pyramid_levels_ok(const char *fn, const pr_pyramid_level *levels, uint32_t n_levels, uint32_t P, const pr_result *results_host)
{
    if (n_levels == 0 || n_levels > PR_PYRAMID_MAX_LEVELS) { set_error("%s: n_levels must be 1..%d (got %u)", fn, PR_PYRAMID_MAX_LEVELS, n_levels); return PR_ERR_INVALID; }
    if (!levels) { if (P == 0) return PR_OK; set_error("%s: bad arguments (levels is null)", fn); return PR_ERR_INVALID; }
    for (uint32_t l = 0; l < n_levels; ++l) {
        if (levels[l].stride == 0 || levels[l].stride > PR_PYRAMID_MAX_STRIDE) { set_error("%s: level %u has stride %u, must be 1..%d", fn, l, levels[l].stride, PR_PYRAMID_MAX_STRIDE); return PR_ERR_INVALID; }
        if (levels[l].crit.max_iteration < 0) { set_error("%s: level %u: max_iteration must be >= 0", fn, l); return PR_ERR_INVALID; }
    }
    if (P && !results_host) { set_error("%s: results_host is null", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
// Hypotheses [p0, p0 + np) are rendered (render_chunk: depth boxes, pixel boxes).  One pass counts every level's samples and the sizes of all levels come
// back in the chunk's one read-back; then, level by level: the carry records (accumulated transform, cloud start) are staged, the level's clouds emitted
// through them, icp_drive run on them as on any batch of clouds, and the accumulated transform advanced on the host (T_l * T_acc, pr_mat4_mul) -- both
// solve modes leave a level's records on the host, and the next level's emit needs them staged either way.
int pyramid_chunk(const PyramidPlan &py, uint32_t p0, uint32_t np, uint32_t W, uint32_t H, const float K[9], const uint32_t *box_off, const SceneSel &sc,
                  pr_result *results_host, const pr_robust *robust)      // robust: the job's table, one descriptor per level
{
    const uint32_t L = py.n_levels;
    const size_t plane = (size_t)L * np * H;                      // words of row counts; the row offsets follow
    PR_TRY(g->lvl_rows.ensure(sizeof(uint32_t) * 2 * plane));
    PR_TRY(g->lvl_counts.ensure(sizeof(uint32_t) * L * np));
    PR_TRY(g->h_counts.ensure(sizeof(uint32_t) * L * np));
    PR_TRY(g->lvl_carry.ensure(sizeof(prk::PyramidCarry) * np));
    PR_TRY(g->h_lvl_carry.ensure(sizeof(prk::PyramidCarry) * np));
    uint32_t *row_count = g->lvl_rows.as<uint32_t>(), *row_off = row_count + plane;
    prk::PyramidStrides lv{};
    lv.n = L;
    for (uint32_t l = 0; l < PR_PYRAMID_MAX_LEVELS; ++l) lv.s[l] = l < L ? py.levels[l].stride : 1u;
    uint32_t *h_counts = g->h_counts.as<uint32_t>();
    {
        SpanGuard sp(kSpanCloud);
        HIP_TRY(prk::launch_pyramid_counts(g->depth.as<int32_t>(), g->bbox.as<int4>(), box_off, np, W, H, lv, row_count, row_off, g->lvl_counts.as<uint32_t>(), g->stream));
        HIP_TRY(prk::launch_copy_words32(g->lvl_counts.p, g->h_counts.dev, L * np, g->stream));   // all levels' sizes through a kernel's stores into the pinned array (see refine_core)
    }
    HIP_TRY(hipStreamSynchronize(g->stream));
    trace_mark("pyramid_chunk: level sizes on host");
    // every level's clouds packed one behind the other like the stride-1 clouds of refine_core; the workspace holds the largest level
    size_t most = 4;
    for (uint32_t l = 0; l < L; ++l) {
        size_t total = 0;
        for (uint32_t i = 0; i < np; ++i) total += prk::cloud_slot(h_counts[(size_t)l * np + i]);
        if (total > 0xffffffffull) { set_error("pr_refine_pyramid: more than 2^32 cloud points in one chunk"); return PR_ERR_INVALID; }
        most = std::max(most, total);
    }
    PR_TRY(g->cloud.ensure(sizeof(pr_vec3) * most));
    prk::PyramidCarry *h_carry = g->h_lvl_carry.as<prk::PyramidCarry>();
    std::vector<pr_result> acc(np), rec(np);
    std::vector<uint32_t> start(np), count(np);
    for (uint32_t i = 0; i < np; ++i) { identity16(acc[i].T); acc[i].fitness = 0.0f; acc[i].inlier_rmse = 0.0f; }
    for (uint32_t l = 0; l < L; ++l) {
        size_t total = 0;
        for (uint32_t i = 0; i < np; ++i) {
            start[i] = (uint32_t)total; count[i] = h_counts[(size_t)l * np + i];
            total += prk::cloud_slot(count[i]);
            std::memset(&h_carry[i], 0, sizeof(prk::PyramidCarry));
            std::memcpy(h_carry[i].T, acc[i].T, sizeof(float) * 12);
            h_carry[i].start = start[i];
        }
        if (total > 0) {
            SpanGuard sp(kSpanCloud);
            HIP_TRY(prk::launch_stage_words(g->h_lvl_carry.dev, g->lvl_carry.p, sizeof(prk::PyramidCarry) * np, g->stream));
            HIP_TRY(prk::launch_pyramid_emit(g->depth.as<int32_t>(), np, W, H, g->bbox.as<int4>(), box_off, K[0], K[4], K[2], K[5], py.levels[l].stride,
                                             row_count + (size_t)l * np * H, row_off + (size_t)l * np * H, g->lvl_carry.as<prk::PyramidCarry>(), l > 0,
                                             g->cloud.as<pr_vec3>(), g->stream));
        }
        trace_mark("pyramid_chunk: level emitted, icp_drive next");
        PR_TRY(icp_drive(g->cloud.as<pr_vec3>(), start.data(), count.data(), np, sc, py.levels[l].crit, rec.data(), nullptr, robust[l]));     // (returns with the stream drained: the pinned carry records are free again)
        for (uint32_t i = 0; i < np; ++i) {
            prh::mat4_mul(rec[i].T, acc[i].T, acc[i].T);
            acc[i].fitness = rec[i].fitness; acc[i].inlier_rmse = rec[i].inlier_rmse;
        }
        if (py.level_results) std::memcpy(py.level_results + (size_t)l * py.P + p0, rec.data(), sizeof(pr_result) * np);
        if (py.level_sizes) std::memcpy(py.level_sizes + (size_t)l * py.P + p0, count.data(), sizeof(uint32_t) * np);
    }
    std::memcpy(results_host, acc.data(), sizeof(pr_result) * np);
    return PR_OK;
}

// One synchronous batch: chunk by chunk the hypotheses rendered into their pixel boxes, the clouds emitted (with `pyramid`: every level's, by
// pyramid_chunk) and icp_drive run on them.  The records go to results_host and to job.results_dev, the cloud sizes to sizes_host; each may be null.
// (info: pr_pose_information -- the information pass on the chunk's clouds in place of icp_drive; centres, radii and records in the batch's order)
struct InfoPlan { pr_robust robust; const float *centers, *radii; pr_pose_info *info; pr_pose_eig *eig; };
int refine_core(const RefineJob &job, const pr_mat4 *poses_host, uint32_t P, pr_result *results_host, uint32_t *sizes_host, const PyramidPlan *pyramid = nullptr,
                const InfoPlan *info = nullptr)
{
    if (P == 0) return PR_OK;
    const MeshSource &src = job.mesh;
    const uint32_t W = job.W, H = job.H;
    const float *K = job.K;
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);           // also zeroes padding: sc is part of the graph-cache key
    const Camera cam{ W, H, K[0], K[4], K[2], K[5] };
    trace_mark("refine_impl: enter");
    PR_TRY(make_scene(job.scene_kind, job.scene(), /*want_packed=*/true, sc, nullptr, nullptr, &cam));
    trace_mark("refine_impl: scene ready");
    const size_t img = (size_t)W * H;
    uint32_t chunk = depth_chunk(img, P);
    std::vector<uint32_t> start(chunk), count(chunk);
    // model box: recomputed from the triangle buffer on every call (one pass over the mesh; nothing is cached by address here)
    PR_TRY(model_boxes(src, chunk));
    for (uint32_t p0 = 0; p0 < P; p0 += chunk) {
        const uint32_t np = std::min(chunk, P - p0);
        uint32_t *box_off = nullptr;
        PR_TRY(chunk_workspaces(img, H, np, box_off));
        PR_TRY(g->h_counts.ensure(sizeof(uint32_t) * np));
        uint32_t *h_counts = g->h_counts.as<uint32_t>();
        if (!src.plan && opt.raster_mode == 1) box_off = nullptr;         // (the band raster writes full frames)
        {                                                            // per-pose pixel boxes; raster + row counts + row scan
            SpanGuard sp(kSpanRender);
            PR_TRY(render_chunk(src, poses_host, p0, np, chunk, W, H, &job.proj, job.roi, box_off, !src.plan && opt.raster_mode == 1));
        }
        if (pyramid) { PR_TRY(pyramid_chunk(*pyramid, p0, np, W, H, K, box_off, sc, results_host + p0, job.robust)); continue; }
        // the cloud sizes come back through a kernel's stores into the pinned array, not through a copy command (see drive_host's result block)
        HIP_TRY(prk::launch_copy_words32(g->counts.p, g->h_counts.dev, np, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        trace_mark("refine_impl: render done, counts on host");
        uint32_t max_n = 0;
        for (uint32_t i = 0; i < np; ++i) max_n = std::max(max_n, h_counts[i]);
        // the clouds packed one behind the other, as in the asynchronous path (d2c_pack_starts_kernel; the host adds the same rounded sizes)
        size_t total = 0;
        for (uint32_t i = 0; i < np; ++i) {
            start[i] = (uint32_t)total; count[i] = h_counts[i];
            total += prk::cloud_slot(h_counts[i]);
        }
        if (total > 0xffffffffull) { set_error("pr_refine_batch: more than 2^32 cloud points in one chunk"); return PR_ERR_INVALID; }
        PR_TRY(g->cloud.ensure(sizeof(pr_vec3) * std::max<size_t>(4, total)));
        if (max_n > 0) {
            SpanGuard sp(kSpanCloud);
            PR_TRY(g->meta.ensure(sizeof(prk::PoseMeta) * np));
            HIP_TRY(prk::launch_d2c_pack_starts(g->counts.as<uint32_t>(), np, g->meta.as<prk::PoseMeta>(), g->stream));
            HIP_TRY(prk::launch_emit_box(g->depth.as<int32_t>(), np, W, H, g->bbox.as<int4>(), K[0], K[4], K[2], K[5],
                                         g->row_count.as<uint32_t>(), g->row_off.as<uint32_t>(), g->cloud.as<pr_vec3>(), g->meta.as<prk::PoseMeta>(), g->stream, box_off));
        }
        if (sizes_host) std::memcpy(sizes_host + p0, count.data(), sizeof(uint32_t) * np);
        trace_mark("refine_impl: clouds emitted, icp_drive next");
        if (info) {
            PR_TRY(info_drive(g->cloud.as<pr_vec3>(), start.data(), count.data(), np, sc, info->robust, info->centers + 3 * (size_t)p0, info->radii + p0,
                              info->info + p0, info->eig ? info->eig + p0 : nullptr));
            continue;
        }
        PR_TRY(icp_drive(g->cloud.as<pr_vec3>(), start.data(), count.data(), np, sc, job.crit,
                         results_host ? results_host + p0 : nullptr, job.results_dev ? job.results_dev + p0 : nullptr, job.robust[0]));
    }
    return PR_OK;
}
// ---- render-and-compare scoring (pr_score_poses) ---------------------------------------------------------------------------
// refine_core's render (staged poses, model box, per-pose pixel boxes packed one behind the other) followed by one kernel that compares every
// rendered box pixel with the scene frame.  Everything runs on the context's own stream and workspaces, which no asynchronous slot owns, so a
// batch pending on a slot is neither waited for nor disturbed.  The scene is read as it is on every call: nothing derived from it is kept.
// A block of records back to the caller: queue() = a kernel's stores into the pinned block (no copy command, see read_back_words), then -- after
// the caller's one hipStreamSynchronize for everything it queued -- deliver() copies the block's next `bytes` to where they are wanted.
struct ReadBack {
    const unsigned char *next = nullptr;
    int queue(const void *dev, const PinBuf &pinned, uint32_t n_words) { next = pinned.as<unsigned char>(); HIP_TRY(prk::launch_copy_words32(dev, pinned.dev, n_words, g->stream)); return PR_OK; }
    void deliver(void *host, size_t bytes) { std::memcpy(host, next, bytes); next += bytes; }
};
// One request (checked: score_request_ok; P > 0) on the hypotheses as req.poses has them: req.batch's, in its order.
// kScoreOverlap / req.overlap: the P x P matrix of shared inlier pixels, in the order of req.poses.  Every chunk also leaves
// its hypotheses' support bits (select.hip) and pixel boxes in workspaces sized for all P -- g->depth and g->bbox belong to the next chunk as soon
// as this one is scored -- and one launch over all pairs follows the last chunk.  The planes are dense: P x H x ceil(W / 64) words of 8 bytes.
// kScoreContours: the contour records of the same renders against the scene's edge distance image (contour.hip), one more
// kernel over every chunk's boxes right behind the score kernel; the records travel like the scores.
// kScoreContourFit: the silhouette's normal equations of the same renders against the scene's nearest-edge map (contour_fit.hip): the centres staged
// through the information pass' pinned block, one kernel over every chunk's boxes and one that adds its partial sums; the fit records travel like the
// scores, the pr_pose_info records are stored straight into the pinned block (info_drive's way).  req.scores may be null.
// kScoreNormals: the normal records of the same renders against the scene (normals.hip), one more kernel over every chunk's boxes right behind
// the score kernel; the records travel like the scores.
// kScoreCompose: the same renders taken together (compose.hip).  One more kernel over every chunk's boxes folds them into
// the key frame of the context -- the front-most render of every frame pixel with the CALLER's index of its hypothesis (Batch::order: grouped position ->
// caller's index, null: the identity), so ties and labels need no remapping -- and every chunk leaves its pixel boxes in a workspace sized for
// all P, as for the overlap matrix.  Behind the last chunk: the counts of what every hypothesis keeps, then one pass over the frame for the labels,
// the front depth and the frame record.  visible is written in the caller's order whatever `order` is.
// kScoreCover: the support bits and boxes as for the matrix, and behind every chunk's score kernel the walk's per-hypothesis state from its records
// (cover.hip).  Behind the last chunk the walk: rounds of gain + commit, kCoverRoundsPerSync of them enqueued at a time, then the finished word read
// back -- a round after the end is two launches that return at once, so how many are enqueued changes no byte -- at most min(max_keep, n_order) + 1
// in all; one more gain pass against the final claimed plane; the whole state back through pinned memory.  cov_order, the records and the selected
// list are in the order of req.poses (score_run maps a mixed batch).
constexpr uint32_t kCoverRoundsPerSync = 4;
int score_core(const ScoreRequest &req)
{
    const uint32_t P = req.P, W = req.W, H = req.H;
    const int32_t tau = req.tau;
    const bool contours = req.kind == kScoreContours, normals = req.kind == kScoreNormals, compose = req.kind == kScoreCompose, cover = req.kind == kScoreCover;
    const bool fit = req.kind == kScoreContourFit;
    const MeshSource &src = req.batch->src;
    const uint32_t *order = req.batch->order();                   // grouped position -> caller's index (null: the identity)
    static_assert(sizeof(pr_pose_visible) == sizeof(pr_pose_score) && sizeof(pr_frame_explained) == sizeof(pr_pose_score), "pr_pose_visible, pr_frame_explained: 32-byte records");
    static_assert(sizeof(pr_pose_contour) == sizeof(pr_pose_score) && offsetof(pr_pose_contour, dist_sum) == 24, "pr_pose_contour: one 32-byte record, the sum in words 6 and 7");
    static_assert(sizeof(pr_pose_normal) == sizeof(pr_pose_score), "pr_pose_normal: one 32-byte record");
    static_assert(sizeof(pr_contour_fit) == sizeof(pr_pose_score) && offsetof(pr_contour_fit, sum_d2) == 24, "pr_contour_fit: one 32-byte record, the sum in words 6 and 7");
    static_assert(sizeof(pr_pose_info) % sizeof(uint32_t) == 0, "pr_pose_info travels in 32-bit words");
    const prk::FitParams fit_params = fit ? prk::FitParams{ (double)req.K[0], (double)req.K[2], (double)req.K[4], (double)req.K[5], tau, req.jump } : prk::FitParams{};
    const uint32_t fit_nblk = prk::fit_blocks(H);
    const prk::NormalParams normal_params = normals ? prk::NormalParams{ (double)req.K[0], (double)req.K[2], (double)req.K[4], (double)req.K[5],
                                                                          (double)req.cos_min * (double)req.cos_min, req.step, req.jump, tau } : prk::NormalParams{};
    const bool has_roi = req.roi.width > 0 && req.roi.height > 0;
    const int4 window = has_roi ? make_int4(req.roi.x, req.roi.y, req.roi.x + req.roi.width - 1, req.roi.y + req.roi.height - 1) : make_int4(0, 0, (int)W - 1, (int)H - 1);
    constexpr uint32_t kWords = sizeof(pr_pose_score) / sizeof(uint32_t);
    static_assert(sizeof(pr_pose_score) == 32 && kWords == 8, "pr_pose_score: one 32-byte record");
    const size_t img = (size_t)W * H;
    const uint32_t chunk = depth_chunk(img, P);
    PR_TRY(model_boxes(src, chunk));
    const size_t plane_words = (size_t)H * prk::overlap_words_per_row(W);
    if (req.overlap || cover) {
        PR_TRY(g->ov_bits.ensure(sizeof(uint64_t) * plane_words * P));
        PR_TRY(g->ov_box.ensure(sizeof(int4) * P));
    }
    const prk::CoverRule &rule = req.cov_rule;
    const size_t cov_words = prk::CoverState::words(P, rule.n_order);
    if (cover) {
        static_assert(sizeof(pr_pose_cover) == 16 && sizeof(pr_cover_frame) == 16, "pr_pose_cover, pr_cover_frame: 16-byte records");
        if (cov_words > 0xffffffffull) { set_error("%s: too many hypotheses for one call", req.fn); return PR_ERR_INVALID; }
        PR_TRY(g->cov_state.ensure(sizeof(uint32_t) * cov_words));
        PR_TRY(g->cov_claimed.ensure(sizeof(uint64_t) * plane_words));
        PR_TRY(g->h_cov.ensure(sizeof(uint32_t) * cov_words));
    }
    const prk::CoverState cov(g->cov_state.as<uint32_t>(), P, rule.n_order), h_covs(g->h_cov.as<uint32_t>(), P, rule.n_order);
    if (cover) {                                                     // order position of every hypothesis and its inverse, staged behind whatever the stream holds
        std::fill(h_covs.pos, h_covs.pos + P, prk::kCoverNoPos);
        for (uint32_t k = 0; k < rule.n_order; ++k) { h_covs.pos[req.cov_order[k]] = k; h_covs.at[k] = req.cov_order[k]; }
        HIP_TRY(prk::launch_copy_words32(g->h_cov.dev_as<uint32_t>() + (h_covs.pos - h_covs.ctl), cov.pos, P + rule.n_order, g->stream));
        HIP_TRY(prk::launch_fill_i32(g->cov_claimed.as<int32_t>(), 2 * plane_words, 0, g->stream));
    }
    if (req.overlap) {
        PR_TRY(g->ov_mat.ensure(sizeof(uint32_t) * (size_t)P * P));
        PR_TRY(g->h_ov.ensure(sizeof(uint32_t) * (size_t)P * P));
    }
    // composition: records = P x pr_pose_visible, then the frame's; the pinned block holds them and, behind them, the index table on its way in
    const size_t cmp_rec_bytes = sizeof(pr_pose_visible) * ((size_t)P + 1), cmp_idx_bytes = (sizeof(uint32_t) * (size_t)P + 15) / 16 * 16;
    uint32_t *cmp_index = nullptr;                                  // device: grouped position -> caller's index (null: the identity)
    if (compose) {
        PR_TRY(g->cmp_keys.ensure(sizeof(uint64_t) * img));
        PR_TRY(g->cmp_box.ensure(sizeof(int4) * P + cmp_idx_bytes));
        PR_TRY(g->cmp_rec.ensure(cmp_rec_bytes));
        PR_TRY(g->h_cmp.ensure(cmp_rec_bytes + cmp_idx_bytes));
        if (order) {
            std::memcpy(g->h_cmp.as<unsigned char>() + cmp_rec_bytes, order, sizeof(uint32_t) * P);
            cmp_index = reinterpret_cast<uint32_t *>(g->cmp_box.as<int4>() + P);
            HIP_TRY(prk::launch_stage_words(g->h_cmp.dev_as<unsigned char>() + cmp_rec_bytes, cmp_index, sizeof(uint32_t) * P, g->stream));
        }
    }
    for (uint32_t p0 = 0; p0 < P; p0 += chunk) {
        const uint32_t np = std::min(chunk, P - p0);
        uint32_t *box_off = nullptr;
        PR_TRY(chunk_workspaces(img, H, np, box_off));
        PR_TRY(g->scores.ensure(sizeof(pr_pose_score) * np));
        PR_TRY(g->h_scores.ensure(sizeof(pr_pose_score) * np));
        if (contours) { PR_TRY(g->contours.ensure(sizeof(pr_pose_contour) * np)); PR_TRY(g->h_contours.ensure(sizeof(pr_pose_contour) * np)); }
        if (normals) { PR_TRY(g->normals.ensure(sizeof(pr_pose_normal) * np)); PR_TRY(g->h_normals.ensure(sizeof(pr_pose_normal) * np)); }
        if (fit) {                                                   // the contour check's record buffers and the information pass' workspaces: neither runs beside this kind
            PR_TRY(g->contours.ensure(sizeof(pr_contour_fit) * np)); PR_TRY(g->h_contours.ensure(sizeof(pr_contour_fit) * np));
            PR_TRY(g->info_meta.ensure(sizeof(prk::FitMeta) * np)); PR_TRY(g->h_info_meta.ensure(sizeof(prk::FitMeta) * np));
            PR_TRY(g->info_part.ensure(sizeof(double) * prk::kFitSums * (size_t)fit_nblk * np));
            PR_TRY(g->h_info_out.ensure(sizeof(pr_pose_info) * np));
        }
        {
            SpanGuard sp(kSpanRender);
            PR_TRY(render_chunk(src, req.poses, p0, np, chunk, W, H, req.proj, req.roi, box_off, /*bands=*/false));
        }
        // records zeroed by a kernel and read back through the pinned array by a kernel: no memset or copy commands on this path (see refine_core)
        ReadBack scores_back, contours_back, normals_back;
        HIP_TRY(prk::launch_fill_i32(g->scores.as<int32_t>(), (size_t)kWords * np, 0, g->stream));
        HIP_TRY(prk::launch_score_boxes(g->depth.as<int32_t>(), g->bbox.as<int4>(), box_off, np, W, H, req.scene, req.scene_i32, tau,
                                        g->scores.as<uint32_t>(), g->stream));
        if (contours) {
            HIP_TRY(prk::launch_fill_i32(g->contours.as<int32_t>(), (size_t)kWords * np, 0, g->stream));
            HIP_TRY(prk::launch_contour_boxes(g->depth.as<int32_t>(), g->bbox.as<int4>(), box_off, np, W, H, window, req.scene, req.scene_i32, req.edge_dist, tau,
                                              req.jump, g->contours.as<uint32_t>(), g->stream));
            PR_TRY(contours_back.queue(g->contours.p, g->h_contours, kWords * np));
        }
        if (fit) {
            std::memcpy(g->h_info_meta.p, req.fit_meta + p0, sizeof(prk::FitMeta) * np);
            HIP_TRY(prk::launch_stage_words(g->h_info_meta.dev, g->info_meta.p, sizeof(prk::FitMeta) * np, g->stream));
            HIP_TRY(prk::launch_fill_i32(g->contours.as<int32_t>(), (size_t)kWords * np, 0, g->stream));
            HIP_TRY(prk::launch_contour_fit(g->depth.as<int32_t>(), g->bbox.as<int4>(), box_off, np, W, H, window, req.scene, req.scene_i32, req.nearest,
                                            g->info_meta.as<prk::FitMeta>(), fit_params, g->contours.as<uint32_t>(), g->info_part.as<double>(),
                                            g->h_info_out.dev_as<pr_pose_info>(), g->stream));
            PR_TRY(contours_back.queue(g->contours.p, g->h_contours, kWords * np));
        }
        if (normals) {
            HIP_TRY(prk::launch_fill_i32(g->normals.as<int32_t>(), (size_t)kWords * np, 0, g->stream));
            HIP_TRY(prk::launch_normal_boxes(g->depth.as<int32_t>(), g->bbox.as<int4>(), box_off, np, W, H, window, req.scene, req.scene_i32, normal_params,
                                             g->normals.as<uint32_t>(), g->stream));
            PR_TRY(normals_back.queue(g->normals.p, g->h_normals, kWords * np));
        }
        if (req.overlap || cover) {
            HIP_TRY(prk::launch_support_bits(g->depth.as<int32_t>(), g->bbox.as<int4>(), box_off, np, W, H, req.scene, req.scene_i32, tau,
                                             g->ov_bits.as<unsigned long long>() + plane_words * p0, g->stream));
            HIP_TRY(prk::launch_copy_words32(g->bbox.p, g->ov_box.as<int4>() + p0, 4 * np, g->stream));
        }
        if (cover) HIP_TRY(prk::launch_cover_init(g->scores.as<uint32_t>(), p0, np, cov, g->stream));
        if (compose) {
            HIP_TRY(prk::launch_compose_tiles(g->depth.as<int32_t>(), g->bbox.as<int4>(), box_off, np, W, H, window, cmp_index ? cmp_index + p0 : nullptr, p0,
                                              g->cmp_keys.as<unsigned long long>(), p0 == 0, g->stream));
            HIP_TRY(prk::launch_copy_words32(g->bbox.p, g->cmp_box.as<int4>() + p0, 4 * np, g->stream));
        }
        PR_TRY(scores_back.queue(g->scores.p, g->h_scores, kWords * np));
        HIP_TRY(hipStreamSynchronize(g->stream));
        if (req.scores) scores_back.deliver(req.scores + p0, sizeof(pr_pose_score) * np);
        if (fit) {
            contours_back.deliver(req.fit + p0, sizeof(pr_contour_fit) * np);
            std::memcpy(req.fit_info + p0, g->h_info_out.p, sizeof(pr_pose_info) * np);
        }
        if (contours) contours_back.deliver(req.contours + p0, sizeof(pr_pose_contour) * np);
        if (normals) normals_back.deliver(req.normals + p0, sizeof(pr_pose_normal) * np);
    }
    if (req.overlap) {
        ReadBack back;
        HIP_TRY(prk::launch_pair_overlap(g->ov_bits.as<unsigned long long>(), g->ov_box.as<int4>(), P, W, H, g->ov_mat.as<uint32_t>(), g->stream));
        PR_TRY(back.queue(g->ov_mat.p, g->h_ov, P * P));
        HIP_TRY(hipStreamSynchronize(g->stream));
        back.deliver(req.overlap, sizeof(uint32_t) * (size_t)P * P);
    }
    if (cover) {
        const unsigned long long *planes = g->ov_bits.as<unsigned long long>();
        const uint32_t max_rounds = rule.n_order ? std::min(rule.max_keep, rule.n_order) + 1 : 0;
        for (uint32_t done = 0; done < max_rounds;) {
            const uint32_t n = std::min(kCoverRoundsPerSync, max_rounds - done);
            for (uint32_t k = 0; k < n; ++k)
                HIP_TRY(prk::launch_cover_round(planes, g->ov_box.as<int4>(), P, W, H, rule, cov, g->cov_claimed.as<unsigned long long>(), g->stream));
            done += n;
            uint32_t finished = 1;
            if (done < max_rounds) PR_TRY(read_back_words(cov.ctl, &finished, 1, g->stream));
            if (finished) break;
        }
        ReadBack back;
        HIP_TRY(prk::launch_cover_final(planes, g->ov_box.as<int4>(), P, W, H, cov, g->cov_claimed.as<unsigned long long>(), g->stream));
        PR_TRY(back.queue(cov.ctl, g->h_cov, (uint32_t)cov_words));
        HIP_TRY(hipStreamSynchronize(g->stream));
        const uint32_t n_sel = h_covs.ctl[1];
        std::memcpy(req.cover, h_covs.rec, sizeof(pr_pose_cover) * P);
        *req.cover_frame = pr_cover_frame{ h_covs.ctl[2], n_sel, { 0, 0 } };
        std::memcpy(req.selected, h_covs.selected, sizeof(uint32_t) * n_sel);
        *req.n_selected = n_sel;
    }
    if (compose) {
        ReadBack back;
        uint32_t *rec = g->cmp_rec.as<uint32_t>();
        HIP_TRY(prk::launch_fill_i32(g->cmp_rec.as<int32_t>(), cmp_rec_bytes / sizeof(int32_t), 0, g->stream));
        HIP_TRY(prk::launch_compose_counts(g->cmp_keys.as<unsigned long long>(), g->cmp_box.as<int4>(), cmp_index, P, W, H, req.scene, req.scene_i32, tau, rec, g->stream));
        HIP_TRY(prk::launch_compose_emit(g->cmp_keys.as<unsigned long long>(), W, H, window, req.scene, req.scene_i32, tau, req.labels_dev, req.depth_dev,
                                         rec + (size_t)kWords * P, g->stream));
        PR_TRY(back.queue(rec, g->h_cmp, (uint32_t)(cmp_rec_bytes / sizeof(uint32_t))));
        HIP_TRY(hipStreamSynchronize(g->stream));
        back.deliver(req.visible, sizeof(pr_pose_visible) * P);
        back.deliver(req.frame, sizeof(pr_frame_explained));
    }
    drain_spans();
    return PR_OK;
}

// ---- mixed batches: the entry points' bodies (a Batch in, outputs scattered back to the caller's order) ------------------------------------
// pr_refine_batch_multi and the pyramid entries behind their argument checks: refine_core on the batch in its order (job.mesh = b.src) into
// temporaries -- nothing reaches the caller's arrays unless the whole call succeeded -- and the records, cloud sizes and (py) per-level blocks
// back to the caller's order.
int refine_ordered(const RefineJob &job, const Batch &b, const PyramidPlan *py, pr_result *results_host, uint32_t *sizes_host)
{
    const uint32_t P = (uint32_t)b.P, L = py ? py->n_levels : 0;
    std::vector<pr_result> res(P), lres(py && py->level_results ? (size_t)L * P : 0);
    std::vector<uint32_t> sizes(P), lsizes(py && py->level_sizes ? (size_t)L * P : 0);
    const PyramidPlan inner{ py ? py->levels : nullptr, L, P, lres.empty() ? nullptr : lres.data(), lsizes.empty() ? nullptr : lsizes.data() };
    PR_TRY(refine_core(job, b.poses, P, res.data(), sizes.data(), py ? &inner : nullptr));
    b.scatter(res.data(), results_host);
    b.scatter(sizes.data(), sizes_host);
    if (py) { b.scatter(lres.data(), py->level_results, L); b.scatter(lsizes.data(), py->level_sizes, L); }
    return PR_OK;
}

// A checked request (score_request_ok; P > 0) on its prepared batch: score_core with the poses in the batch's order.  One mesh: the request as it
// is, into the caller's arrays.  A mesh table: into temporaries, and the scores, contours, normals, fit records and the matrix back to the caller's
// order -- nothing reaches the caller's arrays unless the call succeeded (the composition's records are written in the caller's order as they
// are: Batch::order).
int score_run(const ScoreRequest &req, const Batch &b)
{
    const uint32_t P = req.P;
    ScoreRequest run = req;
    run.batch = &b; run.poses = b.poses;
    std::vector<pr_pose_score> sc; std::vector<uint32_t> ov; std::vector<pr_pose_contour> cc; std::vector<pr_pose_normal> nn;
    std::vector<pr_contour_fit> ff; std::vector<pr_pose_info> fi; std::vector<prk::FitMeta> fm;
    run.scores = b.temp(sc, P, req.scores);
    if (req.overlap) run.overlap = b.temp(ov, (size_t)P * P, req.overlap);
    if (req.contours) run.contours = b.temp(cc, P, req.contours);
    if (req.normals) run.normals = b.temp(nn, P, req.normals);
    if (req.fit) { run.fit = b.temp(ff, P, req.fit); run.fit_info = b.temp(fi, P, req.fit_info); run.fit_meta = b.gather(req.fit_meta, fm); }
    // the cover walk of a mixed batch runs on grouped positions: the order goes in through the inverse, records and selected list come back through Batch::caller
    const bool walk_mixed = req.kind == kScoreCover && b.mixed;
    std::vector<uint32_t> walk(walk_mixed ? req.cov_rule.n_order : 0), chosen(walk.size());
    std::vector<pr_pose_cover> cv(walk_mixed ? P : 0);
    pr_cover_frame cf{};
    uint32_t n_chosen = 0;
    if (walk_mixed) {
        const std::vector<uint32_t> where = b.inverse();
        for (size_t k = 0; k < walk.size(); ++k) walk[k] = where[req.cov_order[k]];
        run.cov_order = walk.data(); run.cover = cv.data(); run.cover_frame = &cf; run.selected = chosen.data(); run.n_selected = &n_chosen;
    }
    PR_TRY(score_core(run));
    if (walk_mixed) {
        b.scatter(cv.data(), req.cover);
        for (uint32_t k = 0; k < n_chosen; ++k) req.selected[k] = b.caller(chosen[k]);
        *req.cover_frame = cf; *req.n_selected = n_chosen;
    }
    b.scatter(run.scores, req.scores);
    b.scatter(run.fit, req.fit); b.scatter(run.fit_info, req.fit_info);
    b.scatter(run.contours, req.contours);
    b.scatter(run.normals, req.normals);
    b.scatter_matrix(run.overlap, req.overlap);
    return PR_OK;
}
// Every scoring entry point behind PR_ENTER: the checks, then the batch (a mesh table's checks and grouping) and score_run
int score_call(const ScoreRequest &req)
{
    PR_TRY(score_request_ok(req));
    if (req.P == 0) { if (req.kind == kScoreCover && req.n_selected) *req.n_selected = 0; return PR_OK; }
    Batch b;
    PR_TRY(b.make(req.fn, req.mesh, req.poses, req.P));
    return score_run(req, b);
}
// ---- visible surface discrepancy (pr_pose_vsd, pr_pose_vsd_multi) ------------------------------------------------------------------------
// score_core's render (staged poses, model box, packed pixel boxes) of BOTH poses of every pair in one chunk, followed by one kernel that walks the
// union of a pair's two boxes against the scene frame (vsd.hip); the score kernel does not run and the records are per pair, so this is a
// small core of its own beside score_core.  Same stream, workspaces and read-back: a batch pending on a slot is neither waited for nor disturbed.
// renders: the pairs interleaved (estimate, truth, estimate, truth ...: 2 P poses; of a mixed batch, in its plan's order) -- or, with one_gt,
// the P estimates alone, and every chunk renders the one truth once, behind its estimates.  Chunks hold whole pairs.
int vsd_core(const MeshSource &src, const pr_mat4 *renders, const pr_mat4 *one_gt, uint32_t P, uint32_t W, uint32_t H, const pr_mat4 *proj,
             const void *scene, bool scene_i32, const prk::VsdParams &pm, pr_vsd_counts *out)
{
    constexpr uint32_t kWords = sizeof(pr_vsd_counts) / sizeof(uint32_t);
    static_assert(sizeof(pr_vsd_counts) == 64 && kWords == 4 + PR_VSD_MAX_TAUS, "pr_vsd_counts: sixteen counters");
    const size_t img = (size_t)W * H;
    const uint32_t cap = depth_chunk(img, one_gt ? P + 1 : 2 * P);                  // renders a chunk may hold: at least 2
    const uint32_t pairs_chunk = std::max(1u, one_gt ? cap - 1 : cap / 2), chunk = one_gt ? pairs_chunk + 1 : 2 * pairs_chunk;
    PR_TRY(model_boxes(src, chunk));
    std::vector<pr_mat4> with_gt(one_gt ? chunk : 0);
    for (uint32_t q0 = 0; q0 < P; q0 += pairs_chunk) {
        const uint32_t nq = std::min(pairs_chunk, P - q0), np = one_gt ? nq + 1 : 2 * nq;
        uint32_t *box_off = nullptr;
        PR_TRY(chunk_workspaces(img, H, np, box_off));
        PR_TRY(g->vsd_rec.ensure(sizeof(pr_vsd_counts) * nq));
        PR_TRY(g->h_vsd.ensure(sizeof(pr_vsd_counts) * nq));
        if (one_gt) { std::copy(renders + q0, renders + q0 + nq, with_gt.begin()); with_gt[nq] = *one_gt; }
        {
            SpanGuard sp(kSpanRender);
            PR_TRY(render_chunk(src, one_gt ? with_gt.data() : renders, one_gt ? 0 : 2 * q0, np, chunk, W, H, proj, pr_roi{ 0, 0, 0, 0 }, box_off, /*bands=*/false));
        }
        const prk::VsdPairing pairing = one_gt ? prk::VsdPairing{ 1, 0, nq } : prk::VsdPairing{ 2, 2, 1 };
        ReadBack back;
        HIP_TRY(prk::launch_fill_i32(g->vsd_rec.as<int32_t>(), (size_t)kWords * nq, 0, g->stream));
        HIP_TRY(prk::launch_vsd_boxes(g->depth.as<int32_t>(), g->bbox.as<int4>(), box_off, nq, pairing, W, H, scene, scene_i32, pm, g->vsd_rec.as<uint32_t>(), g->stream));
        PR_TRY(back.queue(g->vsd_rec.p, g->h_vsd, kWords * nq));
        HIP_TRY(hipStreamSynchronize(g->stream));
        back.deliver(out + q0, sizeof(pr_vsd_counts) * nq);
    }
    drain_spans();
    return PR_OK;
}
prk::VsdParams vsd_params(const float *K, float delta, const float *taus, uint32_t n_taus)
{
    prk::VsdParams pm{};
    pm.delta = delta; pm.n_taus = n_taus;
    for (uint32_t k = 0; k < n_taus; ++k) pm.tau[k] = taus[k];
    if (K) { pm.has_k = 1; pm.fx = K[0]; pm.cx = K[2]; pm.fy = K[4]; pm.cy = K[5]; }
    return pm;
}
// estimates and truths of as many pairs interleaved: the batch vsd_core renders
std::vector<pr_mat4> interleaved_pairs(const pr_mat4 *est, const pr_mat4 *gt, uint32_t P)
{
    std::vector<pr_mat4> out(2 * (size_t)P);
    for (uint32_t i = 0; i < P; ++i) { out[2 * (size_t)i] = est[i]; out[2 * (size_t)i + 1] = gt[i]; }
    return out;
}

// ---- interpenetration of hypotheses (pr_render_span, pr_pose_penetration, pr_pose_penetration_multi) -----------------------------------------------
// A small core beside vsd_core: the model box(es), the span render of all P hypotheses (checked: penetration_args_ok -- both planes are resident
// together, there are no chunks: render_chunk's layout for the whole call, the far plane in g->solid_far at the near one's box_off), one pair kernel
// (solid.hip), the P x P records back through pinned memory.  The context's own stream and workspaces: a batch pending on a slot is neither waited
// for nor disturbed.  out: in the order of `poses` (of a mixed batch: its plan's).
int solid_core(const MeshSource &src, const pr_mat4 *poses, uint32_t P, uint32_t W, uint32_t H, const pr_mat4 *proj, int32_t slack, pr_pair_solid *out)
{
    constexpr uint32_t kWords = sizeof(pr_pair_solid) / sizeof(uint32_t);
    static_assert(sizeof(pr_pair_solid) == 24 && kWords == 6 && offsetof(pr_pair_solid, sum_mm) == 16, "pr_pair_solid: four counters and a 64-bit sum");
    const size_t img = (size_t)W * H, n_rec = (size_t)P * P;
    uint32_t *box_off = nullptr;
    PR_TRY(model_boxes(src, P));
    PR_TRY(chunk_workspaces(img, H, P, box_off, /*rows=*/false));
    PR_TRY(g->solid_far.ensure(sizeof(int32_t) * (img + prk::kBoxPack) * P));
    PR_TRY(g->solid_rec.ensure(sizeof(pr_pair_solid) * n_rec));
    PR_TRY(g->h_solid.ensure(sizeof(pr_pair_solid) * n_rec));
    {
        SpanGuard sp(kSpanRender);
        PR_TRY(render_chunk(src, poses, 0, P, P, W, H, proj, pr_roi{ 0, 0, 0, 0 }, box_off, /*bands=*/false, g->solid_far.as<int32_t>()));
    }
    ReadBack back;
    HIP_TRY(prk::launch_pair_solid(g->depth.as<int32_t>(), g->solid_far.as<int32_t>(), g->bbox.as<int4>(), box_off, P, H, slack, g->solid_rec.as<uint32_t>(), g->stream));
    PR_TRY(back.queue(g->solid_rec.p, g->h_solid, (uint32_t)(kWords * n_rec)));
    HIP_TRY(hipStreamSynchronize(g->stream));
    back.deliver(out, sizeof(pr_pair_solid) * n_rec);
    drain_spans();
    return PR_OK;
}

// the request of an entry point from what all fourteen have in common, in the C arguments' order; the entry point's body adds the outputs of its kind
ScoreRequest score_request(const char *fn, ScoreKind kind, const MeshArg &mesh, const pr_mat4 *poses_host, uint32_t P, uint32_t W, uint32_t H, const pr_mat4 *proj, pr_roi roi,
                           const void *scene_dev, int depth_is_i32, int32_t tau, pr_pose_score *scores_host)
{
    ScoreRequest r{};
    r.fn = fn; r.kind = kind; r.mesh = mesh; r.poses = poses_host; r.P = P; r.W = W; r.H = H; r.proj = proj; r.roi = roi;
    r.scene = scene_dev; r.scene_i32 = depth_is_i32 != 0; r.tau = tau; r.scores = scores_host;
    return r;
}
// pr_render, pr_render_span and pr_render_multi: P full frames (or the ROI) of one mesh, or of a mesh table in the caller's order -- the hypotheses are
// grouped by mesh and the raster writes hypothesis j of the grouped batch into image Batch::caller(j).  The planes are filled by kernels, one raster pass draws
// into near_dev (the nearest fragment of every pixel) and, given far_dev, into it as well (the farthest), and (zero_empty) "nothing drawn" becomes 0
// in both.  Every check (render_args_ok, then the mesh table's) comes before anything is written.
int render_frames(const char *fn, const MeshArg &src, const pr_mat4 *poses_host, size_t P, size_t W, size_t H, const pr_mat4 *proj, pr_roi roi,
                  int32_t *near_dev, int32_t *far_dev, bool span, bool zero_empty)
{
    PR_TRY(render_args_ok(fn, src.multi, span, src.tris, src.n_tris, poses_host, P, W, H, proj, roi, near_dev, far_dev));
    if (P == 0) return PR_OK;
    Batch b;
    PR_TRY(b.make(fn, src, poses_host, P));
    const auto [rw, rh] = image_extent(roi, W, H);
    SpanGuard sp(kSpanRender);
    PR_TRY(stage_poses(b.poses, P));
    prk::RasterMesh mesh{};
    prk::RasterTarget t{};
    t.depth = near_dev; t.far = far_dev; t.rw = (uint32_t)rw; t.rh = (uint32_t)rh; t.roi = roi; t.width = (uint32_t)W; t.height = (uint32_t)H; t.proj = proj;
    if (b.mixed) {
        const MultiLayout l = multi_layout(b.pl.mesh.size(), P);     // the box-index slot holds the image of every hypothesis here
        PR_TRY(g->multi.ensure(l.bytes));
        PR_TRY(g->h_multi.ensure(l.bytes));
        PR_TRY(stage_groups(b.pl, 0, (uint32_t)P, (uint32_t)P, b.order(), mesh));
        t.image_of = mesh.box_index;
    } else { mesh.tris = src.tris; mesh.n_tris = (uint32_t)src.n_tris; }
    HIP_TRY(prk::launch_fill_i32(near_dev, P * rw * rh, INT32_MAX, g->stream));
    if (far_dev) HIP_TRY(prk::launch_fill_i32(far_dev, P * rw * rh, INT32_MIN, g->stream));
    HIP_TRY(prk::launch_raster(mesh, g->poses.as<pr_mat4>(), (uint32_t)P, t, nullptr, g->stream));
    if (zero_empty) HIP_TRY(prk::launch_sentinel2zero(near_dev, P * rw * rh, /*far=*/false, g->stream));
    if (zero_empty && far_dev) HIP_TRY(prk::launch_sentinel2zero(far_dev, P * rw * rh, /*far=*/true, g->stream));
    return PR_OK;
}

// ---- asynchronous fused refinement: two slots, everything of a batch enqueued without a host round trip -------------------
// The synchronous path above reads the cloud sizes back in the middle of a step (they size the cloud stride and the grid),
// uploads the start state and returns only after the results are in: ≈150 µs of a 1.3 ms step during which the GPU idles.
// Here the host computes the per-pose pixel boxes itself (pose_pixel_box, the function pose_bbox_kernel runs), which
// bounds every cloud by its box area, the start state is written by a kernel from the device-side counts, and a batch is
// only waited for when its results are wanted -- so the next batch can be enqueued while this one runs.
// The streams of BOTH slots are created together, in one run: main and first side stream of slot 0, then of slot 1.  Which
// hardware queue -- and with it which of the command processor's four pipes -- a stream lands on follows from the order in which
// the process created its queues (queue k -> pipe k mod 4), and two of these four streams on one pipe cost up to half the
// throughput (tools/queue_fairness.hip: two chains of dependent launches on one pipe take 2.1x a lone chain each, on two pipes
// 1.25x; bench.py with PR_STREAM_PADS-style gaps: 250 k -> 118-213 k poses/s).  Created lazily, slot by slot, anything the host does
// in between (its first synchronous copy creates the null stream's queue) shifts slot 1 onto slot 0's pipes; four queues
// created back to back always sit on four different pipes.  Further side streams (3-4 pose groups) come lazily, ensure_stream.
int slot_streams(Slot &sl)
{
    if (sl.stream) return PR_OK;
    for (Slot &o : g->slots) {
        if (o.stream || (!opt.eager_streams && &o != &sl)) continue;
        HIP_TRY(hipStreamCreateWithFlags(&o.stream, hipStreamNonBlocking));
        if (opt.eager_streams) PR_TRY(ensure_stream(o.side[0], &o.join[0]));
    }
    for (Slot &o : g->slots) {
        if (o.done) continue;
        HIP_TRY(hipEventCreateWithFlags(&o.scene_ready, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&o.fork, hipEventDisableTiming));
        // `done` is the one event a host thread waits on (pr_refine_wait): option "blocking_wait" makes that wait sleep instead of spin --
        // eight ranks spinning on a node whose cgroup grants sixteen CPUs leave nothing for RCCL's proxy threads
        HIP_TRY(hipEventCreateWithFlags(&o.done, hipEventDisableTiming | (opt.blocking_wait ? hipEventBlockingSync : 0u)));
        HIP_TRY(hipEventCreateWithFlags(&o.progress, hipEventDisableTiming));
    }
    return PR_OK;
}
// wait for everything a slot has in flight (its stream and side streams)
void slot_worker_wait(Slot &sl)      // the helper thread's batch, if one is running, has finished when this returns
{
    if (!sl.worker || !sl.worker_job) return;
    std::unique_lock<std::mutex> lk(sl.worker->mu);
    sl.worker->cv.wait(lk, [&] { return sl.worker->done || !sl.worker->alive; });
}
void slot_worker_stop(Slot &sl)
{
    if (!sl.worker) return;
    { std::lock_guard<std::mutex> lk(sl.worker->mu); sl.worker->quit = true; }
    sl.worker->cv.notify_all();
    if (sl.worker->th.joinable()) sl.worker->th.join();
    sl.worker.reset();
    sl.worker_job = false;
}
void slot_drain(Slot &sl)
{
    slot_worker_wait(sl);
    for (int i = 0; i < 3; ++i) if (sl.side[i]) (void)hipStreamSynchronize(sl.side[i]);
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);
}
void drain_all_slots()
{
    for (Slot &o : g->slots) if (o.pending && !o.delivered) slot_drain(o);
}
void drain_slots_reading(const void *p, size_t bytes)
{
    if (!p || bytes == 0) return;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
    auto hit = [&](const void *a, size_t ab) { const uintptr_t s = reinterpret_cast<uintptr_t>(a); return a && ab && s < hi && lo < s + ab; };
    for (Slot &sl : g->slots) {
        if (!sl.pending || sl.delivered) continue;
        const RefineJob &r = (sl.worker_job && sl.worker) ? sl.worker->in : sl.again;     // (a helper thread's job is posted and read under g->mu by this thread only)
        bool reads = hit(r.mesh.tris, r.mesh.n_tris * sizeof(pr_triangle)) || hit(r.results_dev, (size_t)sl.P * sizeof(pr_result));
        if (r.scene_kind == PR_SCENE_NN)
            reads = reads || hit(r.sn.pcd, (size_t)r.sn.n_points * sizeof(pr_vec3)) || hit(r.sn.normal, (size_t)r.sn.n_points * sizeof(pr_vec3)) ||
                    hit(r.sn.nodes, (size_t)r.sn.n_nodes * sizeof(pr_kdnode));
        else if (r.scene_kind == PR_SCENE_GRID)
            reads = reads || hit(r.sg.cell_point, (size_t)r.sg.dim[0] * r.sg.dim[1] * r.sg.dim[2] * sizeof(uint32_t)) || hit(r.sg.rec, (size_t)r.sg.n_points * 8 * sizeof(float));
        else {
            const size_t n = (size_t)r.sp.view.width * r.sp.view.height;
            reads = reads || hit(r.sp.view.pcd, n * sizeof(pr_vec3)) || hit(r.sp.view.normal, n * sizeof(pr_vec3));
        }
        if (reads) slot_drain(sl);
    }
}
void slot_release(Slot &sl)
{
    slot_drain(sl);
    slot_worker_stop(sl);
    for (DevBuf *b : { &sl.poses_bbox, &sl.depth, &sl.row_count, &sl.row_off, &sl.counts, &sl.cloud, &sl.meta, &sl.partial, &sl.dstate,
                       &sl.dresults, &sl.arrive, &sl.aabb_keys, &sl.nn_prev, &sl.packed.rec }) b->release();
    sl.packed = PackedCache();
    sl.h_in.release(); sl.h_out.release();
    for (int i = 0; i < 3; ++i) {
        if (sl.side[i]) hipStreamDestroy(sl.side[i]);
        if (sl.join[i]) hipEventDestroy(sl.join[i]);
        sl.side[i] = nullptr; sl.join[i] = nullptr;
    }
    if (sl.fork) hipEventDestroy(sl.fork);
    if (sl.done) hipEventDestroy(sl.done);
    if (sl.scene_ready) hipEventDestroy(sl.scene_ready);
    if (sl.progress) hipEventDestroy(sl.progress);
    sl.progress = nullptr; sl.progress_valid = false;
    if (sl.stream) hipStreamDestroy(sl.stream);
    sl.fork = sl.done = sl.scene_ready = nullptr; sl.stream = nullptr; sl.pending = false;
    sl.spans.destroy(); sl.timed = false;
}

// Host-side copy of a triangle buffer's box, once per (pointer, size): it feeds the per-pose pixel boxes computed on the host,
// which size a batch before anything of it has run.  With it (option mesh_order; from the buffer's second batch on) comes a copy of the triangles in spatial order
// (prh::mesh_order) in a buffer the context owns: what the asynchronous path's raster reads, because depth is a per-pixel minimum --
// no order of the triangles changes a pixel -- while the cost of its atomics is the number of 64-byte segments a wavefront's
// fragments touch (profiles/mesh_order).  Both are ASSUMPTIONS about memory the caller owns: every batch that uses them re-derives,
// from the CALLER's buffer on the device (one pass over the mesh, carried by the raster's first workgroups), the box and an
// order-independent fingerprint of every word (BatchCheck: the box alone would miss a rewrite that keeps the box), and refine_wait
// re-runs the batch through the synchronous path, which reads the caller's buffer only, if either differs -- a rewritten mesh costs
// one repeated batch, never a wrong one.
// Made with the ordered copy, from the same host copy, and valid exactly when it is: the buffer's distinct vertices (prh::mesh_vertices), which option
// tight_box's box kernel walks.  The fingerprint guards it as it guards the order -- and there it is what keeps a rewritten mesh from being CLIPPED.
// (An indexed form of the soup with a per-pose vertex stage was built and measured as well: three divergent 16-byte gathers
// per triangle cost the texture addresser more than the 170 saved VALU instructions give back -- 1.27 -> 1.32 ms per step.)
// a batch still pending on a slot's streams finishes first (it stays pending: pr_refine_wait collects it; a helper thread's batch runs on a context of its own)
int wait_pending_slots()
{
    for (Slot &o : g->slots) if (o.pending && !o.delivered && !o.worker_job && o.done) HIP_TRY(hipEventSynchronize(o.done));
    return PR_OK;
}
int ensure_model_box(const pr_triangle *tris_dev, size_t n_tris)
{
    // The ordered copy costs a host sort (35 ms for obj_06): it is made for a buffer that STAYS -- on the second batch in a row that finds the
    // same (pointer, size) -- so a caller that alternates between models on one context pays what it paid before (one read-back per batch).
    const bool seen = g->mesh_key == tris_dev && g->mesh_n == n_tris && g->aabb_host_valid;
    const bool want_copies = opt.mesh_order || opt.tight_box;
    if (seen && (!want_copies || g->mesh_sorted_valid)) return PR_OK;
    std::vector<pr_triangle> h(n_tris);
    if (n_tris) HIP_TRY(hipMemcpy(h.data(), tris_dev, sizeof(pr_triangle) * n_tris, hipMemcpyDeviceToHost));
    const float *f = reinterpret_cast<const float *>(h.data());
    float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    for (size_t v = 0; v < n_tris * 3; ++v)
        for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], f[3 * v + d]); hi[d] = fmaxf(hi[d], f[3 * v + d]); }
    for (int d = 0; d < 3; ++d) { g->aabb_host[d] = lo[d]; g->aabb_host[3 + d] = hi[d]; }
    g->mesh_hash = prh::mesh_fingerprint(h.data(), n_tris);
    g->mesh_sorted_valid = false; g->mesh_verts_n = 0;
    if (want_copies && seen && n_tris > 0 && n_tris <= 0xffffffffull) {
        std::vector<uint32_t> perm(n_tris);
        prh::mesh_order(h.data(), n_tris, perm.data());
        std::vector<pr_triangle> sorted(n_tris);
        for (size_t k = 0; k < n_tris; ++k) sorted[k] = h[perm[k]];
        // the other slot's batch may still be rastering the previous copy (another mesh, or a rewritten one): let it finish first
        PR_TRY(wait_pending_slots());
        PR_TRY(g->mesh_sorted.ensure(sizeof(pr_triangle) * n_tris));
        HIP_TRY(hipMemcpy(g->mesh_sorted.p, sorted.data(), sizeof(pr_triangle) * n_tris, hipMemcpyHostToDevice));
        // the buffer's distinct vertices, from the same host copy (option tight_box: what pose_tight_box_kernel walks; obj_06: 94 404 -> 15 736)
        std::vector<float4> verts;
        prh::mesh_vertices(h.data(), n_tris, verts);
        PR_TRY(g->mesh_verts.ensure(sizeof(float4) * verts.size()));
        HIP_TRY(hipMemcpy(g->mesh_verts.p, verts.data(), sizeof(float4) * verts.size(), hipMemcpyHostToDevice));
        g->mesh_verts_n = (uint32_t)verts.size();
        g->mesh_sorted_valid = true;
    }
    g->mesh_key = tris_dev; g->mesh_n = n_tris; g->aabb_host_valid = true;
    return PR_OK;
}

// the synchronous entry points run on whichever slot holds no unfinished batch of the caller's (-1: none)
int free_slot() { for (int i = 0; i < kSlots; ++i) if (!g->slots[i].pending) return i; return -1; }

int refine_wait(int slot)
{
    if (slot < 0 || slot >= kSlots) { set_error("slot must be 0..%d", kSlots - 1); return PR_ERR_INVALID; }
    Slot &sl = g->slots[slot];
    if (!sl.pending) { set_error("pr_refine_wait: nothing was submitted on slot %d", slot); return PR_ERR_INVALID; }
    if (sl.delivered) { sl.pending = false; return PR_OK; }
    if (sl.worker_job) {                                          // the batch ran on the slot's helper thread: collect its verdict
        slot_worker_wait(sl);
        sl.worker_job = false; sl.pending = false;
        std::lock_guard<std::mutex> lk(sl.worker->mu);
        if (!sl.worker->done) { set_error("pr_refine_wait: the slot's helper thread ended before its batch did"); return PR_ERR_HIP; }
        if (sl.worker->rc != PR_OK) set_error("%s", sl.worker->err.c_str());
        return sl.worker->rc;
    }
    {
        // the slot stays occupied until its batch has really finished: if the wait itself fails, everything the slot has in flight is
        // drained before the error goes back (a later submit must never reuse the slot's buffers under a running batch)
        const hipError_t we = hipEventSynchronize(sl.done);
        if (we != hipSuccess) { slot_drain(sl); sl.pending = false; set_error("pr_refine_wait: hipEventSynchronize failed: %s", hipGetErrorString(we)); return PR_ERR_HIP; }
    }
    sl.pending = false;
    const unsigned char *h_out = sl.h_out.as<unsigned char>();
    const SlotOut out(sl.P);
    if (*reinterpret_cast<const volatile uint32_t *>(h_out + out.flag) != 0u) {
        // the triangle buffer no longer has the box this batch was sized with, or the content its ordered copy was made from: forget both
        // and run the batch again, synchronously (that path derives every box on the device and reads the caller's buffer); outputs are overwritten in full
        g->drop_mesh();
        g->stat_repeated++;                                         // (pr_stats: the safety net is not free -- a caller that sees this count grow should call pr_invalidate)
        // (or a scene array no longer has the content its cached form was derived from: same cure)
        drain_all_slots();
        for (Slot &o : g->slots) o.packed.valid = false;
        g->packed.valid = false;
        for (NNDerived &d : g->nn_sets) { d.valid = false; d.grid_valid = false; }
        return refine_core(sl.again, sl.h_in.as<pr_mat4>(), sl.P, sl.user_results_host, sl.user_sizes);
    }
    const uint32_t *h_counts = sl.h_out.as<uint32_t>();
    uint32_t largest = 1;
    for (uint32_t i = 0; i < sl.P; ++i) largest = std::max(largest, h_counts[i]);
    g->cloud_hint = largest;
    if (sl.timed) { sl.spans.drain([&](uint32_t i) { return h_counts[i]; }); sl.timed = false; }     // the batch carried timing events: the same accounts as the synchronous timed path keeps
    if (sl.user_sizes) std::memcpy(sl.user_sizes, h_counts, sizeof(uint32_t) * sl.P);
    if (sl.user_results_host) std::memcpy(sl.user_results_host, h_out + out.res, sizeof(pr_result) * sl.P);
    return PR_OK;
}

// the helper thread of a slot: a private context on the slot's device, then one synchronous batch per job
void slot_worker_main(SlotWorker *w)
{
    bool ready = bind_shared(w->device) == PR_OK && pr_thread_context(1) == PR_OK;
    // the streams this thread's batches will run on -- its context's own and the first side stream (two pose groups) -- are created NOW, while the thread
    // that starts the helpers waits: the helpers of a context's slots are started one after the other (slot_worker_post), so their four streams get four
    // consecutive hardware queues = four different pipes of the command processor.  Created lazily by whichever helper came first, two of them could share a
    // pipe: the host-solve pipeline then ran at 208 k instead of 240-254 k poses/s, in about one process out of three (round 6, same box).
    if (ready) {
        std::lock_guard<std::mutex> ck(g->mu);
        ready = require_ctx() == PR_OK && ensure_stream(g->side[0], &g->ev_join[0]) == PR_OK;
    }
    { std::lock_guard<std::mutex> lk(w->mu); w->started = true; }
    w->cv.notify_all();
    for (;;) {
        std::unique_lock<std::mutex> lk(w->mu);
        w->cv.wait(lk, [&] { return w->has_job || w->quit; });
        if (w->quit) break;
        lk.unlock();
        trace_mark("worker: job taken");
        int rc = PR_ERR_HIP;
        if (!ready) set_error("the slot's helper thread could not create its context: %s", std::string(prh::g_err).c_str());
        else {
            std::lock_guard<std::mutex> ck(g->mu);
            rc = require_ctx();
            if (rc == PR_OK) rc = refine_core(w->in, w->poses.data(), (uint32_t)w->poses.size(), w->results_host, w->sizes_host);
        }
        trace_mark("worker: job done");
        lk.lock();
        w->rc = rc; w->err = (rc == PR_OK) ? std::string() : prh::g_err;
        w->has_job = false; w->done = true;
        lk.unlock();
        w->cv.notify_all();
    }
    if (ready) (void)pr_thread_context(0);
    { std::lock_guard<std::mutex> lk(w->mu); w->alive = false; }
    w->cv.notify_all();
}
int slot_worker_post(Slot &sl, const RefineJob &job, const pr_mat4 *poses_host, uint32_t P, pr_result *results_host, uint32_t *sizes_host)
{
    if (!sl.worker) {
        // the helpers of ALL slots of this context, one after the other, each with its streams made before the next one starts (see slot_worker_main)
        for (Slot &o : g->slots) {
            if (o.worker) continue;
            o.worker.reset(new SlotWorker());
            o.worker->device = g->device; o.worker->alive = true;
            try { o.worker->th = std::thread(slot_worker_main, o.worker.get()); }
            catch (...) { o.worker.reset(); if (&o == &sl) { set_error("pr_refine_submit: cannot start the slot's helper thread"); return PR_ERR_NOMEM; } continue; }
            std::unique_lock<std::mutex> lk(o.worker->mu);
            o.worker->cv.wait(lk, [&] { return o.worker->started; });
        }
    }
    SlotWorker &w = *sl.worker;
    {
        std::lock_guard<std::mutex> lk(w.mu);
        w.in = job;
        w.poses.assign(poses_host, poses_host + P);
        w.results_host = results_host; w.sizes_host = sizes_host;
        w.done = false; w.has_job = true;
    }
    w.cv.notify_all();
    return PR_OK;
}

// ---- refine_submit_async, phase by phase ------------------------------------------------------------------------------------------------
// The slot's streams, and the batch's scene on the stream that is idle until the loop forks.  The packed copy of the scene does not depend on the
// render: when it has to be (re)built that happens on the first side stream, the loop waits for it (scene_ready); batches without pose groups
// build it in line.
int async_scene(Slot &sl, const RefineJob &job, uint32_t P, SceneSel &sc, hipStream_t &scene_stream)
{
    PR_TRY(slot_streams(sl));
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    const uint32_t groups_hint = std::max(1u, std::min({ pose_groups_for(job.scene_kind), 4u, std::min<uint32_t>(P, (uint32_t)std::max(32, opt.sub_batch)) / 32u }));
    for (uint32_t k = 1; k < groups_hint; ++k) PR_TRY(ensure_stream(sl.side[k - 1], &sl.join[k - 1]));
    scene_stream = groups_hint > 1 ? sl.side[0] : sl.stream;
    const Camera cam{ job.W, job.H, job.K[0], job.K[4], job.K[2], job.K[5] };            // kd-tree scenes: the pixel grid of the scene points under this camera
    // nothing of this batch may run beside the loop of a TIMED batch on the other slot -- not even the small checks on the scene stream
    if (scene_stream != sl.stream)
        for (Slot &o : g->slots) if (&o != &sl && o.pending && !o.delivered && o.timed && o.progress_valid) HIP_TRY(hipStreamWaitEvent(scene_stream, o.progress, 0));
    PR_TRY(make_scene(job.scene_kind, job.scene(), /*want_packed=*/true, sc, &sl.packed, scene_stream, job.scene_kind == PR_SCENE_NN ? &cam : nullptr, /*verify_now=*/false));
    sl.nn_set = (job.scene_kind == PR_SCENE_NN) ? sc.nn_set : -1;        // (what make_scene must not rebuild under this batch while it is in flight)
    return PR_OK;
}
// The record of the batch's stale-cache checks: the model box and the mesh fingerprint the host assumed (ensure_model_box) and, with option
// scene_cache, the caller's scene arrays against the fingerprint taken when their cached form was built.  Every batch checks both against the
// buffers' present content (refine_wait acts on the flag).  Round 5: both checks ride on the raster launch (BatchCheck, pr_internal.h) -- as
// launches of their own on the scene stream (a memset, two box kernels, the fingerprint kernel) they cost 1.3-1.5 % of the headline whatever
// their number (skipped: 277.6 against 273.6 k poses/s on one box; fused into one launch: 274.1 k).
prk::BatchCheck batch_check(const Slot &sl, const RefineJob &job, const SceneSel &sc, uint32_t *flag_dev)
{
    prk::BatchCheck chk{};
    chk.keys = sl.aabb_keys.as<uint32_t>();
    for (int a = 0; a < 6; ++a) chk.expect.v[a] = g->aabb_host[a];
    chk.caller = job.mesh.tris; chk.mesh_hash = g->mesh_hash;
    chk.flag = flag_dev;
    if (!opt.scene_cache) return chk;
    if (job.scene_kind == PR_SCENE_NN)
        prk::check_sources(chk, prk::scene_sources(job.sn), &g->nn_sets[sc.nn_set].nndepth.as<prk::NNInfo>()->fp.sample);
    else if (sl.packed.valid)
        prk::check_sources(chk, prk::scene_sources(job.sp.view), &sl.packed.at<ProjTail>(packed_layout(job.sp.view.width, job.sp.view.height).tail)->fp.sample);
    return chk;
}
// What the phases of one asynchronous batch share: the batch, its plan and where its parts live on the device.
struct AsyncBatch {
    Slot &sl; const RefineJob &job; uint32_t P;
    SceneSel sc; AsyncPlan pl{}; NNLayout nl{}; prk::BatchCheck chk{};
    uint32_t *nn_prev = nullptr;                                  // kd-tree scene: the search workspace (nn_layout), or null
    pr_result *dres = nullptr;
    bool timed = false, tight = false, bands = false, pipeline_start = true;
    pr_mat4 *d_poses = nullptr; int4 *d_box = nullptr; uint32_t *d_off = nullptr;      // SlotIn on the device
    const pr_triangle *raster_tris = nullptr;
    int workspaces(); int stage(); int sub_batch(uint32_t q0, uint32_t nq);
};
// the slot's workspaces for the plan (the depth workspace, which the plan's offsets index, first)
int AsyncBatch::workspaces()
{
    const uint32_t sub = pl.sub;
    PR_TRY(sl.depth.ensure(sizeof(int32_t) * depth_ints_per_pose(job.W, job.H, bands) * sub));
    PR_TRY(sl.row_count.ensure(sizeof(uint32_t) * (size_t)job.H * sub));
    PR_TRY(sl.row_off.ensure(sizeof(uint32_t) * (size_t)job.H * sub));
    PR_TRY(sl.counts.ensure(sizeof(uint32_t) * P));
    PR_TRY(sl.cloud.ensure(sizeof(pr_vec3) * pl.cstride * sub));
    PR_TRY(sl.meta.ensure(sizeof(prk::PoseMeta) * P));
    PR_TRY(sl.partial.ensure(sizeof(float) * prk::kAccStride * (size_t)pl.nblk * sub));
    PR_TRY(sl.dstate.ensure(sizeof(prk::DevIcpState) * P));
    PR_TRY(sl.arrive.ensure(sizeof(uint32_t) * P));
    dres = job.results_dev;
    if (!dres) { PR_TRY(sl.dresults.ensure(sizeof(pr_result) * P)); dres = sl.dresults.as<pr_result>(); }
    // kd-tree scene: the workspace (nn_layout, as icp_drive) indexed like the clouds of one sub-batch; the search kernel's grid comes from the
    // box bound, surplus workgroups exit at once
    nl = nn_layout(pl.cstride * (size_t)sub, sub);
    if (sc.kind == PR_SCENE_NN) {
        sc.nn_split = nn_split_for(sc);
        sc.nn_max_points = (uint32_t)std::min<size_t>(pl.max_area, 0xffffffffu);
        if (sc.nn.rec32 && (opt.nn_seed || sc.nn_split)) {
            PR_TRY(sl.nn_prev.ensure(nl.bytes));
            nn_prev = sl.nn_prev.as<uint32_t>();
        }
    }
    return PR_OK;
}
// the inputs onto the device, behind the other slot's release point
int AsyncBatch::stage()
{
    const SlotIn in(P);
    hipStream_t st = sl.stream;
    d_poses = sl.poses_bbox.as<pr_mat4>();
    d_box = reinterpret_cast<int4 *>(sl.poses_bbox.as<unsigned char>() + in.box);
    d_off = reinterpret_cast<uint32_t *>(sl.poses_bbox.as<unsigned char>() + in.off);
    // this batch's render is held back until the other slot has issued the release pass of its loop (release_pass_for)
    for (Slot &o : g->slots)
        if (&o != &sl && o.pending && !o.delivered && o.progress_valid) HIP_TRY(hipStreamWaitEvent(st, o.progress, 0));
    sl.progress_valid = false;
    HIP_TRY(prk::launch_stage_words(sl.h_in.dev, d_poses, in.bytes, st));
    // Option tight_box: the uploaded boxes are the LOOSE ones (hull of the projected corners of the mesh's box) -- they sized everything above.  On the
    // device each is replaced by its intersection with the hull of the mesh's projected vertices (57 % of the pixels for obj_06), and the packed
    // offsets of each sub-batch are formed again from those: what fill, raster, count and emit then walk.  Never larger than the loose box, so
    // every capacity holds; no host round trip.  Needs the context's vertex list (ensure_model_box: from the buffer's second batch on).
    tight = opt.tight_box && g->mesh_sorted_valid && g->mesh_verts_n > 0;
    if (tight) {
        HIP_TRY(prk::launch_tight_boxes(g->mesh_verts.as<float4>(), g->mesh_verts_n, d_poses, P, job.proj, job.W, job.H, d_box, st));
        g_tight_batches.fetch_add(1);
    }
    // the raster's triangles: the context's ordered copy (same triangles, same minima; the first render's checks read the caller's buffer)
    raster_tris = (opt.mesh_order && g->mesh_sorted_valid) ? g->mesh_sorted.as<pr_triangle>() : job.mesh.tris;
    return PR_OK;
}
// one sub-batch, hypotheses [q0, q0 + nq): render, emit, the iteration loop
int AsyncBatch::sub_batch(uint32_t q0, uint32_t nq)
{
    const uint32_t W = job.W, H = job.H;
    const float *K = job.K;
    hipStream_t st = sl.stream;
    prk::PoseMeta *meta = sl.meta.as<prk::PoseMeta>() + q0;
    prk::DevIcpState *dstate = sl.dstate.as<prk::DevIcpState>() + q0;
    uint32_t *arrive = sl.arrive.as<uint32_t>() + q0;
    const pr_roi none{ 0, 0, 0, 0 };                              // the ROI is already part of the host-computed boxes
    size_t te = timed ? sl.spans.begin(st) : kNoEvent;
    // (the first render carries the batch's checks: the fingerprint's expected value belongs to the scene build, so the scene comes first --
    // an event that is complete when recorded unless a cache missed)
    // (ADVICE r05 asked whether this wait costs a rebuilt scene its overlap with the render: it does not -- make_scene reads the rebuilt form's
    // `exact` flag / tree depth back before it returns, so a rebuild has finished on the host's clock before the render is even enqueued; on a
    // cache hit the event is complete when recorded)
    if (q0 == 0) HIP_TRY(hipStreamWaitEvent(st, sl.scene_ready, 0));
    if (tight) HIP_TRY(prk::launch_box_pack_offsets(d_box + q0, nq, d_off + q0, H, bands, st));
    prk::RasterMesh mesh{};
    mesh.tris = raster_tris; mesh.n_tris = (uint32_t)job.mesh.n_tris;
    prk::RasterTarget target{};
    target.depth = sl.depth.as<int32_t>(); target.box_off = d_off + q0; target.roi = none; target.bands = bands; target.width = W; target.height = H; target.proj = &job.proj;
    const prk::BoxRows rows{ sl.row_count.as<uint32_t>(), sl.row_off.as<uint32_t>(), sl.counts.as<uint32_t>() + q0, meta, dstate, arrive };
    HIP_TRY(prk::launch_render_boxes(mesh, d_poses + q0, nq, d_box + q0, target, rows, st, /*compute_boxes=*/false, q0 == 0 ? &chk : nullptr));
    if (timed) { sl.spans.end(te, kSpanRender, q0, nq, false, st); te = sl.spans.begin(st); }
    HIP_TRY(prk::launch_emit_box(sl.depth.as<int32_t>(), nq, W, H, d_box + q0, K[0], K[4], K[2], K[5], sl.row_count.as<uint32_t>(),
                                 sl.row_off.as<uint32_t>(), sl.cloud.as<pr_vec3>(), meta, st, d_off + q0, bands));
    if (timed) sl.spans.end(te, kSpanCloud, q0, nq, false, st);
    if (timed && q0 == 0)                                     // the timed loop starts when the other slot's batch is complete
        for (Slot &o : g->slots) if (&o != &sl && o.pending && !o.delivered && o.done) HIP_TRY(hipStreamWaitEvent(st, o.done, 0));

    const uint32_t n_groups = pose_group_count(job.scene_kind, nq, timed);
    if (nn_prev) HIP_TRY(prk::launch_fill_i32(reinterpret_cast<int32_t *>(nn_prev + nl.qcount), (size_t)prk::kQCountStride * nq, 0, st));
    prk::IcpBatch b{};
    b.cloud = sl.cloud.as<pr_vec3>(); b.partial = sl.partial.as<float>(); b.nblk = pl.nblk; b.grid_x = pl.grid_x; b.steps = pl.steps;
    if (nn_prev) nn_carve(b, nn_prev, nl);
    const uint32_t last_pass = (uint32_t)job.crit.max_iteration;
    // Option resident_loop: every pass of the sub-batch in ONE launch on the slot's stream, a 1024- or 512-lane workgroup per hypothesis (icp_loop_cu_kernel) --
    // no pose groups, no arrival counters, no partial sums in memory.  Packed projective scene and fused device solve only (this path carries no
    // robust weight); a timed batch keeps its per-launch events, and a plan whose blocks would not fit the kernel's LDS keeps the multi-launch loop.
    // The other slot's render is released AHEAD of the launch and runs beside the loop (PR_RESIDENT_RELEASE_AHEAD, pr_tuning.h: behind it measured
    // 302 against 332 k poses/s); overlap_pass has no pass to name here and keeps its meaning for the multi-launch loop.
    if (opt.resident_loop && opt.fused_solve && !timed && job.scene_kind == PR_SCENE_PROJ && sc.kind == PR_SCENE_PROJ && sc.packed
        && prk::icp_loop_cu_lds_bytes(pl.nblk) <= prk::kLoopCuLdsBudget) {
        b.meta = meta; b.st = dstate; b.crit = job.crit; b.fused = 1;
        const bool release = q0 + pl.sub >= P;
#if PR_RESIDENT_RELEASE_AHEAD
        if (release) { HIP_TRY(hipEventRecord(sl.progress, st)); sl.progress_valid = true; }
#endif
        // Option loop_lds_blocks: the head of every cloud stays in the workgroup's LDS over the loop.  Those points of sl.cloud are stale afterwards,
        // and nobody looks: the slot's cloud buffer is written by the emit above and read by this launch only (the next sub-batch's emit overwrites it).
        b.lds_blocks = prk::icp_loop_cu_lds_blocks(pl.nblk, pl.steps, opt.loop_lds_blocks);
        // Option loop_waves: 8-wave workgroups, two to a compute unit, only for a sub-batch that fills the chip (one hypothesis per compute unit
        // at least); a smaller one keeps the sixteen wavefronts and their lower latency.  Option loop_lds_tables: colf / rowf in LDS.
        const uint32_t waves = opt.loop_waves ? (uint32_t)opt.loop_waves : (nq >= (uint32_t)g->n_cus ? PR_LOOP_CU_FULL_CHIP_WAVES : 16u);
        prk::LoopCuUsed used{};
        HIP_TRY(prk::launch_icp_loop_cu_proj_packed(b, sc.pk, nq, st, prk::LoopCuForm{ waves, opt.loop_lds_tables }, &used));
        g_loop_lds_blocks.store(used.lds_blocks);
        g_loop_waves.store(used.waves);
        g_loop_lds_tables.store(used.table_bytes);
#if !PR_RESIDENT_RELEASE_AHEAD
        if (release) { HIP_TRY(hipEventRecord(sl.progress, st)); sl.progress_valid = true; }
#endif
        g_resident_batches.fetch_add(1);
        return PR_OK;
    }
    auto pass = [&](const prk::IcpBatch &bb, uint32_t p0, uint32_t np, hipStream_t gs) -> int {
        if (!timed) { HIP_TRY(launch_pass(bb, sc, np, gs)); return PR_OK; }
        const size_t e0 = sl.spans.begin(st);                    // (one group: gs == st)
        // a kd-tree pass is four kernels: three more events between them give each kernel's own time (pr_profile_nn)
        size_t mi[3] = { 0, 0, 0 }; hipEvent_t me[3] = { nullptr, nullptr, nullptr };
        const bool marks = sc.kind == PR_SCENE_NN && sc.nn_split && bb.nn_prev && np <= 32768u && sl.spans.reserve_marks(mi, me);
        HIP_TRY(launch_pass(bb, sc, np, gs, marks ? me : nullptr));
        sl.spans.end(e0, kSpanIcp, q0 + p0, np, bb.iter == 0 || bb.iter == last_pass, st, marks ? mi : nullptr);
        return PR_OK;
    };
    // the pass of the batch's last sub-batch behind which the other slot's render may start
    const uint32_t release_pass = release_pass_for(job.mesh.n_tris, nq, g->cloud_hint, job.crit, job.scene_kind, timed, pipeline_start, opt.start_overlap, opt.overlap_pass);
    auto after = [&](uint32_t it, bool &) -> int {
        if (q0 + pl.sub >= P && it == release_pass) { HIP_TRY(hipEventRecord(sl.progress, st)); sl.progress_valid = true; }
        return PR_OK;
    };
    // the iteration loop: (max_iteration+1) x [pass (+ fused finalize/solve)], pose groups on the slot's side streams
    const Lanes lanes{ sl.stream, sl.side, sl.fork, sl.join };
    return device_solve_loop(lanes, n_groups, b, nq, job.crit, opt.fused_solve != 0, meta, dstate, arrive, pass, after);
}
// everything of a batch onto the slot's streams; the poses are in sl.h_in already (refine_submit).  Streams and scene, plan, workspaces, staging,
// then sub-batch by sub-batch render -> emit -> loop, the export and the done event.
int refine_submit_async(Slot &sl, const RefineJob &job, uint32_t P, pr_result *results_host)
{
    AsyncBatch a{ sl, job, P };
    hipStream_t scene_stream = nullptr;
    PR_TRY(async_scene(sl, job, P, a.sc, scene_stream));
    PR_TRY(ensure_model_box(job.mesh.tris, job.mesh.n_tris));             // once per triangle buffer ...
    const SlotIn in(P);
    const SlotOut out(P);
    PR_TRY(sl.h_out.ensure(out.bytes));
    unsigned char *h_out_dev = sl.h_out.dev_as<unsigned char>();  // the pinned block as the device sees it
    HIP_TRY(hipEventRecord(sl.scene_ready, scene_stream));      // (complete as it is recorded unless a cache missed and the scene is being rebuilt on this stream)
    // ... and checked against the buffer's present content by every batch, together with the scene caches (batch_check)
    const bool keys_new = sl.aabb_keys.p == nullptr;
    PR_TRY(sl.aabb_keys.ensure(prk::kBatchCheckWords * sizeof(uint32_t)));
    if (keys_new) {                                               // armed once; the last workgroup of every check re-arms the words itself
        HIP_TRY(hipMemsetAsync(sl.aabb_keys.p, 0xff, 6 * sizeof(uint32_t), sl.stream));
        HIP_TRY(hipMemsetAsync(sl.aabb_keys.as<uint32_t>() + 6, 0, (prk::kBatchCheckWords - 6) * sizeof(uint32_t), sl.stream));
    }
    *reinterpret_cast<volatile uint32_t *>(sl.h_out.as<unsigned char>() + out.flag) = 0u;
    a.chk = batch_check(sl, job, a.sc, reinterpret_cast<uint32_t *>(h_out_dev + out.flag));

    // the plan (SlotIn: poses | pixel boxes | offsets of the packed boxes): the host computes the boxes, the largest one sizes the clouds and the grid
    PR_TRY(sl.poses_bbox.ensure(in.bytes + 16));
    const pr_mat4 *h_poses = sl.h_in.as<pr_mat4>();
    int4 *h_box = reinterpret_cast<int4 *>(sl.h_in.as<unsigned char>() + in.box);
    for (uint32_t i = 0; i < P; ++i) h_box[i] = prk::pose_pixel_box(g->aabb_host, h_poses[i].m, job.proj, job.W, job.H, job.roi);
    // Option box_bands: the depth boxes of this batch interleave four image rows (pose_box.h, band_box) -- the plan places them, fill, raster, count and
    // emit address them; private to this path, every output the same bytes as with row-major boxes
    a.bands = opt.box_bands != 0;
    if (a.bands) g_band_batches.fetch_add(1);
    a.pl = plan_async(P, job.W, job.H, h_box, opt.steps, opt.sub_batch, g->cloud_hint, reinterpret_cast<uint32_t *>(sl.h_in.as<unsigned char>() + in.off), a.bands);
    PR_TRY(a.workspaces());

    // A TIMED batch (profile 3) stays asynchronous: its render runs under the other slot's loop like any other, but its own loop waits
    // until the other slot's batch is complete, runs as ONE pose group, lets the other slot's next render start only when it has
    // finished, and carries HIP events around every launch (sl.spans) -- the timed launches have the chip to themselves as in the synchronous
    // timed path (profile 1), without that path's host round trips and its idle render.
    a.timed = sl.timed = (opt.profile == 3);
    sl.spans.reset();
    // A batch submitted while the other slot is idle starts a pipeline.  Option start_overlap says when the NEXT batch's render may start
    // in that case: -1 (default) = by release_pass_for's rule, like any other batch; a pass number releases it earlier (see the option's note).
    for (Slot &o : g->slots) if (&o != &sl && o.pending && !o.delivered) a.pipeline_start = false;
    PR_TRY(a.stage());
    for (uint32_t q0 = 0; q0 < P; q0 += a.pl.sub) PR_TRY(a.sub_batch(q0, std::min(a.pl.sub, P - q0)));
    HIP_TRY(prk::launch_pack_export(sl.dstate.as<prk::DevIcpState>(), a.dres, sl.counts.as<uint32_t>(), reinterpret_cast<uint32_t *>(h_out_dev),
                                    results_host ? reinterpret_cast<pr_result *>(h_out_dev + out.res) : nullptr, P, sl.stream));
    HIP_TRY(hipEventRecord(sl.done, sl.stream));
    return PR_OK;
}

// may a batch be submitted on this slot?
int slot_idle(int slot)
{
    if (slot < 0 || slot >= kSlots) { set_error("slot must be 0..%d", kSlots - 1); return PR_ERR_INVALID; }
    if (g->slots[slot].pending) { set_error("pr_refine_submit: slot %d still holds an unfinished batch (call pr_refine_wait)", slot); return PR_ERR_INVALID; }
    return PR_OK;
}
// a batch onto an idle slot: enqueued on the slot's streams, handed to its helper thread, or run to completion here
int refine_submit(Slot &sl, const RefineJob &job, const pr_mat4 *poses_host, uint32_t P, pr_result *results_host, uint32_t *sizes_host)
{
    if (!poses_host || (!results_host && !job.results_dev)) { set_error("pr_refine_submit: bad arguments"); return PR_ERR_INVALID; }
    sl.P = P; sl.user_results_host = results_host; sl.user_sizes = sizes_host; sl.delivered = false;
    const uint64_t period = (uint64_t)std::max(1, opt.sample_period);
    const bool sample_call = (opt.profile == 2) && (g->sample_clock % period == 0);
    // (an instrumented kd-tree run stays synchronous; large frames: the asynchronous path sizes its sub-batches to its workspace bound)
    const bool async_ok = P > 0 && opt.solve_mode == PR_SOLVE_DEVICE && opt.raster_mode == 0 && (job.scene_kind != PR_SCENE_NN || !opt.nn_count)
                          && job.scene_kind != PR_SCENE_GRID      // (a grid scene takes the synchronous route: its bytes are pr_refine_batch's by construction)
                          && (opt.profile == 0 || opt.profile == 3 || (opt.profile == 2 && !sample_call));
    if (!async_ok && P > 0 && opt.solve_mode == PR_SOLVE_HOST && opt.host_worker && opt.profile == 0 && !opt.nn_count && !tl_sums_trace.active.rows) {   // (a traced batch runs on the thread that armed the recorder)
        // host solve, nothing to time: the batch goes to the slot's helper thread (see SlotWorker) and this call returns
        PR_TRY(slot_worker_post(sl, job, poses_host, P, results_host, sizes_host));
        sl.pending = true; sl.delivered = false; sl.worker_job = true;
        return PR_OK;
    }
    if (!async_ok) {
        // the synchronous path (host solve, timed calls, oversized batches): let the other slot drain first so
        // that a timed launch has the chip to itself, then run to completion; pr_refine_wait has nothing left to do
        for (Slot &o : g->slots) if (o.pending && !o.delivered && o.done) HIP_TRY(hipEventSynchronize(o.done));
        PR_TRY(refine_core(job, poses_host, P, results_host, sizes_host));
        sl.pending = true; sl.delivered = true;
        return PR_OK;
    }
    g->sample_clock++;
    // the host copies of this batch's inputs (the poses are staged from here; the rest is what a re-run needs)
    PR_TRY(sl.h_in.ensure(SlotIn(P).bytes + 16));
    std::memcpy(sl.h_in.p, poses_host, sizeof(pr_mat4) * P);
    sl.again = job;
    const int rc = refine_submit_async(sl, job, P, results_host);
    if (rc != PR_OK) {                                            // part of the batch may already be queued: do not leave it running
        slot_drain(sl);                                           // behind the caller's back (its buffers may go away next)
        sl.pending = false;
        return rc;
    }
    sl.pending = true;
    return PR_OK;
}

}  // namespace prr

using namespace prr;

// ---- the bodies of the entry points that exist for one mesh and for a mesh table: each takes the mesh as a MeshArg, and its extern "C" forms
// below only name it.  What is PR_TRY'd before PR_ENTER() needs no device and is refused on a machine without one.
static int render_call(const char *fn, const MeshArg &mesh, const pr_mat4 *poses_host, size_t n_poses, size_t width, size_t height, const pr_mat4 *proj, pr_roi roi,
                       int32_t *near_dev_out, int32_t *far_dev_out, bool span)
{
    PR_ENTER();
    const auto [rw, rh] = image_extent(roi, width, height);
    if (near_dev_out) note_write(near_dev_out, sizeof(int32_t) * n_poses * rw * rh);
    if (far_dev_out) note_write(far_dev_out, sizeof(int32_t) * n_poses * rw * rh);
    PR_TRY(render_frames(fn, mesh, poses_host, n_poses, width, height, proj, roi, near_dev_out, far_dev_out, span, true));
    HIP_TRY(hipStreamSynchronize(g->stream));            // renderer.cu:295 cudaDeviceSynchronize
    drain_spans();
    return PR_OK;
}
// the scoring kinds: the request (score_request) with the outputs of its kind added, then score_call
static int score_poses(const ScoreRequest &r) { PR_ENTER(); return score_call(r); }
static int score_overlap(ScoreRequest r, uint32_t *overlap_host) { PR_ENTER(); r.overlap = overlap_host; return score_call(r); }
static int score_cover(ScoreRequest r, const uint32_t *order, uint32_t n_order, uint32_t new_num, uint32_t new_den, uint32_t min_new, uint32_t max_keep,
                       pr_pose_cover *cover_host, pr_cover_frame *frame_host, uint32_t *selected_out, uint32_t *n_selected)
{
    PR_ENTER();
    r.cov_order = order; r.cov_rule = prk::CoverRule{ new_num, new_den, min_new, max_keep, n_order };
    r.cover = cover_host; r.cover_frame = frame_host; r.selected = selected_out; r.n_selected = n_selected;
    return score_call(r);
}
static int score_contours(ScoreRequest r, int32_t jump_mm, const uint8_t *edge_dist_dev, pr_pose_contour *contours_host, uint32_t *overlap_host)
{
    PR_ENTER();
    r.jump = jump_mm; r.edge_dist = edge_dist_dev; r.contours = contours_host; r.overlap = overlap_host;
    return score_call(r);
}
static int score_normals(ScoreRequest r, const float K[9], uint32_t step, int32_t jump_mm, float cos_min, pr_pose_normal *normals_host, uint32_t *overlap_host)
{
    PR_TRY(normal_params_ok(r.fn, step, jump_mm, cos_min));          // before any device use
    PR_ENTER();
    r.K = K; r.step = step; r.jump = jump_mm; r.cos_min = cos_min; r.normals = normals_host; r.overlap = overlap_host;
    return score_call(r);
}
static int compose_detections(ScoreRequest r, uint16_t *labels_dev_out, int32_t *depth_dev_out, pr_pose_visible *visible_host, pr_frame_explained *frame_host)
{
    PR_TRY(compose_args_ok(r.fn, r.P));          // before any device use
    PR_ENTER();
    if (r.P && labels_dev_out) note_write(labels_dev_out, sizeof(uint16_t) * (size_t)r.W * r.H);      // (the two images are the caller's device memory, written on this context's stream)
    if (r.P && depth_dev_out) note_write(depth_dev_out, sizeof(int32_t) * (size_t)r.W * r.H);
    r.labels_dev = labels_dev_out; r.depth_dev = depth_dev_out; r.visible = visible_host; r.frame = frame_host;
    return score_call(r);
}
// pr_scene_edge_distance_dev and pr_scene_edge_nearest_dev: one image of Out per frame pixel from the scene's depth edges; launch(bits, rows, stream): the kind's launcher
template <class Out, class Launch>
static int scene_edge_call(const char *fn, const void *scene_depth_dev, uint32_t width, uint32_t height, int32_t jump_mm, uint32_t radius, Out *out_dev, Launch &&launch)
{
    PR_ENTER();
    if (!scene_depth_dev || !out_dev || width == 0 || height == 0) { set_error("%s: bad arguments", fn); return PR_ERR_INVALID; }
    if (!frame_size_ok(width, height)) return PR_ERR_INVALID;
    if (jump_mm < 0 || radius > PR_CONTOUR_MAX_RADIUS) {
        set_error("%s: jump_mm must be >= 0 and radius <= PR_CONTOUR_MAX_RADIUS = %d (got %d, %u)", fn, PR_CONTOUR_MAX_RADIUS, (int)jump_mm, radius);
        return PR_ERR_INVALID;
    }
    const size_t img = (size_t)width * height;
    note_write(out_dev, sizeof(Out) * img);
    PR_TRY(g->edge_bits.ensure(sizeof(uint64_t) * (size_t)height * prk::overlap_words_per_row(width)));
    PR_TRY(g->edge_rows.ensure(img));
    HIP_TRY(launch(g->edge_bits.as<unsigned long long>(), g->edge_rows.p, g->stream));
    // the wait makes the call synchronous like every other entry point: the buffer is the caller's, who may hand it to another context (a private
    // thread context has a stream of its own) or read it with the runtime directly; nothing is copied to or from the host
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

// the four pyramid entry points (fn: whose messages; mesh: one mesh or a mesh table; robust: null, or the table of a _robust call)
static int refine_pyramid_impl(const char *fn, const MeshArg &mesh, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj,
                               const float K[9], int scene_kind, const void *scene, const pr_pyramid_level *levels, uint32_t n_levels, pr_roi roi, pr_result *results_host,
                               pr_result *level_results_host, uint32_t *level_sizes_host, const pr_robust *robust, uint32_t n_robust)
{
    PR_TRY(pyramid_levels_ok(fn, levels, n_levels, n_poses, results_host));      // before any device use
    PR_ENTER();
    PR_TRY(wait_pending_slots());                                   // (the scene caches are shared with the asynchronous slots)
    if (n_poses == 0) return PR_OK;
    if (!poses_host) { set_error("%s: bad arguments", fn); return PR_ERR_INVALID; }
    RefineJob job;                                                // (every level brings its own criteria)
    PR_TRY(make_job(fn, mesh.tris, mesh.n_tris, width, height, proj, K, scene_kind, scene, pr_criteria{ 0.0f, 0.0f, 0 }, roi, nullptr, job, robust, n_robust, n_levels));
    Batch b;
    PR_TRY(b.make(fn, mesh, poses_host, n_poses));
    job.mesh = b.src;
    const PyramidPlan py{ levels, n_levels, n_poses, level_results_host, level_sizes_host };
    return refine_ordered(job, b, &py, results_host, nullptr);
}
// what a _robust entry point refuses before it touches a device (so also on a machine without one), with nothing written
static int robust_call_ok(const char *fn, const pr_pyramid_level *levels, uint32_t n_levels, uint32_t n_poses, const pr_result *results_host,
                          const pr_robust *robust, uint32_t n_robust, bool pointers_ok)
{
    PR_TRY(pyramid_levels_ok(fn, levels, n_levels, n_poses, results_host));
    PR_TRY(robust_table_ok(fn, robust, n_robust, n_levels));
    if (n_poses && !pointers_ok) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    return PR_OK;
}

// pr_contour_information and its _multi form (a mesh table: a centre and a radius per mesh): the checks that need no request before any device is
// touched, the batch, the centres in the camera frame exactly as pr_pose_information forms them (camera_centers; here in the caller's order: score_run
// gathers them with the poses), then score_run on the batch
static int contour_information_impl(ScoreRequest r, int32_t jump_mm, const uint32_t *nearest_dev, const float K[9], const float *centers_model,
                                    const float *radii, pr_contour_fit *fit_host, pr_pose_info *info_host)
{
    const char *fn = r.fn;
    const MeshArg &mesh = r.mesh;
    PR_TRY(fit_intrinsics_ok(fn, K));
    if (!centers_model || !radii) { set_error("%s: bad arguments (a null centre or radius)", fn); return PR_ERR_INVALID; }
    PR_TRY(info_center_radius_ok(fn, centers_model, radii, mesh.multi ? mesh.n_meshes : 1u));
    if (r.P && (!r.poses || (mesh.multi && !mesh.mesh_index))) { set_error("%s: bad arguments", fn); return PR_ERR_INVALID; }
    Batch b;
    PR_TRY(b.make(fn, mesh, r.poses, r.P));
    std::vector<prk::FitMeta> meta(r.P);
    std::vector<float> centers(3 * (size_t)r.P), rad(r.P);
    camera_centers(r.poses, mesh.mesh_index, r.P, centers_model, radii, centers.data(), rad.data());
    for (uint32_t j = 0; j < r.P; ++j) { std::memcpy(meta[j].c, &centers[3 * (size_t)j], sizeof meta[j].c); meta[j].rho = rad[j]; }
    PR_TRY(info_center_radius_ok(fn, centers.data(), rad.data(), r.P));      // (a pose with a non-finite entry)
    r.jump = jump_mm; r.nearest = nearest_dev; r.K = K; r.fit_meta = meta.data(); r.fit = fit_host; r.fit_info = info_host;
    PR_TRY(score_request_ok(r));                                    // every remaining check before the device is touched
    if (r.P == 0) return PR_OK;
    PR_ENTER();
    return score_run(r, b);
}

// pr_pose_penetration and its _multi form: the records of a mesh table's batch into a temporary (nothing reaches pairs_host unless the call
// succeeded), rows and columns back to the caller's order as pr_score_overlap_multi's matrix; one mesh's straight into pairs_host
static int pose_penetration(const char *fn, const MeshArg &mesh, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj,
                            int32_t slack_mm, pr_pair_solid *pairs_host)
{
    PR_TRY(penetration_args_ok(fn, mesh.multi, mesh.tris, mesh.n_tris, poses_host, n_poses, width, height, proj, slack_mm, pairs_host));   // before any device use, like the mesh table's checks
    if (n_poses == 0) return PR_OK;
    Batch b;
    PR_TRY(b.make(fn, mesh, poses_host, n_poses));
    PR_ENTER();
    std::vector<pr_pair_solid> tmp;
    pr_pair_solid *rec = b.temp(tmp, (size_t)n_poses * n_poses, pairs_host);
    PR_TRY(solid_core(b.src, b.poses, n_poses, width, height, proj, slack_mm, rec));
    b.scatter_matrix(rec, pairs_host);
    return PR_OK;
}

// pr_pose_information and its _multi form (a mesh table: a centre and a radius per mesh): every check before any device is touched, the centres
// in the camera frame on the host (in the batch's order, like everything refine_core takes), refine_core with the information pass into
// temporaries, and the records back to the caller's order.
static int pose_information_impl(const char *fn, const MeshArg &mesh, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj,
                                 const float K[9], int scene_kind, const void *scene, pr_roi roi, const pr_robust *robust, const float *centers_model,
                                 const float *radii, pr_pose_info *info_host, pr_pose_eig *eig_host, uint32_t *cloud_sizes_host)
{
    if (robust) PR_TRY(robust_desc_ok(fn, robust));
    RefineJob job;
    PR_TRY(make_job(fn, mesh.tris, mesh.n_tris, width, height, proj, K, scene_kind, scene, pr_criteria{ 0.0f, 0.0f, 0 }, roi, nullptr, job));
    if (!centers_model || !radii || (n_poses && (!poses_host || !info_host))) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    Batch b;
    PR_TRY(b.make(fn, mesh, poses_host, n_poses));
    job.mesh = b.src;
    PR_TRY(info_center_radius_ok(fn, centers_model, radii, mesh.multi ? mesh.n_meshes : 1u));
    std::vector<uint32_t> mesh_of;
    std::vector<float> centers(3 * (size_t)n_poses), rad(n_poses);
    camera_centers(b.poses, mesh.multi ? b.gather(mesh.mesh_index, mesh_of) : nullptr, n_poses, centers_model, radii, centers.data(), rad.data());
    PR_TRY(info_center_radius_ok(fn, centers.data(), rad.data(), n_poses));      // (a pose with a non-finite entry)
    if (n_poses == 0) return PR_OK;
    PR_ENTER();
    PR_TRY(wait_pending_slots());                                   // (the scene caches are shared with the asynchronous slots)
    std::vector<pr_pose_info> info(n_poses);
    std::vector<pr_pose_eig> eig(eig_host ? n_poses : 0);
    std::vector<uint32_t> sizes(n_poses);
    const InfoPlan ip{ robust ? *robust : pr_robust{ PR_ROBUST_NONE, 0.0f, 0.0f, 0 }, centers.data(), rad.data(), info.data(), eig_host ? eig.data() : nullptr };
    PR_TRY(refine_core(job, b.poses, n_poses, nullptr, sizes.data(), nullptr, &ip));
    b.scatter(info.data(), info_host);
    b.scatter(eig.data(), eig_host);
    b.scatter(sizes.data(), cloud_sizes_host);
    return PR_OK;
}

extern "C" {

int pr_render(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, size_t n_poses, size_t width, size_t height,
              const pr_mat4 *proj, pr_roi roi, int32_t *depth_dev_out)
{
    return render_call("pr_render", MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, depth_dev_out, nullptr, false);
}

int pr_render_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host, size_t n_poses,
                    size_t width, size_t height, const pr_mat4 *proj, pr_roi roi, int32_t *depth_dev_out)
{
    return render_call("pr_render_multi", MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, roi, depth_dev_out, nullptr, false);
}

int pr_render_span(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, size_t n_poses, size_t width, size_t height,
                   const pr_mat4 *proj, pr_roi roi, int32_t *near_dev_out, int32_t *far_dev_out)
{
    return render_call("pr_render_span", MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, near_dev_out, far_dev_out, true);
}

int pr_render_to_host(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, size_t n_poses, size_t width, size_t height,
                      const pr_mat4 *proj, pr_roi roi, int32_t *depth_host_out)
{
    PR_ENTER();
    const auto [rw, rh] = image_extent(roi, width, height);
    PR_TRY(g->depth.ensure(sizeof(int32_t) * std::max<size_t>(1, n_poses * rw * rh)));
    PR_TRY(render_frames("pr_render", MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, g->depth.as<int32_t>(), nullptr, false, true));
    HIP_TRY(hipMemcpyAsync(depth_host_out, g->depth.p, sizeof(int32_t) * n_poses * rw * rh, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    drain_spans();
    return PR_OK;
}

int pr_depth2cloud_i32(const int32_t *depth_dev, uint32_t width, uint32_t height, const float K[9], uint32_t stride, uint32_t tl_x,
                       uint32_t tl_y, pr_vec3 **cloud_dev_out, uint32_t *n_points)
{
    PR_ENTER();
    return depth2cloud_impl<int32_t>(depth_dev, width, height, K, stride, tl_x, tl_y, cloud_dev_out, n_points);
}

int pr_depth2cloud_u16(const uint16_t *depth_dev, uint32_t width, uint32_t height, const float K[9], uint32_t stride, uint32_t tl_x,
                       uint32_t tl_y, pr_vec3 **cloud_dev_out, uint32_t *n_points)
{
    PR_ENTER();
    return depth2cloud_impl<uint16_t>(depth_dev, width, height, K, stride, tl_x, tl_y, cloud_dev_out, n_points);
}

int pr_refine_batch_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                          uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9], int scene_kind,
                          const void *scene, pr_criteria crit, pr_roi roi, pr_result *results_host, uint32_t *cloud_sizes_host)
{
    PR_ENTER();
    if (n_poses == 0) return PR_OK;
    if (!results_host || !poses_host) { set_error("pr_refine_batch_multi: bad arguments"); return PR_ERR_INVALID; }
    RefineJob job;
    PR_TRY(make_job("pr_refine_batch_multi", nullptr, 0, width, height, proj, K, scene_kind, scene, crit, roi, nullptr, job));
    Batch b;
    PR_TRY(b.make("pr_refine_batch_multi", MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses));
    job.mesh = b.src;
    return refine_ordered(job, b, nullptr, results_host, cloud_sizes_host);
}

int pr_refine_pyramid_robust(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                             const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, const pr_pyramid_level *levels, uint32_t n_levels,
                             pr_roi roi, pr_result *results_host, pr_result *level_results_host, uint32_t *level_sizes_host,
                             const pr_robust *robust, uint32_t n_robust)
{
    const char *fn = "pr_refine_pyramid_robust";
    PR_TRY(robust_call_ok(fn, levels, n_levels, n_poses, results_host, robust, n_robust, poses_host && proj && K && scene && (tris_dev || n_tris == 0)));
    return refine_pyramid_impl(fn, MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, K, scene_kind, scene, levels, n_levels, roi, results_host, level_results_host,
                               level_sizes_host, robust, n_robust);
}

int pr_refine_pyramid_robust_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                                   uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9], int scene_kind,
                                   const void *scene, const pr_pyramid_level *levels, uint32_t n_levels, pr_roi roi, pr_result *results_host,
                                   pr_result *level_results_host, uint32_t *level_sizes_host, const pr_robust *robust, uint32_t n_robust)
{
    const char *fn = "pr_refine_pyramid_robust_multi";
    PR_TRY(robust_call_ok(fn, levels, n_levels, n_poses, results_host, robust, n_robust, poses_host && proj && K && scene && meshes && mesh_index_host));
    return refine_pyramid_impl(fn, MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, K, scene_kind, scene, levels, n_levels, roi, results_host,
                               level_results_host, level_sizes_host, robust, n_robust);
}

int pr_refine_pyramid(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                      const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, const pr_pyramid_level *levels, uint32_t n_levels,
                      pr_roi roi, pr_result *results_host, pr_result *level_results_host, uint32_t *level_sizes_host)
{
    return refine_pyramid_impl("pr_refine_pyramid", MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, K, scene_kind, scene, levels, n_levels, roi, results_host,
                               level_results_host, level_sizes_host, nullptr, 0);
}

int pr_refine_pyramid_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                            uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9], int scene_kind,
                            const void *scene, const pr_pyramid_level *levels, uint32_t n_levels, pr_roi roi, pr_result *results_host,
                            pr_result *level_results_host, uint32_t *level_sizes_host)
{
    return refine_pyramid_impl("pr_refine_pyramid_multi", MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, K, scene_kind, scene, levels, n_levels, roi,
                               results_host, level_results_host, level_sizes_host, nullptr, 0);
}

int pr_score_poses(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                   const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, pr_pose_score *scores_host)
{
    return score_poses(score_request("pr_score_poses", kScorePoses, MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, scene_depth_dev, depth_is_i32, tau_mm, scores_host));
}

int pr_score_poses_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                         uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                         int depth_is_i32, int32_t tau_mm, pr_pose_score *scores_host)
{
    return score_poses(score_request("pr_score_poses_multi", kScorePoses, MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, roi, scene_depth_dev,
                       depth_is_i32, tau_mm, scores_host));
}

int pr_score_overlap(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                     const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, pr_pose_score *scores_host,
                     uint32_t *overlap_host)
{
    return score_overlap(score_request("pr_score_overlap", kScoreOverlap, MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, scene_depth_dev, depth_is_i32, tau_mm,
                         scores_host), overlap_host);
}

int pr_score_overlap_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                           uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                           int depth_is_i32, int32_t tau_mm, pr_pose_score *scores_host, uint32_t *overlap_host)
{
    return score_overlap(score_request("pr_score_overlap_multi", kScoreOverlap, MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, roi, scene_depth_dev,
                         depth_is_i32, tau_mm, scores_host), overlap_host);
}

int pr_score_cover(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                   const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, const uint32_t *order, uint32_t n_order,
                   uint32_t new_num, uint32_t new_den, uint32_t min_new, uint32_t max_keep, pr_pose_score *scores_host, pr_pose_cover *cover_host,
                   pr_cover_frame *frame_host, uint32_t *selected_out, uint32_t *n_selected)
{
    return score_cover(score_request("pr_score_cover", kScoreCover, MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, scene_depth_dev, depth_is_i32, tau_mm, scores_host),
                       order, n_order, new_num, new_den, min_new, max_keep, cover_host, frame_host, selected_out, n_selected);
}

int pr_score_cover_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host, uint32_t n_poses,
                         uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm,
                         const uint32_t *order, uint32_t n_order, uint32_t new_num, uint32_t new_den, uint32_t min_new, uint32_t max_keep,
                         pr_pose_score *scores_host, pr_pose_cover *cover_host, pr_cover_frame *frame_host, uint32_t *selected_out, uint32_t *n_selected)
{
    return score_cover(score_request("pr_score_cover_multi", kScoreCover, MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, roi, scene_depth_dev,
                       depth_is_i32, tau_mm, scores_host), order, n_order, new_num, new_den, min_new, max_keep, cover_host, frame_host, selected_out, n_selected);
}

int pr_scene_edge_distance_dev(const void *scene_depth_dev, int depth_is_i32, uint32_t width, uint32_t height, int32_t jump_mm, uint32_t radius,
                               uint8_t *dist_dev_out)
{
    return scene_edge_call("pr_scene_edge_distance_dev", scene_depth_dev, width, height, jump_mm, radius, dist_dev_out, [&](unsigned long long *bits, void *rows, hipStream_t st) {
        return prk::launch_scene_edge_distance(scene_depth_dev, depth_is_i32 != 0, width, height, jump_mm, radius, bits, static_cast<uint8_t *>(rows), dist_dev_out, st);
    });
}

int pr_scene_edge_nearest_dev(const void *scene_depth_dev, int depth_is_i32, uint32_t width, uint32_t height, int32_t jump_mm, uint32_t radius,
                              uint32_t *nearest_dev_out)
{
    return scene_edge_call("pr_scene_edge_nearest_dev", scene_depth_dev, width, height, jump_mm, radius, nearest_dev_out, [&](unsigned long long *bits, void *rows, hipStream_t st) {
        return prk::launch_scene_edge_nearest(scene_depth_dev, depth_is_i32 != 0, width, height, jump_mm, radius, bits, static_cast<int8_t *>(rows), nearest_dev_out, st);
    });
}

int pr_score_contours(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                      const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, int32_t jump_mm,
                      const uint8_t *edge_dist_dev, pr_pose_score *scores_host, pr_pose_contour *contours_host, uint32_t *overlap_host)
{
    return score_contours(score_request("pr_score_contours", kScoreContours, MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, scene_depth_dev, depth_is_i32, tau_mm,
                          scores_host), jump_mm, edge_dist_dev, contours_host, overlap_host);
}

int pr_score_contours_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                            uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                            int depth_is_i32, int32_t tau_mm, int32_t jump_mm, const uint8_t *edge_dist_dev, pr_pose_score *scores_host,
                            pr_pose_contour *contours_host, uint32_t *overlap_host)
{
    return score_contours(score_request("pr_score_contours_multi", kScoreContours, MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, roi, scene_depth_dev,
                          depth_is_i32, tau_mm, scores_host), jump_mm, edge_dist_dev, contours_host, overlap_host);
}

int pr_contour_information(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                           const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, int32_t jump_mm,
                           const uint32_t *nearest_dev, const float K[9], const float *center_model, float radius, pr_pose_score *scores_host_or_null,
                           pr_contour_fit *fit_host, pr_pose_info *info_host)
{
    return contour_information_impl(score_request("pr_contour_information", kScoreContourFit, MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, scene_depth_dev,
                                    depth_is_i32, tau_mm, scores_host_or_null), jump_mm, nearest_dev, K, center_model, &radius, fit_host, info_host);
}

int pr_contour_information_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host, uint32_t n_poses,
                                 uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm,
                                 int32_t jump_mm, const uint32_t *nearest_dev, const float K[9], const float *centers_model, const float *radii,
                                 pr_pose_score *scores_host_or_null, pr_contour_fit *fit_host, pr_pose_info *info_host)
{
    return contour_information_impl(score_request("pr_contour_information_multi", kScoreContourFit, MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, roi,
                                    scene_depth_dev, depth_is_i32, tau_mm, scores_host_or_null), jump_mm, nearest_dev, K, centers_model, radii, fit_host, info_host);
}

int pr_score_normals(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                     const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, const float K[9], uint32_t step,
                     int32_t jump_mm, float cos_min, pr_pose_score *scores_host, pr_pose_normal *normals_host, uint32_t *overlap_host)
{
    return score_normals(score_request("pr_score_normals", kScoreNormals, MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, scene_depth_dev, depth_is_i32, tau_mm,
                         scores_host), K, step, jump_mm, cos_min, normals_host, overlap_host);
}

int pr_score_normals_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                           uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                           int depth_is_i32, int32_t tau_mm, const float K[9], uint32_t step, int32_t jump_mm, float cos_min,
                           pr_pose_score *scores_host, pr_pose_normal *normals_host, uint32_t *overlap_host)
{
    return score_normals(score_request("pr_score_normals_multi", kScoreNormals, MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, roi, scene_depth_dev,
                         depth_is_i32, tau_mm, scores_host), K, step, jump_mm, cos_min, normals_host, overlap_host);
}

int pr_compose_detections(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                          const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, uint16_t *labels_dev_out,
                          int32_t *depth_dev_out, pr_pose_score *scores_host, pr_pose_visible *visible_host, pr_frame_explained *frame_host)
{
    return compose_detections(score_request("pr_compose_detections", kScoreCompose, MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, roi, scene_depth_dev, depth_is_i32,
                              tau_mm, scores_host), labels_dev_out, depth_dev_out, visible_host, frame_host);
}

int pr_compose_detections_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                                uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                                int depth_is_i32, int32_t tau_mm, uint16_t *labels_dev_out, int32_t *depth_dev_out, pr_pose_score *scores_host,
                                pr_pose_visible *visible_host, pr_frame_explained *frame_host)
{
    return compose_detections(score_request("pr_compose_detections_multi", kScoreCompose, MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, roi,
                              scene_depth_dev, depth_is_i32, tau_mm, scores_host), labels_dev_out, depth_dev_out, visible_host, frame_host);
}

int pr_pose_vsd(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *est_host, uint32_t n_est, const pr_mat4 *gt_host, uint32_t n_gt, uint32_t width,
                uint32_t height, const pr_mat4 *proj, const void *scene_depth_dev, int depth_is_i32, const float K[9], float delta_mm, const float *taus_mm,
                uint32_t n_taus, pr_vsd_counts *out_host)
{
    PR_TRY(vsd_args_ok("pr_pose_vsd", false, tris_dev, n_tris, est_host, n_est, gt_host, n_gt, width, height, proj, scene_depth_dev, K, delta_mm, taus_mm, n_taus,
                       out_host));                                   // before any device use
    if (n_est == 0) return PR_OK;
    PR_ENTER();
    const MeshSource src{ tris_dev, n_tris, nullptr };
    const prk::VsdParams pm = vsd_params(K, delta_mm, taus_mm, n_taus);
    if (n_gt == 1 && n_est != 1) return vsd_core(src, est_host, gt_host, n_est, width, height, proj, scene_depth_dev, depth_is_i32 != 0, pm, out_host);
    const std::vector<pr_mat4> pairs = interleaved_pairs(est_host, gt_host, n_est);
    return vsd_core(src, pairs.data(), nullptr, n_est, width, height, proj, scene_depth_dev, depth_is_i32 != 0, pm, out_host);
}

// A mixed batch: both poses of pair i carry mesh_index_host[i], so the stable grouping keeps them adjacent -- the batch of 2 n_est renders is interleaved
// pairs again, pair j of it the caller's pair caller(2 j) / 2.  Records into a temporary: nothing reaches out_host unless the call succeeded.
int pr_pose_vsd_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *est_host, uint32_t n_est,
                      const pr_mat4 *gt_host, uint32_t n_gt, uint32_t width, uint32_t height, const pr_mat4 *proj, const void *scene_depth_dev,
                      int depth_is_i32, const float K[9], float delta_mm, const float *taus_mm, uint32_t n_taus, pr_vsd_counts *out_host)
{
    PR_TRY(vsd_args_ok("pr_pose_vsd_multi", true, nullptr, 0, est_host, n_est, gt_host, n_gt, width, height, proj, scene_depth_dev, K, delta_mm, taus_mm, n_taus,
                       out_host));                                   // before any device use, like the mesh table's checks below
    if (n_est == 0) return PR_OK;
    std::vector<uint32_t> index2(2 * (size_t)n_est);
    for (uint32_t i = 0; mesh_index_host && i < n_est; ++i) {
        if (n_meshes && mesh_index_host[i] >= n_meshes) { set_error("pr_pose_vsd_multi: mesh_index[%u] = %u, but there are %u meshes", i, mesh_index_host[i], n_meshes); return PR_ERR_INVALID; }
        index2[2 * (size_t)i] = index2[2 * (size_t)i + 1] = mesh_index_host[i];
    }
    const std::vector<pr_mat4> pairs = interleaved_pairs(est_host, gt_host, n_est);
    Batch b;
    PR_TRY(b.make("pr_pose_vsd_multi", MeshArg::table(meshes, n_meshes, mesh_index_host ? index2.data() : nullptr), pairs.data(), 2 * (size_t)n_est));
    PR_ENTER();
    std::vector<pr_vsd_counts> rec(n_est);
    PR_TRY(vsd_core(b.src, b.poses, nullptr, n_est, width, height, proj, scene_depth_dev, depth_is_i32 != 0, vsd_params(K, delta_mm, taus_mm, n_taus), rec.data()));
    for (uint32_t j = 0; j < n_est; ++j) out_host[b.caller(2 * (size_t)j) / 2] = rec[j];
    return PR_OK;
}

int pr_pose_penetration(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                        const pr_mat4 *proj, int32_t slack_mm, pr_pair_solid *pairs_host)
{
    return pose_penetration("pr_pose_penetration", MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, slack_mm, pairs_host);
}

int pr_pose_penetration_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host, uint32_t n_poses,
                              uint32_t width, uint32_t height, const pr_mat4 *proj, int32_t slack_mm, pr_pair_solid *pairs_host)
{
    return pose_penetration("pr_pose_penetration_multi", MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, slack_mm, pairs_host);
}

int pr_pose_information(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                        const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, pr_roi roi, const pr_robust *robust_or_null,
                        const float *center_model, float radius, pr_pose_info *info_host, pr_pose_eig *eig_host_or_null, uint32_t *cloud_sizes_host_or_null)
{
    return pose_information_impl("pr_pose_information", MeshArg::one(tris_dev, n_tris), poses_host, n_poses, width, height, proj, K, scene_kind, scene, roi, robust_or_null, center_model, &radius,
                                 info_host, eig_host_or_null, cloud_sizes_host_or_null);
}

int pr_pose_information_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host, uint32_t n_poses,
                              uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, pr_roi roi,
                              const pr_robust *robust_or_null, const float *centers_model, const float *radii, pr_pose_info *info_host,
                              pr_pose_eig *eig_host_or_null, uint32_t *cloud_sizes_host_or_null)
{
    return pose_information_impl("pr_pose_information_multi", MeshArg::table(meshes, n_meshes, mesh_index_host), poses_host, n_poses, width, height, proj, K, scene_kind, scene, roi, robust_or_null,
                                 centers_model, radii, info_host, eig_host_or_null, cloud_sizes_host_or_null);
}

int pr_refine_batch_roi(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                        const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, pr_criteria crit, pr_roi roi,
                        pr_result *results_host, uint32_t *cloud_sizes_host)
{
    TraceScope traced;                                            // (pr_debug_trace_sums: this call and no other)
    PR_ENTER();
    if (!results_host) { set_error("pr_refine_batch: results_host is null"); return PR_ERR_INVALID; }
    if (n_poses == 0) return PR_OK;
    PR_TRY(sums_trace_admits("pr_refine_batch", n_poses, crit));    // (before the render is launched; icp_drive asks again)
    if (tl_sums_trace.active.rows && n_poses > depth_chunk((size_t)width * height, n_poses)) {   // (rows are indexed within one icp_drive run)
        set_error("pr_refine_batch: pr_debug_trace_sums records batches that render as one chunk; %u hypotheses at this frame size do not", n_poses);
        return PR_ERR_INVALID;
    }
    const int slot = free_slot();
    if (slot < 0) { set_error("pr_refine_batch: both asynchronous slots hold unfinished batches (pr_refine_wait one of them first)"); return PR_ERR_INVALID; }
    RefineJob job;
    PR_TRY(make_job("pr_refine_batch", tris_dev, n_tris, width, height, proj, K, scene_kind, scene, crit, roi, nullptr, job));
    PR_TRY(refine_submit(g->slots[slot], job, poses_host, n_poses, results_host, cloud_sizes_host));
    return refine_wait(slot);
}

int pr_refine_batch(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                    const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, pr_criteria crit,
                    pr_result *results_host, uint32_t *cloud_sizes_host)
{
    return pr_refine_batch_roi(tris_dev, n_tris, poses_host, n_poses, width, height, proj, K, scene_kind, scene, crit, pr_roi{ 0, 0, 0, 0 }, results_host, cloud_sizes_host);
}

int pr_refine_batch_dev(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                        const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, pr_criteria crit,
                        pr_result *results_dev, uint32_t *cloud_sizes_host)
{
    PR_ENTER();
    if (!results_dev) { set_error("pr_refine_batch_dev: results_dev is null"); return PR_ERR_INVALID; }
    if (n_poses == 0) return PR_OK;
    const int slot = free_slot();
    if (slot < 0) { set_error("pr_refine_batch_dev: both asynchronous slots hold unfinished batches (pr_refine_wait one of them first)"); return PR_ERR_INVALID; }
    RefineJob job;
    PR_TRY(make_job("pr_refine_batch_dev", tris_dev, n_tris, width, height, proj, K, scene_kind, scene, crit, pr_roi{ 0, 0, 0, 0 }, results_dev, job));
    PR_TRY(refine_submit(g->slots[slot], job, poses_host, n_poses, nullptr, cloud_sizes_host));
    return refine_wait(slot);
}

int pr_refine_submit_roi(int slot, const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                         const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, pr_criteria crit, pr_roi roi,
                         pr_result *results_host, pr_result *results_dev, uint32_t *cloud_sizes_host)
{
    trace_mark("pr_refine_submit: enter");
    int rc;
    {
        PR_ENTER();
        RefineJob job;
        rc = slot_idle(slot);
        if (rc == PR_OK) rc = make_job("pr_refine_submit", tris_dev, n_tris, width, height, proj, K, scene_kind, scene, crit, roi, results_dev, job);
        if (rc == PR_OK) rc = refine_submit(g->slots[slot], job, poses_host, n_poses, results_host, cloud_sizes_host);
    }
    trace_mark("pr_refine_submit: exit");
    return rc;
}

int pr_refine_submit(int slot, const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                     const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, pr_criteria crit,
                     pr_result *results_host, pr_result *results_dev, uint32_t *cloud_sizes_host)
{
    return pr_refine_submit_roi(slot, tris_dev, n_tris, poses_host, n_poses, width, height, proj, K, scene_kind, scene, crit, pr_roi{ 0, 0, 0, 0 }, results_host, results_dev, cloud_sizes_host);
}

int pr_refine_wait(int slot)
{
    trace_mark("pr_refine_wait: enter");
    int rc;
    { PR_ENTER(); rc = refine_wait(slot); }
    trace_mark("pr_refine_wait: exit");
    return rc;
}

#if PR_LOOP_CU_PROBE
// measuring builds only (pr_tuning.h): four floats per hypothesis that the resident loop of the slot's last sub-batch left in its partial buffer
int pr_loop_probe_read(int slot, float *out, uint32_t n_poses)
{
    PR_ENTER();
    if (slot < 0 || slot >= kSlots || !out) return PR_ERR_INVALID;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, g->slots[slot].partial.as<float>(), sizeof(float) * 4 * n_poses, hipMemcpyDeviceToHost));
    return PR_OK;
}
#endif

}  // extern "C"
