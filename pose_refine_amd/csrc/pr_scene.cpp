// pr_scene.cpp -- scene caches (packed projective record, kd-tree traversal records, pixel grid) and device-side scene preparation
#include "pr_runtime.h"
#include "frame_stage.h"

namespace prr {

// Packed copy of a projective scene in `pc`: reused while the caller's arrays are unchanged as far as the library can tell
// (option scene_cache, WriteLog above), rebuilt otherwise.  A rebuild also learns (one 4-byte read-back) whether the pcd array
// is exactly what dep2pcd produces -- only then may the packed form stand in for it.
// Synchronous callers (pr_icp_*, the synchronous fused path -- everything the C++ adapters of the reference's API reach) check a cache hit on the
// spot, and since round 6 against a fingerprint of EVERY word of the source arrays (`fp->full`, taken when the cache was built; `fp->call` is this
// call's): the reference reads the caller's arrays at every call (depth_scene.h:29-48), so an in-place edit through a pointer the adapters handed
// out must be seen even when nobody announced it.  ~20 us per call; the asynchronous path compares the 4096-word SAMPLE
// (`fp->sample`) inside its raster launch, which raises the batch's flag (BatchCheck), and documents pr_invalidate for edits the sample cannot see.
static int fingerprint_differs(const prk::SceneSources &src, prk::FpWords *fp, hipStream_t st, bool &differs)
{
    HIP_TRY(prk::launch_scene_fingerprint_full(src, &fp->call, st));
    // both words come back through a kernel's stores into pinned memory (no copy command on the per-batch path: see drive_host's result block)
    uint32_t v[2] = { 0u, 1u };
    PR_TRY(read_back_words(&fp->full, v, 2, st));                 // full, call
    differs = v[0] != v[1];
    return PR_OK;
}
static int ensure_packed(PackedCache &pc, const pr_scene_proj &s, uint32_t tl_x, uint32_t tl_y, hipStream_t st, bool verify_now)
{
    const size_t n = (size_t)s.width * s.height;
    const float k[4] = { s.K[0], s.K[4], s.K[2], s.K[5] };
    const prk::SceneSources src = prk::scene_sources(s);
    const PackedLayout lay = packed_layout(s.width, s.height);
    const bool same = pc.valid && pc.pcd == s.pcd && pc.normal == s.normal && pc.w == s.width && pc.h == s.height &&
                      std::memcmp(pc.k, k, sizeof k) == 0 && pc.tl[0] == tl_x && pc.tl[1] == tl_y;
    if (same && opt.scene_cache && !g_writes.written_since(pc.gen, s.pcd, src.bytes[0]) && !g_writes.written_since(pc.gen, s.normal, src.bytes[1])) {
        bool stale = false;
        if (verify_now) PR_TRY(fingerprint_differs(src, &pc.at<ProjTail>(lay.tail)->fp, st, stale));
        if (!stale) { pc.gen = g_writes.now(); return PR_OK; }
    }
    pc.valid = false;
    const uint64_t gen = g_writes.now();
    PR_TRY(pc.rec.ensure(lay.bytes));
    ProjTail *tail = pc.at<ProjTail>(lay.tail);
    HIP_TRY(prk::launch_pack_proj_scene(s.pcd, s.normal, pc.rec.as<float4>(), n, pc.at<float>(lay.colf), pc.at<float>(lay.rowf), (uint32_t)s.width, (uint32_t)s.height,
                                        k[0], k[1], k[2], k[3], tl_x, tl_y, &tail->exact, st));
    HIP_TRY(prk::launch_scene_fingerprint(src, &tail->fp.sample, st));
    HIP_TRY(prk::launch_scene_fingerprint_full(src, &tail->fp.full, st));
    uint32_t exact = 0;
    PR_TRY(read_back_words(&tail->exact, &exact, 1, st));
    pc.pcd = s.pcd; pc.normal = s.normal; pc.w = s.width; pc.h = s.height; std::memcpy(pc.k, k, sizeof k); pc.tl[0] = tl_x; pc.tl[1] = tl_y;
    pc.gen = gen; pc.exact = exact != 0; pc.valid = true;
    return PR_OK;
}

// ---- make_scene by scene kind ---------------------------------------------------------------------------------------------------------
// projective, whole frame or crop: the caller's arrays, and (want_packed) their packed copy in `pc`, built or verified on `st`
static int scene_proj(int kind, const void *scene, bool want_packed, SceneSel &out, PackedCache &pc, hipStream_t st, bool verify_now)
{
    const pr_scene_proj *s = static_cast<const pr_scene_proj *>(scene);       // pr_scene_proj_crop starts with the plain view
    if (!s || !s->pcd || !s->normal || s->width == 0 || s->height == 0) { set_error("invalid pr_scene_proj"); return PR_ERR_INVALID; }
    if (s->width > 0x7fffffffull || s->height > 0x7fffffffull) { set_error("pr_scene_proj: frame too large"); return PR_ERR_INVALID; }
    uint32_t tl_x = 0, tl_y = 0;
    if (kind == PR_SCENE_PROJ_CROP) { const pr_scene_proj_crop *c = static_cast<const pr_scene_proj_crop *>(scene); tl_x = c->tl_x; tl_y = c->tl_y; }
    out.kind = PR_SCENE_PROJ;
    out.aos = prk::SceneProjAoS{ (uint32_t)s->width, (uint32_t)s->height, s->max_dist_diff, s->K[0], s->K[4], s->K[2], s->K[5],
                                 (float)tl_x, (float)tl_y, s->pcd, s->normal };
    out.packed = false;
    if (!want_packed) return PR_OK;
    PR_TRY(ensure_packed(pc, *s, tl_x, tl_y, st, verify_now));
    if (!pc.exact) return PR_OK;                                // the caller's pcd is not dep2pcd's -- use the arrays as they are
    const PackedLayout lay = packed_layout(s->width, s->height);
    out.packed = true;
    out.pk = prk::SceneProjPacked{ (uint32_t)s->width, (uint32_t)s->height, s->max_dist_diff, s->K[0], s->K[4], s->K[2], s->K[5],
                                   (float)tl_x, (float)tl_y, pc.rec.as<float4>(), pc.at<float>(lay.colf), pc.at<float>(lay.rowf) };
    return PR_OK;
}

// kd-tree scenes.  Everything below runs on g->stream, whatever stream the caller named.
static bool set_in_flight(int set) { for (Slot &o : g->slots) if (o.pending && !o.delivered && o.nn_set == set) return true; return false; }
static void drain_readers(int set) { for (Slot &o : g->slots) if (o.pending && !o.delivered && o.nn_set == set) slot_drain(o); }
// the records of `s` into set `nc`: the traversal arrays (which clears the control words), then the fingerprints, then the wide records
static int derive_nn_set(NNDerived &nc, const pr_scene_nn &s)
{
    nc.valid = false; nc.grid_valid = false;
    const uint64_t gen = g_writes.now();
    const float margin = s.max_dist_diff * 1.01f;
    PR_TRY(nc.topo.ensure((size_t)s.n_nodes * sizeof(int4)));
    PR_TRY(nc.bmin.ensure((size_t)s.n_nodes * sizeof(float4)));
    PR_TRY(nc.bmax.ensure((size_t)s.n_nodes * sizeof(float4)));
    PR_TRY(nc.pts.ensure(((size_t)s.n_points + 16u) * sizeof(float4)));   // + 16: a leaf task of the walk reads its ten slots whatever the leaf holds (nn_tree_wide_kernel)
    PR_TRY(nc.nnrec.ensure((size_t)s.n_nodes * 4 * sizeof(float4)));
    PR_TRY(nc.nndepth.ensure(sizeof(prk::NNInfo)));
    PR_TRY(nc.nnrec32.ensure((size_t)s.n_nodes * 2 * sizeof(uint4)));
    PR_TRY(nc.nndesc.ensure((size_t)s.n_nodes * sizeof(uint2)));
    // wide records: one 128-byte line per wide node
    PR_TRY(nc.nnwide.ensure(prk::nn_wide_capacity(s.n_nodes) * 128));
    PR_TRY(nc.nnwq.ensure(prk::nn_wide_scratch_words(s.n_nodes) * sizeof(uint32_t)));
    prk::NNInfo *info = nc.nndepth.as<prk::NNInfo>();
    const prk::SceneSources src = prk::scene_sources(s);
    HIP_TRY(prk::launch_build_nn_accel(s.nodes, s.n_nodes, s.pcd, s.n_points, nc.topo.as<int4>(), nc.bmin.as<float4>(), nc.bmax.as<float4>(), nc.pts.as<float4>(),
                                       nc.nnrec.as<float4>(), nc.nnrec32.as<uint4>(), nc.nndesc.as<uint2>(), info, g->stream, margin));
    HIP_TRY(prk::launch_scene_fingerprint(src, &info->fp.sample, g->stream));
    HIP_TRY(prk::launch_scene_fingerprint_full(src, &info->fp.full, g->stream));
    // the wide records, eight levels per synchronisation (8^8 wide nodes: deeper only for a lopsided tree)
    for (uint32_t level = 0; ; level += 8) {
        HIP_TRY(prk::launch_nn_wide_levels(nc.topo.as<int4>(), nc.bmin.as<float4>(), nc.bmax.as<float4>(), s.n_nodes, s.n_points, nc.nnwide.as<uint4>(),
                                           nc.nnwq.as<uint32_t>(), info, level, 8, g->stream));
        PR_TRY(read_back_words(info, &nc.info, (uint32_t)(sizeof nc.info / sizeof(uint32_t)), g->stream));
        if (nc.info.wide_state != prk::kWideMoreLevels) break;
        if (level + 8 >= 64) { nc.info.wide_state = prk::kWideNone; break; }    // (as before: more than 64 wide levels -> the binary records)
    }
    nc.pcd = s.pcd; nc.normal = s.normal; nc.nodes = s.nodes; nc.n_points = s.n_points; nc.n_nodes = s.n_nodes; nc.gen = gen; nc.valid = true;
    nc.frame_margin = margin;
    return PR_OK;
}
// Pixel grid of the scene points under the hypotheses' camera (fused paths), or under the camera the scene says it was made with: built into set
// `set` unless it holds that camera's.  Usable when every scene point owns a cell -- a Scene_nn made from a depth image with these
// intrinsics -- else the tree alone.
static int ensure_nn_grid(int set, const pr_scene_nn &s, const Camera &cam)
{
    NNDerived &nc = g->nn_sets[set];
    const float gk[4] = { cam.fx, cam.fy, cam.cx, cam.cy };
    if (nc.grid_valid && nc.gw == cam.w && nc.gh == cam.h && std::memcmp(nc.gk, gk, sizeof gk) == 0) return PR_OK;
    drain_readers(set);
    const size_t cells = (size_t)cam.w * cam.h;
    PR_TRY(nc.nn_cells.ensure(cells * sizeof(int32_t) + 16));
    PR_TRY(nc.nn_grid.ensure(prk::nn_grid_cells(cam.w, cam.h) * sizeof(float4)));
    uint32_t *flag = reinterpret_cast<uint32_t *>(nc.nn_cells.as<int32_t>() + cells);
    HIP_TRY(prk::launch_build_nn_grid(s.pcd, s.n_points, cam.w, cam.h, gk[0], gk[1], gk[2], gk[3], nc.nn_cells.as<int32_t>(), nc.nn_grid.as<float4>(), flag, g->stream));
    uint32_t usable = 0;
    PR_TRY(read_back_words(flag, &usable, 1, g->stream));
    nc.grid_valid = true; nc.grid_usable = usable != 0; nc.gw = cam.w; nc.gh = cam.h; std::memcpy(nc.gk, gk, sizeof gk);
    return PR_OK;
}
// what the searches take (SceneSel::nn): the set's arrays as the route uses them; the grid's fields stay empty
static prk::SceneNNDev nn_dev(const NNDerived &nc, const pr_scene_nn &s, const NNRoute &route)
{
    prk::SceneNNDev d{};
    d.max_dist_diff = s.max_dist_diff;
    d.topo = nc.topo.as<int4>(); d.bmin = nc.bmin.as<float4>(); d.bmax = nc.bmax.as<float4>(); d.pts = nc.pts.as<float4>();
    d.pcd = s.pcd; d.normal = s.normal; d.n_nodes = s.n_nodes;
    d.lds_nodes = route.lds_nodes; d.topo_nodes = route.topo_nodes; d.rec = nc.nnrec.as<float4>(); d.stack_depth = route.stack_depth; d.desc = nc.nndesc.as<uint2>();
    if (route.compact) {
        d.rec32 = nc.nnrec32.as<uint4>();
        std::memcpy(d.qmin, nc.info.qmin, sizeof d.qmin); std::memcpy(d.qscale, nc.info.qscale, sizeof d.qscale);
    }
    if (route.wide) {
        d.wide = nc.nnwide.as<uint4>(); d.n_wide = nc.info.n_wide;
        std::memcpy(d.wmin, nc.info.wmin, sizeof d.wmin); std::memcpy(&d.wscale, &nc.info.wscale, sizeof d.wscale);
    }
    return d;
}
static int scene_nn(const void *scene, SceneSel &out, const Camera *cam, bool verify_now)
{
    const pr_scene_nn *s = static_cast<const pr_scene_nn *>(scene);
    if (!s || !s->pcd || !s->normal || !s->nodes || s->n_nodes == 0 || s->n_points == 0) { set_error("invalid pr_scene_nn"); return PR_ERR_INVALID; }
    const prk::SceneSources src = prk::scene_sources(*s);
    // which of the sets of derived records (pick_nn_set has the rules)
    NNSetFacts facts[kNNSets];
    for (int i = 0; i < kNNSets; ++i) {
        const NNDerived &d = g->nn_sets[i];
        const bool same_arrays = d.pcd == s->pcd && d.nodes == s->nodes;
        const bool matches = d.valid && same_arrays && d.normal == s->normal && d.n_points == s->n_points && d.n_nodes == s->n_nodes &&
                             s->max_dist_diff * 1.01f <= d.frame_margin;      // (a smaller radius keeps its pruning inside the larger frame; a larger one would lose it outside the old)
        const bool hit = matches && opt.scene_cache && !g_writes.written_since(d.gen, s->pcd, src.bytes[0]) && !g_writes.written_since(d.gen, s->nodes, src.bytes[1]);
        facts[i] = NNSetFacts{ d.valid, hit, same_arrays, set_in_flight(i), d.used };
    }
    const NNSetPick pick = pick_nn_set(facts, kNNSets);
    NNDerived &nc = g->nn_sets[pick.set];
    bool hit = pick.hit;
    if (hit && verify_now) {                                    // (a hit that turns out stale is rebuilt in the same set)
        bool stale = false;
        PR_TRY(fingerprint_differs(src, &nc.nndepth.as<prk::NNInfo>()->fp, g->stream, stale));
        hit = !stale;
    }
    nc.used = ++g->nn_clock;
    out.nn_set = pick.set;
    if (hit) nc.gen = g_writes.now();                           // (the normals are read through the caller's pointer, never copied)
    else {
        drain_readers(pick.set);                                // (a batch in flight that reads this very set: it finishes first)
        PR_TRY(derive_nn_set(nc, *s));
    }
    if (nc.info.depth >= 0x7fffffffu) { nc.valid = false; set_error("pr_scene_nn: the nodes do not form a consistent tree (child / parent links disagree or point outside the array)"); return PR_ERR_INVALID; }
    const NNRoute route = nn_route(nc.info, s->n_nodes, opt.nn_lds_nodes, opt.nn_lds_records, opt.nn_stack, opt.nn_compact, opt.nn_wide);
    out.nn = nn_dev(nc, *s, route);
    // a bare ICP call has no camera of its own: the scene's hint, if it carries one (pose_refine.h)
    Camera hinted;
    if (!cam && s->cam_magic == PR_SCENE_NN_CAM_MAGIC && s->cam_w && s->cam_h && s->cam_fx > 0.0f && s->cam_fy > 0.0f) { hinted = Camera{ s->cam_w, s->cam_h, s->cam_fx, s->cam_fy, s->cam_cx, s->cam_cy }; cam = &hinted; }
    if (!(cam && opt.nn_grid && route.compact && (size_t)cam->w * cam->h <= ((size_t)1 << 24))) return PR_OK;
    PR_TRY(ensure_nn_grid(pick.set, *s, *cam));
    if (nc.grid_usable) {
        out.nn.grid = nc.nn_grid.as<float4>(); out.nn.gw = cam->w; out.nn.gh = cam->h; out.nn.gfx = cam->fx; out.nn.gfy = cam->fy; out.nn.gcx = cam->cx; out.nn.gcy = cam->cy;
        const size_t w4 = (cam->w + 3) / 4, h4 = (cam->h + 3) / 4, w16 = (w4 + 3) / 4, h16 = (h4 + 3) / 4;
        out.nn.pyr4 = out.nn.grid + (size_t)cam->w * cam->h; out.nn.pyr16 = out.nn.pyr4 + w4 * h4; out.nn.pyr64 = out.nn.pyr16 + w16 * h16;
    }
    return PR_OK;
}
// closest-point grid: the caller's two arrays as they are: nothing is derived from them and nothing is kept by address
static int scene_grid(const void *scene, SceneSel &out)
{
    const pr_scene_grid *s = static_cast<const pr_scene_grid *>(scene);
    PR_TRY(grid_desc_ok("pr_scene_grid", s, /*built=*/true));
    out.grid = prk::SceneGridDev{ { s->origin[0], s->origin[1], s->origin[2] }, s->cell, s->inv_cell, { s->dim[0], s->dim[1], s->dim[2] }, s->max_dist_diff,
                                  s->cell_point, reinterpret_cast<const float4 *>(s->rec) };
    return PR_OK;
}
int make_scene(int kind, const void *scene, bool want_packed, SceneSel &out, PackedCache *pc_in, hipStream_t st, const Camera *cam,
               bool verify_now)
{
    out.kind = kind;
    if (kind == PR_SCENE_PROJ || kind == PR_SCENE_PROJ_CROP) return scene_proj(kind, scene, want_packed, out, pc_in ? *pc_in : g->packed, st ? st : g->stream, verify_now);
    if (kind == PR_SCENE_NN) return scene_nn(scene, out, cam, verify_now);
    if (kind == PR_SCENE_GRID) return scene_grid(scene, out);
    set_error("unknown scene kind %d", kind);
    return PR_ERR_INVALID;
}

// KDTree_cpu::build_tree on the device (kd_build.hip): three launches per level over all points; the host reads the 32-byte control record back
// after twelve levels and then every four (launches past the last level return at once)
int kd_build_dev(pr_vec3 *pcd, pr_vec3 *nrm, uint32_t n, int max_leaf, pr_kdnode *nodes, size_t cap, uint32_t *n_nodes)
{
    if (n == 0 || cap == 0) { set_error("kd-tree build: no points"); return PR_ERR_INVALID; }
    if (n >= 0x7fffffffu) { set_error("kd-tree build: %u points are more than the node records' int ranges hold", n); return PR_ERR_INVALID; }
    const uint32_t cap32 = (uint32_t)std::min<size_t>(cap, 0x7fffffff);
    prk::KdWork w;
    PR_TRY(g->kd_scratch.ensure(prk::kd_work_bytes(n, cap32, max_leaf, nullptr)));
    w.base = g->kd_scratch.p;
    prk::kd_work_bytes(n, cap32, max_leaf, &w);
    PR_TRY(g->kd_tmp.ensure(sizeof(pr_vec3) * 2 * (size_t)n));
    HIP_TRY(prk::launch_kd_init(w, nodes, cap32, pcd, n, max_leaf, g->stream));
    prk::KdCtrl ctrl{};
    uint32_t level = 0;
    for (uint32_t until = 12; ; until += 4) {
        for (; level < until; ++level) HIP_TRY(prk::launch_kd_level(w, nodes, cap32, pcd, n, max_leaf, level, g->stream));
        PR_TRY(read_back_words(w.ctrl[level & 1u], &ctrl, (uint32_t)(sizeof ctrl / sizeof(uint32_t)), g->stream));
        if (ctrl.error == 2u) { set_error("kd-tree build: a level holds more nodes than the work arrays were sized for (%u points, max_leaf %d) -- an internal bound, not the caller's capacity", n, max_leaf); return PR_ERR_INVALID; }
        if (ctrl.error) { set_error("kd-tree build: node capacity %u too small", cap32); return PR_ERR_NOMEM; }
        if (ctrl.done) break;
        if (level >= 4096) { set_error("kd-tree build: more than 4096 levels (max_leaf %d)", max_leaf); return PR_ERR_INVALID; }
    }
    pr_vec3 *tp = g->kd_tmp.as<pr_vec3>(), *tn = tp + n;
    HIP_TRY(prk::launch_kd_permute(w, level, pcd, nrm, n, tp, tn, g->stream));
    HIP_TRY(hipMemcpyAsync(pcd, tp, sizeof(pr_vec3) * n, hipMemcpyDeviceToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(nrm, tn, sizeof(pr_vec3) * n, hipMemcpyDeviceToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (n_nodes) *n_nodes = ctrl.next;
    return PR_OK;
}

template <typename T>
int scene_nn_prepare_dev_t(const T *depth, const float K[9], uint32_t W, uint32_t H, int max_leaf, pr_vec3 *pcd, pr_vec3 *nrm,
                           pr_kdnode *nodes, size_t cap, uint32_t *n_points, uint32_t *n_nodes)
{
    const size_t px = (size_t)W * H;
    PR_TRY(g->nn_full.ensure(sizeof(pr_vec3) * 2 * px));
    PR_TRY(g->row_count.ensure(sizeof(uint32_t) * H));
    PR_TRY(g->row_off.ensure(sizeof(uint32_t) * H));
    PR_TRY(g->counts.ensure(sizeof(uint32_t)));
    pr_vec3 *full_pcd = g->nn_full.as<pr_vec3>(), *full_nrm = full_pcd + px;
    // normals of every pixel (get_normal sees the uint16 image), then the valid pixels in row-major order
    HIP_TRY(prk::launch_scene_proj_prepare<T>(depth, W, H, K[0], K[4], K[2], K[5], full_pcd, full_nrm, g->stream));
    HIP_TRY(prk::launch_nn_gather<T>(depth, W, H, K[0], K[4], K[2], K[5], full_nrm, g->row_count.as<uint32_t>(), g->row_off.as<uint32_t>(),
                                     g->counts.as<uint32_t>(), nullptr, nullptr, false, g->stream));
    uint32_t n = 0;
    PR_TRY(read_back_words(g->counts.p, &n, 1, g->stream));
    if (n_points) *n_points = n;
    if (n == 0) { if (n_nodes) *n_nodes = 0; return PR_OK; }
    HIP_TRY(prk::launch_nn_gather<T>(depth, W, H, K[0], K[4], K[2], K[5], full_nrm, g->row_count.as<uint32_t>(), g->row_off.as<uint32_t>(),
                                     g->counts.as<uint32_t>(), pcd, nrm, true, g->stream));
    return kd_build_dev(pcd, nrm, n, max_leaf, nodes, cap, n_nodes);
}

}  // namespace prr

using namespace prr;

extern "C" {

int pr_scene_proj_prepare_dev(const void *depth_dev, int depth_is_i32, const float K[9], size_t width, size_t height,
                              pr_vec3 *pcd_dev_out, pr_vec3 *normal_dev_out)
{
    PR_ENTER();
    if (!depth_dev || !K || !pcd_dev_out || !normal_dev_out || width == 0 || height == 0) { set_error("pr_scene_proj_prepare_dev: bad arguments"); return PR_ERR_INVALID; }
    note_write(pcd_dev_out, width * height * sizeof(pr_vec3)); note_write(normal_dev_out, width * height * sizeof(pr_vec3));
    HIP_TRY(with_depth(depth_dev, depth_is_i32 != 0, [&](auto *depth) {
        return prk::launch_scene_proj_prepare(depth, (uint32_t)width, (uint32_t)height, K[0], K[4], K[2], K[5], pcd_dev_out, normal_dev_out, g->stream);
    }));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

int pr_kdtree_build_dev(pr_vec3 *pcd_dev, pr_vec3 *normal_dev, size_t n_points, int max_leaf, pr_kdnode *nodes_dev_out, size_t cap_nodes, uint32_t *n_nodes)
{
    PR_ENTER();
    if (!pcd_dev || !normal_dev || !nodes_dev_out) { set_error("pr_kdtree_build_dev: bad arguments"); return PR_ERR_INVALID; }
    note_write(pcd_dev, n_points * sizeof(pr_vec3)); note_write(normal_dev, n_points * sizeof(pr_vec3)); note_write(nodes_dev_out, cap_nodes * sizeof(pr_kdnode));
    return kd_build_dev(pcd_dev, normal_dev, (uint32_t)n_points, max_leaf, nodes_dev_out, cap_nodes, n_nodes);
}

int pr_scene_nn_prepare_dev(const void *depth_dev, int depth_is_i32, const float K[9], int width, int height, int max_leaf,
                            pr_vec3 *pcd_dev_out, pr_vec3 *normal_dev_out, pr_kdnode *nodes_dev_out, size_t cap_nodes,
                            uint32_t *n_points, uint32_t *n_nodes)
{
    PR_ENTER();
    if (!depth_dev || !K || !pcd_dev_out || !normal_dev_out || !nodes_dev_out || width <= 0 || height <= 0) { set_error("pr_scene_nn_prepare_dev: bad arguments"); return PR_ERR_INVALID; }
    note_write(pcd_dev_out, (size_t)width * height * sizeof(pr_vec3)); note_write(normal_dev_out, (size_t)width * height * sizeof(pr_vec3)); note_write(nodes_dev_out, cap_nodes * sizeof(pr_kdnode));
    return with_depth(depth_dev, depth_is_i32 != 0, [&](auto *depth) {
        return scene_nn_prepare_dev_t(depth, K, (uint32_t)width, (uint32_t)height, max_leaf, pcd_dev_out, normal_dev_out, nodes_dev_out, cap_nodes, n_points, n_nodes);
    });
}

// pr_scene_grid over the box [lo, hi]: pure host code.  dim[a] = floor((hi[a] - lo[a]) * inv_cell) + 1 in float32, so that hi itself -- and with it the
// whole box -- lies inside the grid (a point is inside iff (p - origin) * inv_cell < dim), and lo == hi gives one cell.
int pr_scene_grid_describe(const float lo[3], const float hi[3], float cell, float max_dist_diff, float reach, pr_scene_grid *out)
{
    const char *fn = "pr_scene_grid_describe";
    if (!lo || !hi || !out) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(cell) || !(cell > 0.0f)) { set_error("%s: cell must be finite and positive (got %g)", fn, (double)cell); return PR_ERR_INVALID; }
    const float inv_cell = 1.0f / cell;
    if (!std::isfinite(inv_cell) || !(inv_cell > 0.0f)) { set_error("%s: 1 / cell is not a positive finite float (cell %g)", fn, (double)cell); return PR_ERR_INVALID; }
    if (!std::isfinite(max_dist_diff) || !(max_dist_diff > 0.0f) || !std::isfinite(reach) || !(reach > 0.0f)) {
        set_error("%s: max_dist_diff and reach must be finite and positive (got %g, %g)", fn, (double)max_dist_diff, (double)reach); return PR_ERR_INVALID;
    }
    pr_scene_grid gd;
    std::memset(&gd, 0, sizeof gd);
    uint64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) { set_error("%s: lo[%d] / hi[%d] is not finite", fn, a, a); return PR_ERR_INVALID; }
        if (hi[a] < lo[a]) { set_error("%s: hi[%d] = %g is below lo[%d] = %g", fn, a, (double)hi[a], a, (double)lo[a]); return PR_ERR_INVALID; }
        const volatile float extent = hi[a] - lo[a];              // (volatile: each step rounded to float32, whatever the host compiler's excess precision)
        const volatile float f = extent * inv_cell;
        if (!(f < 4294967040.0f)) { set_error("%s: dim[%d] overflows 32 bits (extent %g, cell %g)", fn, a, (double)extent, (double)cell); return PR_ERR_INVALID; }
        const uint64_t d = (uint64_t)std::floor((float)f) + 1u;
        cells = (d > PR_GRID_MAX_CELLS) ? (uint64_t)PR_GRID_MAX_CELLS + 1u : cells * d;
        if (cells > PR_GRID_MAX_CELLS) { set_error("%s: more than PR_GRID_MAX_CELLS = %u cells (a larger cell or a smaller box)", fn, (uint32_t)PR_GRID_MAX_CELLS); return PR_ERR_INVALID; }
        gd.origin[a] = lo[a]; gd.dim[a] = (uint32_t)d;
    }
    gd.cell = cell; gd.inv_cell = inv_cell; gd.max_dist_diff = max_dist_diff; gd.reach = reach;
    *out = gd;
    return PR_OK;
}

// The build of a closest-point grid into the caller's buffers: one exact search of the scene's kd-tree per cell centre (grid_build_kernel), the
// scene points and normals repacked as 32-byte records.  make_scene derives the tree's traversal arrays, or finds them derived.
int pr_scene_grid_build_dev(const pr_scene_nn *scene, pr_scene_grid *grid, uint32_t *cell_point_dev, float *rec_dev)
{
    PR_ENTER();
    const char *fn = "pr_scene_grid_build_dev";
    if (!scene || !cell_point_dev || !rec_dev) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    PR_TRY(grid_desc_ok(fn, grid, /*built=*/false));
    if (scene->n_points >= (1u << 27)) { set_error("%s: %u scene points, at most 2^27 - 1", fn, scene->n_points); return PR_ERR_INVALID; }
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    PR_TRY(make_scene(PR_SCENE_NN, scene, false, sc));
    const size_t cells = (size_t)grid->dim[0] * grid->dim[1] * grid->dim[2];
    note_write(cell_point_dev, cells * sizeof(uint32_t)); note_write(rec_dev, (size_t)scene->n_points * 8 * sizeof(float));
    const prk::SceneGridDev gd{ { grid->origin[0], grid->origin[1], grid->origin[2] }, grid->cell, grid->inv_cell, { grid->dim[0], grid->dim[1], grid->dim[2] },
                                grid->max_dist_diff, cell_point_dev, reinterpret_cast<const float4 *>(rec_dev) };
    HIP_TRY(prk::launch_grid_build(sc.nn, grid->reach, gd, cell_point_dev, g->stream));
    HIP_TRY(prk::launch_grid_records(scene->pcd, scene->normal, scene->n_points, reinterpret_cast<float4 *>(rec_dev), g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    grid->cell_point = cell_point_dev; grid->rec = rec_dev; grid->n_points = scene->n_points;
    return PR_OK;
}

// Audit entry: the derived search data of a kd-tree scene, as make_scene hands it to the searches (SceneSel::nn) and keeps it (the picked
// NNDerived), copied to the host.  make_scene is the only build path: whatever it reuses, rebuilds or waits for, it does here too.
int pr_debug_nn_records(const pr_scene_nn *scene, uint32_t cam_w, uint32_t cam_h, const float *cam_k, pr_nn_records_counts *counts,
                        const pr_nn_records_out *out)
{
    PR_ENTER();
    if (!scene) { set_error("pr_debug_nn_records: null scene"); return PR_ERR_INVALID; }
    if (cam_k && (cam_w == 0 || cam_h == 0)) { set_error("pr_debug_nn_records: a camera of %u x %u pixels", cam_w, cam_h); return PR_ERR_INVALID; }
    Camera cam{ cam_w, cam_h, cam_k ? cam_k[0] : 0.0f, cam_k ? cam_k[1] : 0.0f, cam_k ? cam_k[2] : 0.0f, cam_k ? cam_k[3] : 0.0f };
    SceneSel sc;
    std::memset(static_cast<void *>(&sc), 0, sizeof sc);
    PR_TRY(make_scene(PR_SCENE_NN, scene, false, sc, nullptr, nullptr, cam_k ? &cam : nullptr));
    const NNDerived &nc = g->nn_sets[sc.nn_set];
    const prk::SceneNNDev &nn = sc.nn;
    const size_t n_nodes = nc.n_nodes, n_points = nc.n_points;
    const size_t n_wide = std::min<size_t>(nc.info.n_wide, prk::nn_wide_capacity(nc.n_nodes));
    // the grid of THIS camera (without one make_scene may still have built the grid of the scene's own hint: not what was asked for)
    const bool grid = cam_k && nc.grid_valid && nc.gw == cam_w && nc.gh == cam_h && std::memcmp(nc.gk, cam_k, sizeof nc.gk) == 0 && nc.nn_cells.p && nc.nn_grid.p;
    const size_t cells = grid ? (size_t)cam_w * cam_h : 0, grid_cells = grid ? prk::nn_grid_cells(cam_w, cam_h) : 0;
    if (counts) *counts = pr_nn_records_counts{ nc.n_nodes, nc.n_points, (uint32_t)n_wide, grid ? cam_w : 0u, grid ? cam_h : 0u, (grid && nc.grid_usable) ? 1u : 0u, grid_cells };
    if (!out) return PR_OK;
    const struct { void *dst; const void *src; size_t bytes; } copies[] = {
        { out->topo, nn.topo, n_nodes * sizeof(int4) }, { out->bmin, nn.bmin, n_nodes * sizeof(float4) }, { out->bmax, nn.bmax, n_nodes * sizeof(float4) },
        { out->rec64, nn.rec, n_nodes * 4 * sizeof(float4) }, { out->rec32, nc.nnrec32.p, n_nodes * 2 * sizeof(uint4) }, { out->desc, nn.desc, n_nodes * sizeof(uint2) },
        { out->pts, nn.pts, n_points * sizeof(float4) }, { out->wide, nc.nnwide.p, n_wide * 128 },
        { out->cell_idx, nc.nn_cells.p, cells * sizeof(int32_t) }, { out->grid, nc.nn_grid.p, grid_cells * sizeof(float4) } };
    hipError_t e = hipSuccess;
    for (const auto &c : copies)
        if (e == hipSuccess && c.dst && c.src && c.bytes) e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("pr_debug_nn_records: %s", hipGetErrorString(e)); return PR_ERR_HIP; }
    if (out->info) std::memcpy(out->info, &nc.info, sizeof nc.info);  // (the host's copy: what make_scene itself decides on; 24 words, prk::NNInfo)
    return PR_OK;
}

int pr_raw2depth_mask(const int32_t *raw_dev, size_t count, uint16_t *depth_host_out, uint8_t *mask_host_out)
{
    PR_ENTER();
    if (count == 0) return PR_OK;                                  // (an empty render stack has no array)
    if (!raw_dev || (!depth_host_out && !mask_host_out)) { set_error("pr_raw2depth_mask: bad arguments"); return PR_ERR_INVALID; }
    if (depth_host_out) PR_TRY(g->conv16.ensure(count * sizeof(uint16_t) + 16));
    if (mask_host_out) PR_TRY(g->conv8.ensure(count + 16));
    HIP_TRY(prk::launch_raw2depth_mask(raw_dev, count, depth_host_out ? g->conv16.as<uint16_t>() : nullptr, mask_host_out ? g->conv8.as<uint8_t>() : nullptr, g->stream));
    // ONE copy per output for the whole stack (the reference issues one thrust::copy per pose, renderer.cu:370-373)
    if (depth_host_out) HIP_TRY(hipMemcpyAsync(depth_host_out, g->conv16.p, count * sizeof(uint16_t), hipMemcpyDeviceToHost, g->stream));
    if (mask_host_out) HIP_TRY(hipMemcpyAsync(mask_host_out, g->conv8.p, count, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

// Scene_projective restricted to a window of the frame: copies the window's rows of the full-frame arrays
int pr_scene_proj_crop_dev(const pr_vec3 *pcd_full_dev, const pr_vec3 *normal_full_dev, size_t width, size_t height, pr_roi window,
                           pr_vec3 *pcd_out_dev, pr_vec3 *normal_out_dev)
{
    PR_ENTER();
    if (!pcd_full_dev || !normal_full_dev || !pcd_out_dev || !normal_out_dev || window.width <= 0 || window.height <= 0 || window.x < 0 || window.y < 0 ||
        (size_t)window.x + (size_t)window.width > width || (size_t)window.y + (size_t)window.height > height) { set_error("pr_scene_proj_crop_dev: bad arguments"); return PR_ERR_INVALID; }
    const size_t cw = (size_t)window.width, ch = (size_t)window.height;
    note_write(pcd_out_dev, cw * ch * sizeof(pr_vec3)); note_write(normal_out_dev, cw * ch * sizeof(pr_vec3));
    const size_t off = (size_t)window.y * width + (size_t)window.x;
    HIP_TRY(hipMemcpy2DAsync(pcd_out_dev, cw * sizeof(pr_vec3), pcd_full_dev + off, width * sizeof(pr_vec3), cw * sizeof(pr_vec3), ch, hipMemcpyDeviceToDevice, g->stream));
    HIP_TRY(hipMemcpy2DAsync(normal_out_dev, cw * sizeof(pr_vec3), normal_full_dev + off, width * sizeof(pr_vec3), cw * sizeof(pr_vec3), ch, hipMemcpyDeviceToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return PR_OK;
}

}  // extern "C"
