// pr_internal.h -- declarations shared by the HIP kernels TU and the C-ABI/host TUs.
// Not part of the public boundary (that is include/pose_refine.h).
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "pose_refine.h"
#include "pr_tuning.h"

namespace prk {

// ---- canonical reduction geometry (DESIGN.md "canonical tree"; oracle: sum29_canonical) -----------
constexpr uint32_t kBlockThreads   = 256;                       // 4 wavefronts
constexpr uint32_t kPointsPerLane  = 4;                         // consecutive points per lane per step
constexpr uint32_t kPointsPerStep  = kBlockThreads * kPointsPerLane;   // 1024
constexpr uint32_t kAccStride      = 32;                        // 29 sums padded to 32 floats
constexpr uint32_t kCloudAlign     = 32;                        // fused path: a hypothesis' cloud starts where the one before it ends, rounded up to this many points (128-byte lines; cloud_slot, pose_box.h)
constexpr uint32_t kBoxPack        = 32;                        // fused path: a hypothesis' pixel box is its own little image in the depth workspace, packed behind the one before it, rounded up to this many ints (box_slot, pose_box.h)
constexpr uint32_t kQCountStride   = 4;                         // queue counters per hypothesis (IcpBatch::nn_qcount)
constexpr uint32_t kNNWordsPerPoint = 6;                        // per cloud point: winner | slack | queue 1 (2 words) | queue 2 (2 words) -- laid out by nn_layout (pr_runtime.h)

// per-hypothesis run state consumed by the correspondence kernel
enum : int32_t { kSkip = 0, kRun = 1, kRunWithTransform = 2 };

// everything a workgroup needs to know about its hypothesis, in ONE 64-byte record so that the
// wavefront fetches it with a single scalar load instead of a chain of dependent ones
struct alignas(64) PoseMeta {
    uint32_t start;             // first point of the cloud (in points, relative to IcpBatch::cloud)
    uint32_t count;             // points in the cloud
    int32_t  state;             // kSkip / kRun / kRunWithTransform
    uint32_t pad;
    float    xform[12];         // pending rigid update, rows 0..2 of the 4x4
};
static_assert(sizeof(PoseMeta) == 64, "PoseMeta must stay one 64-byte record");

struct DevIcpState;
// batch of model clouds handed to one correspondence pass
struct IcpBatch {
    pr_vec3        *cloud;      // base of all clouds (dev)
    const PoseMeta *meta;       // [P] (dev)
    float          *partial;    // [P][nblk][kAccStride] workgroup sums (dev)
    uint32_t        nblk;       // 2048-point blocks a hypothesis may have = stride of `partial` (and grid.x unless grid_x is set)
    uint32_t        grid_x;     // 0, or the number of workgroups per hypothesis when it differs from nblk (workgroups then loop over blocks)
    uint32_t        steps;      // steps of 1024 points per workgroup
    // PR_SOLVE_DEVICE with the solve fused into the pass (option "fused_solve"): the workgroup that delivers the last
    // partial sum of a hypothesis also adds the partials up and runs that hypothesis' iteration logic
    uint32_t        score_only; // 1 on the pass of iteration == max_iteration (PR_SOLVE_DEVICE): only sums 27 (error) and 28 (count) are formed
    uint32_t        fused;      // 0 = separate icp_finalize[_solve] launch; 1 = finalize + solve in the pass; 2 = finalize in the pass, the 29 sums of a
                                // hypothesis go to sums_out (PR_SOLVE_HOST: pinned host memory, read by the host after the stream has drained)
    float          *sums_out;   // fused == 2: [P][kAccStride], same pose indexing as `meta`
    uint32_t       *grp_count;  // fused == 2, optional: device counter of the hypotheses of this launch's pose GROUP that have delivered their sums; the one that makes it
    uint32_t        grp_expected;   // grp_expected re-zeroes it and stores iter + 1 into *grp_flag (pinned host memory): the host polls that one word instead of waiting for the stream
    uint32_t       *grp_flag;
    uint32_t        iter;       // iteration index of this pass (icp.cu:178 loop variable)
    DevIcpState    *st;         // [P]
    uint32_t       *arrive;     // [P] zero before the first pass; the solving workgroup re-zeroes its entry
    uint32_t       *nn_prev;    // kd-tree scenes: per cloud point (same indexing as `cloud`) the scene index of the previous pass' winner, or null
    float          *nn_slack;   // kd-tree scenes, search kernel: per cloud point, a lower bound on the distance of every scene point OTHER than the
                                // winner, minus the distance the point has travelled since that bound was established (<= 0: none)
    uint2          *nn_queue;   // search kernel -> tree kernel: per hypothesis (same indexing as the cloud) the (point, bound) of every query the first
                                // half could not settle;  nn_qcount: kQCountStride counters per hypothesis (same pose indexing as `meta`): fill levels
                                // of queue 1 and of queue 2, two each, alternating per pass
    uint32_t       *nn_qcount;
    uint2          *nn_queue2;  // bound kernel -> task walk: what the pixel window could not settle either, (point, bound)
    uint32_t        pre_transformed;   // 1: the pending update has already been applied to the cloud (nn_search_kernel): the pass must not apply it again
    pr_criteria     crit;
    // robust weight of the pass (pr_robust, include/pose_refine.h), uniform: read by the kRobust instantiations only, which the launchers pick
    // when robust_kind != PR_ROBUST_NONE.  (Behind every older member: their offsets in the kernel argument stay what they were.)
    uint32_t        robust_kind;
    float           robust_c, robust_inv_c;
    uint32_t        lds_blocks; // icp_loop_cu_kernel only: blocks of every cloud's head kept in LDS over the loop (icp_loop_cu_lds_blocks); 0 = none
};
// the weight as the per-point audit kernels take it
struct RobustArgs { uint32_t kind; float c, inv_c; float *corr; };   // corr: null, or n x 8 floats {dx, dy, dz, valid, nx, ny, nz, w}

// projective scene exactly as the reference API hands it over (two Vec3f arrays)
struct SceneProjAoS {
    uint32_t width, height;
    float max_dist_diff, fx, fy, cx, cy;
    float tlx, tly;             // (float)tl_x, (float)tl_y of pcd2dep (common.h:64-67): 0 unless the scene buffers cover a crop of the frame
    const pr_vec3 *pcd, *normal;
};
// projective scene repacked by the fused pipeline: one 16-byte record {nx,ny,nz,z} per pixel
struct SceneProjPacked {
    uint32_t width, height;
    float max_dist_diff, fx, fy, cx, cy;
    float tlx, tly;
    const float4 *rec;
    const float *colf, *rowf;   // colf[x] = ((float)(x + tl_x) - cx)/fx, rowf[y] = ((float)(y + tl_y) - cy)/fy
};
// the same scene with the two tables copied into the workgroup's LDS (icp_loop_cu_kernel, option "loop_lds_tables"): a type of its own, built inside
// the kernel from its LDS array, so that after inlining the table loads of gather_issue are LDS loads at every call site and never flat ones
struct SceneProjPackedLds {
    SceneProjPacked pk;         // pk.colf / pk.rowf are not read through this type
    const float *colf, *rowf;   // LDS: pk.width and pk.height floats
};
// kd-tree scene: reference arrays + the traversal structure derived from them (build_nn_accel)
struct SceneNNDev {
    float max_dist_diff;
    const int4   *topo;         // per node: {split_v|left, child1|right, child2|-1, (parent+1)|dim<<30}
    const float4 *bmin, *bmax;  // per node tight bbox (leaves included)
    const float4 *pts;          // per point {x,y,z,0}
    const pr_vec3 *pcd, *normal;
    uint32_t n_nodes;
    uint32_t lds_nodes;         // how many leading (top-level) nodes the kernel stages in LDS (stackless: 16-byte topo entries; stack: 64-byte records)
    const float4 *rec;          // stack variant: 64-byte record per node (4 x float4), see nn_records_kernel
    uint32_t stack_depth;       // 0 = stackless traversal, else per-lane LDS stack entries (>= tree depth)
    // stack variant, compact form: 32-byte record per node (see nn_records32_kernel) with the two child boxes quantised to
    // 16 bits in the frame of the root box, rounded outwards; null when the tree cannot be expressed that way
    const uint4 *rec32;
    float qmin[3], qscale[3];   // dequantisation: qmin[a] + (float)q * qscale[a]
    const uint2 *desc;          // first 8 bytes of every compact record on their own (split | child | dim): all a descent needs when the
                                // split plane alone already rules the far side out
    // Pixel grid of the scene points (build_nn_grid): cell (px, py) of a gw x gh image holds the scene point that projects into
    // it under (gfx, gfy, gcx, gcy) as {x, y, z, index}, or {huge, huge, huge, -1}.  Null unless every scene point owns a cell of
    // its own (always the case for a Scene_nn made from a depth image with the same intrinsics, pcd_scene.cpp:10-29).
    const float4 *grid;
    uint32_t gw, gh;
    float gfx, gfy, gcx, gcy;
    // three coarser levels of the same grid: one representative scene point per 4 x 4, 16 x 16 and 64 x 64 pixel block
    // (the occupied sub-block nearest the block's centre, recursively), same {x, y, z, index} cells
    const float4 *pyr4, *pyr16, *pyr64;
    // wide records (nn_wide_layout_kernel): one 128-byte line per wide node = eight slots {subtree box, reference}; null when the tree
    // cannot be expressed that way (the binary walk of nn_tree_kernel is used)
    const uint4 *wide;
    uint32_t n_wide;
    float wmin[3], wscale;      // frame of the wide records: coordinate = wmin[a] + (float)q * wscale (one scale for the three axes)
    // instrumented runs (option "nn_count"): per ICP pass (IcpBatch::iter) a row of eight 64-bit counters, the columns of enum NNCounter
    // (nn_search.hip): kCntQueries, kCntWindow, kCntTree, kCntDescents, kCntNodes, kCntLeaves, kCntLeafPoints, kCntCells; else null
    unsigned long long *counters;
    uint32_t topo_nodes;        // host side only: lds_nodes of a stackless launch over this scene (option nn_lds_nodes), whatever walk stack_depth selects
};
// kd-tree scene after the search kernel has run: the correspondence pass only gathers the winners (no search, no transform)
struct SceneNNWinners {
    float max_dist_diff;
    const float4 *pts;          // {x,y,z,0} per scene point
    const pr_vec3 *normal;
    const uint32_t *winner;     // per cloud point (same indexing as IcpBatch::cloud): scene index or 0xffffffff
};

// closest-point grid scene (pr_scene_grid, include/pose_refine.h) as the kernels of grid_scene.hip take it
struct SceneGridDev {
    float origin[3], cell, inv_cell;
    uint32_t dim[3];
    float max_dist_diff;
    const uint32_t *cell_point; // per cell (x fastest): scene point nearest to the cell's centre, or PR_GRID_NONE
    const float4 *rec;          // per scene point: {px, py, pz, 0}, {nx, ny, nz, 0}
};

// device-side solver state for PR_SOLVE_DEVICE (one record per hypothesis)
struct DevIcpState {
    float T[16];
    float fitness, rmse;
    int32_t done;               // 0 running, 1 finished
    int32_t passes;
};

// ---- launchers (all asynchronous on `s`) ----------------------------------------------------------
hipError_t launch_fill_i32(int32_t *dst, size_t n, int32_t v, hipStream_t s);
hipError_t launch_sentinel2zero(int32_t *plane, size_t n, bool far, hipStream_t s);      // "nothing drawn" to 0: INT_MAX of a near plane, INT_MIN of a far one

// depth -> cloud: rows are counted, scanned per image, then emitted in row-major order.
// images: n_img images of width*height pixels each `img_stride` elements apart; cloud i is written
// at cloud + i*cloud_stride; counts[i] receives its size.  empty_intmax: INT_MAX also means "no depth".
template <typename T>
hipError_t launch_depth2cloud(const T *depth, uint32_t n_img, size_t img_stride, uint32_t width, uint32_t height,
                              uint32_t stride, uint32_t tl_x, uint32_t tl_y, float fx, float fy, float cx, float cy,
                              bool empty_intmax, uint32_t *row_count, uint32_t *row_off, uint32_t *counts,
                              pr_vec3 *cloud, size_t cloud_stride, bool emit, hipStream_t s);

hipError_t launch_model_aabb(const pr_triangle *tris, uint32_t n_tris, uint32_t *keys, float *aabb_out, const float *expect, uint32_t *flag_out, hipStream_t s);
hipError_t launch_render_bands(const pr_triangle *tris, uint32_t n_tris, const pr_mat4 *poses_dev, uint32_t n_poses, const float *aabb,
                               int4 *bbox, int32_t *depth, uint32_t *row_count, uint32_t *row_off, uint32_t *counts,
                               uint32_t width, uint32_t height, const pr_mat4 &proj, pr_roi roi, uint32_t n_cus, hipStream_t s);
// The two per-batch safety nets of the asynchronous path, carried by the raster launch itself (round 5): the workgroups of the launch's FIRST
// hypothesis fold their triangles' vertices into keys[0..5] (running minima; keys[6] = arrival ticket; armed once by the caller with six
// words of ones and a zero, re-armed by the last workgroup), the last one compares with the box the host assumed; workgroup (0, 0) takes
// the sampled fingerprint of the caller's scene arrays (fp_expected null: none).  Both only ever RAISE *flag.  keys null: no check.
// The raster may run on the library's ordered copy of the mesh (ensure_model_box): the checks read the CALLER's buffer (`caller`, lane triangle
// ti) and, beside its box, add up its multiset fingerprint (triangle_hash, pose_box.h) in keys[8..9] (one 64-bit word, armed with zero and
// re-armed like the ticket); the last workgroup compares it with `mesh_hash`, the value of the content the copy was made from.
struct AabbExpected { float v[6]; };
constexpr uint32_t kBatchCheckWords = 10;   // keys[0..5] box, [6] ticket, [7] spare, [8..9] fingerprint sum
struct BatchCheck {
    uint32_t *keys; AabbExpected expect;
    const pr_triangle *caller; unsigned long long mesh_hash;
    const uint32_t *fa, *fb, *fc; unsigned long long na, nb, nc; const uint32_t *fp_expected;
    uint32_t *flag;
};
// The caller's arrays a scene cache is derived from, as every fingerprint of them reads them: 32-bit words, IN THIS ORDER (the hashes mix the
// array's ordinal in, so a site that listed them differently would find every batch stale).  A kd-tree scene's order is not its struct's.
struct SceneSources {
    const void *p[3]; size_t bytes[3];                           // unused entries: null, 0
    const uint32_t *words(int k) const { return static_cast<const uint32_t *>(p[k]); }
    unsigned long long n_words(int k) const { return (unsigned long long)(bytes[k] / 4); }
};
inline SceneSources scene_sources(const pr_scene_proj &s)
{
    const size_t b = (size_t)s.width * s.height * sizeof(pr_vec3);
    return SceneSources{ { s.pcd, s.normal, nullptr }, { b, b, 0 } };
}
inline SceneSources scene_sources(const pr_scene_nn &s)
{
    const size_t b = (size_t)s.n_points * sizeof(pr_vec3);
    return SceneSources{ { s.pcd, s.nodes, s.normal }, { b, (size_t)s.n_nodes * sizeof(pr_kdnode), b } };
}
// the scene half of a batch's check: the arrays, and the sampled fingerprint taken when their cached form was built (FpWords::sample, below)
inline void check_sources(BatchCheck &chk, const SceneSources &src, const uint32_t *expected)
{
    chk.fa = src.words(0); chk.na = src.n_words(0); chk.fb = src.words(1); chk.nb = src.n_words(1); chk.fc = src.words(2); chk.nc = src.n_words(2);
    chk.fp_expected = expected;
}
// Asynchronous path, option tight_box (pose_tight_box_kernel): bbox[i], the loose box the host uploaded, overwritten by its intersection with the
// hull of the projected vertices `verts` ({x, y, z, 0}: the mesh's distinct vertices); then, per sub-batch, the packed offsets of those boxes.
hipError_t launch_tight_boxes(const float4 *verts, uint32_t n_verts, const pr_mat4 *poses_dev, uint32_t n_poses, const pr_mat4 &proj,
                              uint32_t width, uint32_t height, int4 *bbox, hipStream_t s);
hipError_t launch_box_pack_offsets(const int4 *bbox, uint32_t n_poses, uint32_t *box_off, uint32_t height, bool bands, hipStream_t s);
// Mixed batches (pr_*_multi): the hypotheses grouped by mesh.  One group of consecutive hypotheses [first, first + count) of a launch that share
// a mesh; raster_multi_kernel's workgroups [first_wg, first_wg + tri_blocks * ceil(count / run)) are its (triangle block, pose run) pairs.
// The host fills tris, n_tris, first and count; launch_raster the rest.  48 bytes: staged in 16-byte words.
struct RasterGroup {
    const pr_triangle *tris;
    uint32_t n_tris, first, count, run;
    uint32_t tri_blocks, reserved0;
    unsigned long long first_wg, reserved1;
};
static_assert(sizeof(RasterGroup) == 48, "RasterGroup: three 16-byte words");
// keys: 6 x n_meshes words of scratch; aabb_out: 6 floats per mesh (launch_model_aabb's box for each mesh alone)
hipError_t launch_model_aabb_multi(const pr_mesh_ref *meshes_dev, const pr_mesh_ref *meshes_host, uint32_t n_meshes, uint32_t *keys, float *aabb_out, hipStream_t s);
// What a raster draws: one mesh for every hypothesis (tris, n_tris), or -- groups_host given -- a mixed batch's groups (groups_host: pinned, filled by the
// host; groups_mapped: the same memory as the device sees it; groups_dev: where launch_raster stages the completed groups).  For launch_render_boxes'
// box front end also the model box(es), 6 floats each, and (mixed batch) the box every hypothesis takes.
struct RasterMesh {
    const pr_triangle *tris; uint32_t n_tris;
    RasterGroup *groups_host; const void *groups_mapped; uint32_t n_groups; RasterGroup *groups_dev;
    const float *aabb; const uint32_t *box_index;
};
// Where the fragments go, under which camera.  depth: the near plane (atomicMin); far: null, or a second plane of the same layout that takes every
// fragment with atomicMax (span renders).  boxes null: full images of rw x rh (the frame, or the window `roi`), hypothesis i in image i -- of a mixed
// batch in image image_of[i] when that is given.  boxes: each hypothesis' pixel box, in full frames or (box_off) packed into the plane at these
// offsets (ints), each with its own pitch; bands: packed in the banded layout of pose_box.h (band_box), placed by box_slot_of -- fill, raster and
// count then address that layout, and so must launch_emit_box.
struct RasterTarget {
    int32_t *depth, *far;
    const int4 *boxes; const uint32_t *box_off, *image_of;
    uint32_t rw, rh; pr_roi roi; bool bands;
    uint32_t width, height; const pr_mat4 *proj;
};
// launch_render_boxes' row outputs (all null: none, the boxes are only drawn); meta, st, arrive: the asynchronous path's per-hypothesis records
struct BoxRows { uint32_t *row_count, *row_off, *counts; PoseMeta *meta; DevIcpState *st; uint32_t *arrive; };
// the caller filled the plane(s) with "nothing drawn" (INT_MAX; far: INT_MIN); check (one mesh only): rides on the first hypothesis' workgroups
hipError_t launch_raster(const RasterMesh &mesh, const pr_mat4 *poses_dev, uint32_t n_poses, const RasterTarget &target, const BatchCheck *check, hipStream_t s);
hipError_t launch_render_boxes(const RasterMesh &mesh, const pr_mat4 *poses_dev, uint32_t n_poses, int4 *bbox, const RasterTarget &target, const BoxRows &rows,
                               hipStream_t s, bool compute_boxes = true, const BatchCheck *check = nullptr);
// solid.hip: pr_pose_penetration's P x P records (6 words each: pr_pair_solid) from the two planes of a span render of all P hypotheses; every
// record is written, none needs clearing
hipError_t launch_pair_solid(const int32_t *depth, const int32_t *far, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t height,
                             int32_t slack, uint32_t *records, hipStream_t s);
// verify.hip: every box pixel a hypothesis renders (launch_render_boxes' layout) against the scene frame (int32 or uint16, mm), added into
// records[8 * i] (pr_pose_score words: visible, inlier, occluded, violation, missing, reserved, abs_err_sum lo / hi), which the caller zeroed
hipError_t launch_score_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height,
                              const void *scene, bool scene_i32, int32_t tau, uint32_t *records, hipStream_t s);
// select.hip: the inlier pixels of launch_score_boxes as one bit plane per hypothesis -- dense, height x overlap_words_per_row(width) 64-bit words,
// bit b of word w of image row y = frame pixel (64 w + b, y); only the words a hypothesis' box touches are written, and only those are read --
// and mat[i * n + j] = the number of pixels set in both planes, for every pair (bbox: the boxes the planes were written with, all n of them)
inline uint32_t overlap_words_per_row(uint32_t width) { return (width + 63) / 64; }
hipError_t launch_support_bits(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height,
                               const void *scene, bool scene_i32, int32_t tau, unsigned long long *planes, hipStream_t s);
hipError_t launch_pair_overlap(const unsigned long long *planes, const int4 *bbox, uint32_t n_poses, uint32_t width, uint32_t height, uint32_t *mat, hipStream_t s);
// cover.hip: the cover rule (pr_score_cover) walked in rounds over launch_support_bits' planes and the boxes they were written with, all n of them.
// state: kCoverCtlWords control words (finished, n_selected, claimed, position of the last accepted one), then n pr_pose_cover records, then the
// order position of every hypothesis (kCoverNoPos: not in order), then the hypothesis at every order position, then the selected list (n_order
// words).  launch_cover_init: once per depth chunk behind the score kernel (records: its pr_pose_score words) -- support, state and position of
// hypotheses p0 .. p0 + np - 1, and (p0 == 0) the control words.  launch_cover_round: one gain + commit pair, a no-op once the finished word is set.
// launch_cover_final: fresh of everything not accepted against the final claimed plane.  claimed: height x overlap_words_per_row(width) words, zeroed by the caller
constexpr uint32_t kCoverCtlWords = 8, kCoverNoPos = 0xffffffffu;
struct CoverRule { uint32_t new_num, new_den, min_new, max_keep, n_order; };
struct CoverState {
    uint32_t *ctl, *rec, *pos, *at, *selected;
    static size_t words(size_t n, size_t n_order) { return kCoverCtlWords + 4 * n + n + n_order + n_order; }
    CoverState(uint32_t *base, size_t n, size_t n_order) : ctl(base), rec(base + kCoverCtlWords), pos(rec + 4 * n), at(pos + n), selected(at + n_order) {}
};
hipError_t launch_cover_init(const uint32_t *records, uint32_t p0, uint32_t np, const CoverState &st, hipStream_t s);
hipError_t launch_cover_round(const unsigned long long *planes, const int4 *bbox, uint32_t n_poses, uint32_t width, uint32_t height, const CoverRule &rule,
                              const CoverState &st, unsigned long long *claimed, hipStream_t s);
hipError_t launch_cover_final(const unsigned long long *planes, const int4 *bbox, uint32_t n_poses, uint32_t width, uint32_t height, const CoverState &st,
                              const unsigned long long *claimed, hipStream_t s);
// contour.hip: the scene's edge pixels (bits: height x overlap_words_per_row(width) words) and their chessboard distance transform (row_dist:
// scratch, dist: the result, width x height bytes each, 255 = no edge within radius) -- three launches; and the edge pixels of every rendered box
// counted against them into records[8 * i] (pr_pose_contour words: contour, hit, occluded, miss, reserved x 2, dist_sum lo / hi), which the
// caller zeroed.  window {x0, row0, x1, row1}: the image the renders live in (the frame or the ROI), in image coordinates
hipError_t launch_scene_edge_distance(const void *scene, bool scene_i32, uint32_t width, uint32_t height, int32_t jump_mm, uint32_t radius,
                                      unsigned long long *bits, uint8_t *row_dist, uint8_t *dist, hipStream_t s);
// ... and the nearest edge pixel of every frame pixel's (2 radius + 1)^2 window as ey << 16 | ex, PR_EDGE_NONE when it holds none (row_off: scratch,
// width x height bytes; nearest: width x height words) -- three launches, the first one the distance transform's
hipError_t launch_scene_edge_nearest(const void *scene, bool scene_i32, uint32_t width, uint32_t height, int32_t jump_mm, uint32_t radius,
                                     unsigned long long *bits, int8_t *row_off, uint32_t *nearest, hipStream_t s);
hipError_t launch_contour_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height, int4 window,
                                const void *scene, bool scene_i32, const uint8_t *edge_dist, int32_t tau, int32_t jump_mm, uint32_t *records, hipStream_t s);
// normals.hip: on the inlier pixels of every rendered box (launch_score_boxes' test with tau), the render's normal against the scene's, both estimated
// from depth at distance `step` with neighbours within `jump` (pr_pose_normal's definition), counted into records[8 * i] (pr_pose_normal words: tested,
// agree, disagree, no_render_normal, no_scene_normal, reserved x 3), which the caller zeroed.  m2 = cos_min squared; window as for launch_contour_boxes
struct NormalParams { double fx, cx, fy, cy, m2; uint32_t step; int32_t jump, tau; };      // K[0], K[2], K[4], K[5], each converted to double once
hipError_t launch_normal_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height, int4 window,
                               const void *scene, bool scene_i32, const NormalParams &p, uint32_t *records, hipStream_t s);
// compose.hip: the hypotheses of a call taken together.  keys: width x height 64-bit words, (depth << 32 | caller's index) of the front-most render at every
// frame pixel, all ones where nothing is drawn; index_of: position in the (grouped) batch -> caller's index, null: index0 + position.
// launch_compose_tiles: once per depth chunk over launch_render_boxes' layout (first: the call's first chunk, which initialises the whole frame);
// launch_compose_counts: once per call over the boxes of all n_poses <= PR_COMPOSE_MAX_POSES hypotheses, added into records[8 * caller's index]
// (pr_pose_visible words), which the caller zeroed; launch_compose_emit: labels / depth_out (either may be null) and frame[0..6] (pr_frame_explained
// words), zeroed by the caller.  window as for launch_contour_boxes
hipError_t launch_compose_tiles(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height, int4 window,
                                const uint32_t *index_of, uint32_t index0, unsigned long long *keys, bool first, hipStream_t s);
hipError_t launch_compose_counts(const unsigned long long *keys, const int4 *bbox, const uint32_t *index_of, uint32_t n_poses, uint32_t width, uint32_t height,
                                 const void *scene, bool scene_i32, int32_t tau, uint32_t *records, hipStream_t s);
hipError_t launch_compose_emit(const unsigned long long *keys, uint32_t width, uint32_t height, int4 window, const void *scene, bool scene_i32, int32_t tau,
                               uint16_t *labels, int32_t *depth_out, uint32_t *frame, hipStream_t s);
// pose_dist.hip: pr_pose_distance for pairs [pair0, pair0 + n_pairs) of a call.  as_rows: rows 0..2 of A_i S_k in double, [i * n_k + k][12];
// b_rows: rows 0..2 of B_j in float, [j][12]; pair p = (p / n_b, p % n_b) when all_pairs, else (p, p).  cam null: no projection (the variant
// without divisions).  The points are split over n_rows workgroup rows of chunks_per_row chunks of kPoseDistChunk points each (every row starts
// inside the range); partials: 16 bytes x n_rows x n_pairs x n_k.  The combine launch folds the rows and takes the three minima over k into records[n_pairs].
constexpr uint32_t kPoseDistChunk = PR_POSE_DIST_CHUNK;
struct PoseDistCamera { float fx, cx, fy, cy; };                  // K[0], K[2], K[4], K[5]
hipError_t launch_pose_dist(const pr_vec3 *points, uint32_t n_points, const double *as_rows, const float *b_rows, uint32_t n_b, uint32_t n_k,
                            uint32_t pair0, uint32_t n_pairs, bool all_pairs, const PoseDistCamera *cam, uint32_t n_rows, uint32_t chunks_per_row,
                            void *partials, hipStream_t s);
hipError_t launch_pose_dist_combine(const void *partials, uint32_t n_rows, uint32_t n_pairs, uint32_t n_k, uint32_t n_points, bool with_proj,
                                    pr_pose_dist *records, hipStream_t s);
// vsd.hip: pr_pose_vsd for the pairs of a rendered chunk (launch_render_boxes' layout).  Pair p compares hypothesis p * est_mul (the estimate) with
// hypothesis p * gt_mul + gt_add (the truth) of the chunk: {2, 2, 1} = estimates and truths interleaved, {1, 0, n} = every estimate against the one
// truth rendered behind them.  Added into records[16 * p] (pr_vsd_counts words), which the caller zeroed; entries of tau at and beyond n_taus are not read.
struct VsdPairing { uint32_t est_mul, gt_mul, gt_add; };
struct VsdParams { float delta; uint32_t n_taus; float tau[PR_VSD_MAX_TAUS]; uint32_t has_k; float fx, cx, fy, cy; };      // K[0], K[2], K[4], K[5]; has_k 0: ray factor 1
hipError_t launch_vsd_boxes(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_pairs, const VsdPairing &pairing, uint32_t width,
                            uint32_t height, const void *scene, bool scene_i32, const VsdParams &pm, uint32_t *records, hipStream_t s);
hipError_t launch_pack_export(const DevIcpState *st, pr_result *out, const uint32_t *counts, uint32_t *host_counts, pr_result *host_results,
                              uint32_t n, hipStream_t s);
hipError_t launch_stage_words(const void *src_host_mapped, void *dst, size_t bytes, hipStream_t s);
hipError_t launch_stage_words64(const void *src_host_mapped, void *dst, size_t bytes, hipStream_t s);
hipError_t launch_copy_words32(const void *src, void *dst, uint32_t n_words, hipStream_t s);   // either direction (pinned host memory through its device pointer)   // 8-byte words: exact for 72-byte records
// meta[i].start = exclusive scan of counts[0..i) rounded up to kCloudAlign points each (the packed layout of a batch's clouds)
hipError_t launch_d2c_pack_starts(const uint32_t *counts, uint32_t n, PoseMeta *meta, hipStream_t s);
hipError_t launch_emit_box(const int32_t *depth, uint32_t n_poses, uint32_t width, uint32_t height, const int4 *bbox, float fx, float fy,
                           float cx, float cy, const uint32_t *row_count, const uint32_t *row_off, pr_vec3 *cloud, const PoseMeta *meta,
                           hipStream_t s, const uint32_t *box_off = nullptr, bool bands = false);     // bands: as launch_render_boxes. cloud i starts at meta[i].start (packed: launch_render_boxes or launch_d2c_pack_starts wrote it)

// pyramid.hip (pr_refine_pyramid): the strided level clouds of the hypotheses of a chunk, from the depth boxes launch_render_boxes left.
// PyramidStrides: the levels' strides (unused entries 1).  PyramidCarry: what the emit of ONE level needs per hypothesis -- rows 0..2 of the transform
// accumulated over the levels before it and where its cloud starts (points, packed like d2c_pack_starts' layout) -- one 64-byte record, staged by the host.
struct PyramidStrides { uint32_t n; uint32_t s[PR_PYRAMID_MAX_LEVELS]; };
struct alignas(64) PyramidCarry { float T[12]; uint32_t start; uint32_t pad[3]; };
static_assert(sizeof(PyramidCarry) == 64, "PyramidCarry must stay one 64-byte record");
// row_count / row_off: [level][hypothesis][height] words each; counts[level * n_poses + hypothesis] = that level cloud's size.  The depth is read once.
hipError_t launch_pyramid_counts(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height,
                                 const PyramidStrides &lv, uint32_t *row_count, uint32_t *row_off, uint32_t *counts, hipStream_t s);
// one level: row_count / row_off are that level's [hypothesis][height] plane; apply: every point goes through its hypothesis' carry transform
hipError_t launch_pyramid_emit(const int32_t *depth, uint32_t n_poses, uint32_t width, uint32_t height, const int4 *bbox, const uint32_t *box_off,
                               float fx, float fy, float cx, float cy, uint32_t stride, const uint32_t *row_count, const uint32_t *row_off,
                               const PyramidCarry *carry, bool apply, pr_vec3 *cloud, hipStream_t s);

hipError_t launch_icp_pass_proj_aos(const IcpBatch &b, const SceneProjAoS &sc, uint32_t n_poses, hipStream_t s);
hipError_t launch_icp_pass_proj_packed(const IcpBatch &b, const SceneProjPacked &sc, uint32_t n_poses, hipStream_t s);
// every pass of the loop in one launch, one 1024-lane workgroup per hypothesis (icp_loop_cu_kernel: fused device solve, no robust weight); its dynamic
// LDS grows with b.nblk, and a batch whose plan needs more than the budget stays on the multi-launch loop
constexpr size_t kLoopCuLdsBudget = 64u << 10;
size_t icp_loop_cu_lds_bytes(uint32_t nblk);
// ... and behind rows and header the kernel keeps the first b.lds_blocks blocks of every cloud in LDS over the whole loop, up to the compute unit's
// 160 KiB (icp_loop_cu_lds_blocks: how many fit, at most nblk and at most `cap`, negative = no cap; 0 for a plan over the budget above).
// *lds_blocks_used receives the number the launch really ran with: 0 when the device refuses the LDS opt-in.
constexpr size_t kLoopCuLdsTotal = 160u << 10;
uint32_t icp_loop_cu_lds_blocks(uint32_t nblk, uint32_t steps, int cap);
// The full layout (options "loop_lds_tables", "loop_waves"): rows and header, the scene's colf / rowf tables (width + height floats), then whole
// blocks, within 160 KiB for a 16-wave workgroup and 80 KiB for an 8-wave one, of which two share a compute unit.  Returns the blocks, *fixed_bytes
// = rows + header + tables granted (a width and height of 0: no tables asked for).  Tables first, whole blocks after.
uint32_t icp_loop_cu_layout(uint32_t nblk, uint32_t steps, int cap, uint32_t width, uint32_t height, uint32_t waves, uint32_t *fixed_bytes);
struct LoopCuForm { uint32_t waves; int tables; };                  // wavefronts per workgroup (16 or 8); tables in LDS: 0 no, 1 yes, -1 the library's choice
struct LoopCuUsed { uint32_t lds_blocks, waves, table_bytes; };     // what the launch really ran with
hipError_t launch_icp_loop_cu_proj_packed(const IcpBatch &b, const SceneProjPacked &sc, uint32_t n_poses, hipStream_t s, LoopCuForm form, LoopCuUsed *used = nullptr);
// The in-pass kd-tree walks stage sc.lds_nodes leading nodes in dynamic LDS beside icp_pass_kernel's kPassStaticLds static bytes.  The stack
// walks stay within 64 KiB by nn_route's cap.  The stackless walks (plain and robust) may ask for up to kNNLdsNodesMax 16-byte entries:
// beyond kNNLdsNodesPlain the launcher opts the kernel in per device, and where the device refuses it stages kNNLdsNodesPlain and runs.
// *ran receives what was launched: the staged count (0 for compact records: nothing is staged beside their stacks) and the stack entries
// per lane (0 = stackless).
constexpr uint32_t kPassStaticLds = 4 * kAccStride * (uint32_t)sizeof(float);                 // wsum
constexpr uint32_t kNNLdsNodesMax = 8192;                                                     // 128 KiB
constexpr uint32_t kNNLdsNodesPlain = ((64u << 10) - kPassStaticLds) / 16u;                   // 4064: static + dynamic <= 64 KiB, no opt-in
struct NNPassRan { uint32_t lds_nodes, stack_depth; };
hipError_t launch_icp_pass_nn(const IcpBatch &b, const SceneNNDev &sc, uint32_t n_poses, hipStream_t s, NNPassRan *ran = nullptr);
// split form of the kd-tree pass: search (pending transform applied, winners written to b.nn_prev) + gather/accumulate pass
// marks (or null): three events recorded after the search, the bound and the walk kernel (timed batches; n_poses <= 32768)
hipError_t launch_nn_search(const IcpBatch &b, const SceneNNDev &sc, uint32_t n_poses, uint32_t max_points, uint32_t run, hipStream_t s, hipEvent_t *marks = nullptr);
hipError_t launch_icp_pass_nn_winners(const IcpBatch &b, const SceneNNWinners &sc, uint32_t n_poses, hipStream_t s);
// grid_scene.hip: the closest-point grid's pass, its build (cell_point: every cell written; `tree`: the scene's kd-tree as make_scene derives it) and its audit entry
hipError_t launch_icp_pass_grid(const IcpBatch &b, const SceneGridDev &sc, uint32_t n_poses, hipStream_t s);
hipError_t launch_grid_build(const SceneNNDev &tree, float reach, const SceneGridDev &grid, uint32_t *cell_point, hipStream_t s);
hipError_t launch_grid_records(const pr_vec3 *pcd, const pr_vec3 *normal, uint32_t n, float4 *rec, hipStream_t s);
hipError_t launch_contrib29_grid(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneGridDev &sc, float *out, hipStream_t s);
// audit entry (icp_debug.hip): the 29 terms of every point of one cloud, out[n][29]; update12 (rows 0..2 of a 4x4) or null is applied first
hipError_t launch_contrib29_proj_aos(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneProjAoS &sc, float *out, hipStream_t s);
hipError_t launch_contrib29_proj_packed(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneProjPacked &sc, float *out, hipStream_t s);
hipError_t launch_contrib29_nn(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneNNDev &sc, float *out, hipStream_t s);
// audit entry of the robust pass (pr_debug_robust_terms): the weighted terms of every point, out[n][29], and (ra.corr) its correspondence and weight
hipError_t launch_robust_terms_proj_aos(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneProjAoS &sc, const RobustArgs &ra, float *out, hipStream_t s);
hipError_t launch_robust_terms_proj_packed(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneProjPacked &sc, const RobustArgs &ra, float *out, hipStream_t s);
hipError_t launch_robust_terms_nn(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneNNDev &sc, const RobustArgs &ra, float *out, hipStream_t s);
hipError_t launch_robust_terms_grid(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneGridDev &sc, const RobustArgs &ra, float *out, hipStream_t s);
// one iteration of pose_iteration_wave per hypothesis on given sums (pr_debug_pose_iteration): one wavefront each
hipError_t launch_pose_iteration_debug(const float *sums, const uint32_t *n_points, uint32_t n, pr_criteria crit, uint32_t iter, pr_result *state,
                                       float *update, uint32_t *finished, hipStream_t s);
// *usable (one device word of its own, no part of NNInfo) = non-zero when every scene point owns a grid cell (the grid may be used), 0 otherwise
// grid: gw*gh cells followed by the three pyramid levels (nn_grid_cells(gw, gh) cells in all)
size_t nn_grid_cells(uint32_t gw, uint32_t gh);
hipError_t launch_build_nn_grid(const pr_vec3 *pcd, uint32_t n_points, uint32_t gw, uint32_t gh, float fx, float fy, float cx, float cy,
                                int32_t *cell_idx, float4 *grid, uint32_t *usable, hipStream_t s);
hipError_t launch_icp_finalize(const float *partial, const PoseMeta *meta, uint32_t nblk,
                               uint32_t steps, float *sums, uint32_t n_poses, hipStream_t s);
// PR_SOLVE_DEVICE: finalize + convergence test + 6x6 solve + state update in one kernel
hipError_t launch_icp_finalize_solve(const float *partial, PoseMeta *meta, uint32_t nblk,
                                     uint32_t steps, DevIcpState *st, pr_criteria crit, uint32_t iter,
                                     uint32_t n_poses, hipStream_t s);
hipError_t launch_pack_results(const DevIcpState *st, pr_result *out, uint32_t n_poses, hipStream_t s);

// kd_build.hip: the level-order build's workspace (one allocation, carved by kd_work_bytes) and its launches
struct KdLevelNode { int left, right, child, axis; float cut; int pad0, pad1, pad2; };   // a node of the level being split: position range, first child's id (-1: a leaf), axis, cut
struct KdCtrl { uint32_t lo, hi, next, done, levels, error, pad0, pad1; };               // nodes [lo, hi) = the level, their children [hi, next); levels = scatter passes done
struct KdWork {
    void *base = nullptr;
    KdCtrl *ctrl[2] = { nullptr, nullptr };                                            // by level parity: a level's launches read [level & 1], its plan writes the other
    int *idx[2] = { nullptr, nullptr }, *owner[2] = { nullptr, nullptr };                // permutation and each position's node (index within its level), double-buffered
    KdLevelNode *lv[2] = { nullptr, nullptr };
    unsigned long long *bbkeys = nullptr, *lrkeys = nullptr;
    uint32_t *left_total = nullptr, *tile_agg = nullptr, *chunk_cnt = nullptr;
    unsigned long long *root_part = nullptr;
    uint32_t max_level = 0;
};
size_t kd_work_bytes(uint32_t n, uint32_t cap, int max_leaf, KdWork *w);           // bytes needed; with w->base set, also fills in the pointers
hipError_t launch_kd_init(const KdWork &w, pr_kdnode *nodes, uint32_t cap, const pr_vec3 *pcd, uint32_t n, int max_leaf, hipStream_t s);
hipError_t launch_kd_level(const KdWork &w, pr_kdnode *nodes, uint32_t cap, const pr_vec3 *pcd, uint32_t n, int max_leaf, uint32_t level, hipStream_t s);
hipError_t launch_kd_permute(const KdWork &w, uint32_t levels_launched, const pr_vec3 *pcd, const pr_vec3 *nrm, uint32_t n, pr_vec3 *pcd_out, pr_vec3 *nrm_out, hipStream_t s);
template <typename T>
hipError_t launch_nn_gather(const T *depth, uint32_t W, uint32_t H, float fx, float fy, float cx, float cy, const pr_vec3 *normal_full,
                            uint32_t *row_count, uint32_t *row_off, uint32_t *count, pr_vec3 *pcd, pr_vec3 *nrm, bool emit, hipStream_t s);
template <typename T>
hipError_t launch_scene_proj_prepare(const T *depth, uint32_t W, uint32_t H, float fx, float fy, float cx, float cy, pr_vec3 *pcd, pr_vec3 *normal, hipStream_t s);
hipError_t launch_raw2depth_mask(const int32_t *raw, size_t n, uint16_t *depth16, uint8_t *mask8, hipStream_t s);
// The fingerprints a scene cache keeps of its source arrays, the same four words in both caches (NNInfo::fp, ProjTail::fp of pr_runtime.h).
// sample: 4096 words per array, taken at the build (launch_scene_fingerprint); every asynchronous batch compares it inside its raster launch
// (BatchCheck::fp_expected).  full: every word, taken at the build; call: the same of a synchronous call's cache hit (launch_scene_fingerprint_full),
// read back beside `full` (fingerprint_differs, pr_scene.cpp).
struct FpWords { uint32_t sample, reserved, full, call; };
static_assert(sizeof(FpWords) == 16 && offsetof(FpWords, call) == offsetof(FpWords, full) + 4, "FpWords: four words, full and call side by side");
hipError_t launch_scene_fingerprint(const SceneSources &src, uint32_t *sample, hipStream_t s);
hipError_t launch_scene_fingerprint_full(const SceneSources &src, uint32_t *sum, hipStream_t s);
hipError_t launch_pack_proj_scene(const pr_vec3 *pcd, const pr_vec3 *normal, float4 *rec, size_t n, float *colf, float *rowf,
                                  uint32_t width, uint32_t height, float fx, float fy, float cx, float cy, uint32_t tl_x, uint32_t tl_y,
                                  uint32_t *exact, hipStream_t s);
// The 24 control words of a set of kd-tree records: written by nn_build.hip's kernels, read back whole by the host (NNDerived::info), handed
// out as 24 words by pr_debug_nn_records -- the positions are part of that interface.  Floats are kept as bit patterns.
enum : uint32_t { kWideNone = 0, kWideValid = 1, kWideMoreLevels = 2 };     // NNInfo::wide_state; more levels: the tree has more wide levels than were launched
struct NNInfo {
    uint32_t depth;             // [0] longest root-to-node path; >= 0x7fffffff: the links are inconsistent (nn_records_kernel)
    uint32_t rec32_valid;       // [1] 1: the 32-byte records express the tree
    uint32_t qmin[3], qscale[3];   // [2..7] their frame
    uint32_t wide_state;        // [8] kWideNone / kWideValid / kWideMoreLevels
    uint32_t n_wide;            // [9] wide nodes
    uint32_t reserved0[2];
    FpWords fp;                 // [12..15]
    uint32_t wmin[3], wscale;   // [16..19] frame of the wide records
    uint32_t wide_frame_ok;     // [20] 1: a unit of that frame is at least one ulp of the largest coordinate -- the wide walk may run (nn_frame_kernel)
    uint32_t reserved1[3];
};
static_assert(sizeof(NNInfo) == 96 && offsetof(NNInfo, depth) == 0 && offsetof(NNInfo, rec32_valid) == 4 && offsetof(NNInfo, qmin) == 8 &&
              offsetof(NNInfo, qscale) == 20 && offsetof(NNInfo, wide_state) == 32 && offsetof(NNInfo, n_wide) == 36 && offsetof(NNInfo, fp) == 48 &&
              offsetof(NNInfo, wmin) == 64 && offsetof(NNInfo, wscale) == 76 && offsetof(NNInfo, wide_frame_ok) == 80, "NNInfo: the documented word positions");
// wide: nn_wide_capacity(n_nodes) lines of 128 bytes, scratch: nn_wide_scratch_words(n_nodes) words
inline size_t nn_wide_capacity(uint32_t n_nodes) { return (size_t)n_nodes / 2 + 2; }
inline size_t nn_wide_scratch_words(uint32_t n_nodes) { const size_t cap = nn_wide_capacity(n_nodes); return 2 * cap + 4 + 2 * (cap / 1024 + 4) + 4 + 8; }   // wq, cnt, chunk sums x 2, flag, control records x 2
hipError_t launch_build_nn_accel(const pr_kdnode *nodes, uint32_t n_nodes, const pr_vec3 *pcd, uint32_t n_points,
                                 int4 *topo, float4 *bmin, float4 *bmax, float4 *pts, float4 *rec, uint4 *rec32, uint2 *desc, NNInfo *info, hipStream_t s,
                                 float wide_margin = 0.0f);   // clears *info first; wide_margin: how far beyond the root box the wide records' frame reaches (the acceptance radius)
hipError_t launch_nn_wide_levels(const int4 *topo, const float4 *bmin, const float4 *bmax, uint32_t n_nodes, uint32_t n_points, uint4 *wide, uint32_t *scratch,
                                 NNInfo *info, uint32_t first, uint32_t count, hipStream_t s);

}  // namespace prk

// ---- host-side math shared by the C ABI (pr_host.cpp) ------------------------------------------
namespace prh {
void solve_666(const float A[36], const float b[6], float T[16]);
void mat4_mul(const float A[16], const float B[16], float C[16]);
// Spatial order of a triangle soup (pr_debug_mesh_order): perm[k] = index of the triangle that goes to place k.  A pure function of the data.
void mesh_order(const pr_triangle *tris, size_t n_tris, uint32_t *perm);
// The distinct vertices of a triangle soup as {x, y, z, 0}, distinct by bit pattern, in ascending order of the words (z, y, x as unsigned): what
// pose_tight_box_kernel walks.  A pure function of the data.
void mesh_vertices(const pr_triangle *tris, size_t n_tris, std::vector<float4> &out);
// multiset fingerprint of a triangle buffer: wrapping sum of triangle_hash (pose_box.h)
unsigned long long mesh_fingerprint(const pr_triangle *tris, size_t n_tris);
// the cover rule's own conditions (pr_score_cover, pr_select_cover_host): the fraction, and order a list of distinct indices < n_poses.  PR_ERR_INVALID with a message
void set_error(const char *fmt, ...);   // pr_context.cpp
inline int cover_rule_ok(const char *fn, const uint32_t *order, uint32_t n_order, uint32_t n_poses, uint32_t new_num, uint32_t new_den)
{
    if (new_den == 0) { set_error("%s: new_den must not be 0", fn); return PR_ERR_INVALID; }
    if (new_num > new_den) { set_error("%s: new_num / new_den must not exceed 1 (got %u / %u)", fn, new_num, new_den); return PR_ERR_INVALID; }
    if (n_order && !order) { set_error("%s: bad arguments (order is null)", fn); return PR_ERR_INVALID; }
    std::vector<unsigned char> seen(n_poses, 0);
    for (uint32_t k = 0; k < n_order; ++k) {
        if (order[k] >= n_poses) { set_error("%s: order[%u] = %u, but there are %u hypotheses", fn, k, order[k], n_poses); return PR_ERR_INVALID; }
        if (seen[order[k]]) { set_error("%s: order[%u] = %u appears twice", fn, k, order[k]); return PR_ERR_INVALID; }
        seen[order[k]] = 1;
    }
    return PR_OK;
}
}
