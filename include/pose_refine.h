/*
 * pose_refine.h -- C ABI of the MI355X-native render -> cloud -> point-to-plane ICP hot path.
 *
 * This is the drop-in boundary.  The reference (meiqua/pose_refine) has no FFI layer: its boundary
 * is the C++ header API (cuda_renderer/renderer.h, cuda_icp/icp.h, cuda_icp/scene/...).  The C++
 * adapter headers in include/cuda_renderer and include/cuda_icp keep that API source-compatible
 * and forward every device-side entry point to the functions below.  Each function cites the
 * reference interface it replaces (paths relative to the reference root).
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  "dev" pointers are device (HBM)
 * pointers obtained from pr_malloc (or any hipMalloc'd memory of the current device); everything
 * else is host memory.  All functions return PR_OK (0) or a negative error code; the message of
 * the last failure on the calling thread is available from pr_last_error().  There is NO CPU
 * fallback: every device entry point fails with PR_ERR_NO_DEVICE when no gfx950 device is usable.
 * Work is issued on one library-owned HIP stream per context; calls are synchronous with respect to the host unless
 * stated otherwise.
 *
 * Contexts and threads.  There is one shared context per device, created by pr_init(device) (or on first use: device 0).
 * A host thread works on the context it last selected with pr_init / pr_set_device; threads that never selected one use the
 * device of the process' first pr_init.  Calls on one context are serialised (a mutex per context); contexts of different
 * devices run side by side, which is how a C++ host drives N GPUs: one thread per device, pr_set_device(d) first.  Threads
 * that each refine their own hypotheses on the SAME device (the reference's usage, README.md:15 / icp.cu:170 per-thread
 * streams) call pr_thread_context(1) once to get a private context (own stream and workspaces) instead of queueing on the
 * shared one (once per thread, for the thread's life: the runtime hands out hardware queues in the order streams are created, and a
 * process that keeps creating and releasing contexts ends up with streams that share a queue -- two host-solve threads 235 k poses/s on
 * fresh contexts, 154 k on the twelfth pair).  Options (pr_set_option) are process-wide.
 *
 * Caches and caller-owned memory.  Derived data is cached by the address of the buffers it was derived from: the packed copy
 * of a projective scene (pcd / normal arrays), the traversal records of a kd-tree scene (pcd / nodes arrays) and the model box
 * of a triangle buffer together with a copy of the buffer in spatial order that the asynchronous path rasterises (option "mesh_order").
 * Both are re-verified on the device by every batch that uses them -- the box, and an order-independent fingerprint of every word of the
 * caller's buffer -- so a rewritten mesh is never rendered from stale data: its first batch is repeated from the caller's buffer (pr_stats).
 * The scene caches are dropped by every write that goes through this library (pr_memcpy_*,
 * pr_fill_i32, pr_free, pr_render, the *_prepare_dev / *_build_dev / *_crop_dev functions); a caller that rewrites a scene
 * array by other means (its own kernels, raw hipMemcpy) MUST announce it with pr_invalidate(ptr, bytes) before the next ICP /
 * refine call, or switch the caches off with pr_set_option("scene_cache", 0).
 * Behind that (round 6): every SYNCHRONOUS call that finds a cached form (pr_icp_*, pr_refine_batch*: what the C++ adapters of the reference's API
 * reach) compares a fingerprint of EVERY word of the scene arrays with the one taken when the cache was built (~20 us) and rebuilds on a mismatch --
 * an in-place edit through any pointer is seen without pr_invalidate, as with the reference, which reads the arrays at every call
 * (depth_scene.h:29-48).  Asynchronous batches (pr_refine_submit) compare a SAMPLE of 4096 words per array inside their raster launch (a mismatch
 * repeats the batch with fresh caches, pr_stats): a frame replaced as a whole is noticed, an edit confined to words the sample does not look at
 * needs pr_invalidate.  A write THROUGH this library into a range that a batch still in flight on the calling context reads (its scene arrays, its
 * mesh, its result block) waits for that batch first: a scene object may be re-initialised while its previous frame's batch is running.  The outputs
 * of the frame stages (pr_depth_fuse_dev, pr_depth_filter_dev, pr_depth_reproject_dev, pr_scene_planes_dev, pr_scene_segments_dev,
 * pr_segment_depth_dev, the pr_ppf_* samplers, tables and accumulators) are ordered like every other write through the library: a stage whose
 * output overlaps such a range waits for the batch before its first kernel that writes is launched.
 */
#ifndef POSE_REFINE_H
#define POSE_REFINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PR_OK                 0
#define PR_ERR_NO_DEVICE     -1
#define PR_ERR_HIP           -2
#define PR_ERR_INVALID       -3
#define PR_ERR_IO            -4
#define PR_ERR_NOMEM         -5
#define PR_ERR_COMM          -6     /* RCCL: library not loadable, communicator missing, or a collective failed */

/* ---- POD mirrors of the reference types (layouts verified by static_assert in the adapters) -- */
typedef struct { float x, y, z; } pr_vec3;                         /* ::Vec3f geometry.h:83-103; Model::float3 renderer.h:50-57 (12 B) */
typedef struct { pr_vec3 v0, v1, v2; } pr_triangle;                /* Model::Triangle renderer.h:58-68 (36 B)                          */
typedef struct { float m[16]; } pr_mat4;                           /* Model::mat4x4 renderer.h:69-141 = ::Mat4x4f, row-major (64 B)    */
typedef struct { int x, y, width, height; } pr_roi;                /* Model::ROI renderer.h:43-48                                      */
typedef struct {                                                   /* ::Node_kdtree pcd_scene.h:5-25 (52 B)                            */
    int parent, child1, child2;
    float split_v;
    float bbox[6];
    int split_dim;
    int left, right;
} pr_kdnode;
typedef struct { float T[16]; float inlier_rmse; float fitness; } pr_result;        /* cuda_icp::RegistrationResult icp.h:26-36 (72 B) */
typedef struct { float relative_fitness, relative_rmse; int max_iteration; } pr_criteria; /* cuda_icp::ICPConvergenceCriteria icp.h:38-50 */

/* Scene_projective (depth_scene.h:7-48): non-owning view, passed by value like the reference does. */
typedef struct {
    uint64_t width, height;
    float max_dist_diff;
    float K[9];
    const pr_vec3 *pcd;        /* dev, width*height, (0,0,0) where depth==0 */
    const pr_vec3 *normal;     /* dev, width*height */
} pr_scene_proj;

/* Scene_nn (pcd_scene.h:48-137): non-owning view of a KDTree_cuda (pcd_scene.h:38-45). */
typedef struct {
    float max_dist_diff;
    const pr_vec3 *pcd;        /* dev, n_points, in tree order */
    const pr_vec3 *normal;     /* dev, n_points */
    const pr_kdnode *nodes;    /* dev, n_nodes, level order, nodes[0] = root */
    uint32_t n_points, n_nodes;
    /* Optional (not in the reference's struct, which drops K after init_Scene_nn_*): the camera of the depth image the scene was made
     * from -- cam_w = 0: unknown.  With it a bare ICP call (no render, hence no camera of its own) can index the scene points by pixel as
     * the fused path does; it is a HINT: the pixel grid is only used if every scene point really projects into a cell of its own. */
    float cam_fx, cam_fy, cam_cx, cam_cy;
    uint32_t cam_w, cam_h;
    /* The hint is read only when cam_magic == PR_SCENE_NN_CAM_MAGIC: a caller that fills the reference's six members field by field and
     * leaves the rest of the struct uninitialised (or zero) never triggers a grid build from garbage.  The struct has grown since round 2
     * (it ends here; sizeof == 72): callers must be compiled against this header -- PR_ABI_VERSION / pr_abi_version() tell them apart. */
    uint32_t cam_magic;
} pr_scene_nn;
#define PR_SCENE_NN_CAM_MAGIC 0x4d414350u   /* 'PCAM' */
#define PR_ABI_VERSION 4                    /* bumped whenever a struct of this header changes size or layout */

/* A Scene_projective whose arrays cover only a window of the frame: pcd2dep(src, K, tl_x, tl_y) / dep2pcd(x, y, d, K, tl_x, tl_y)
 * (common.h:47-73) with the offsets the reference declares but never passes.  view.width / view.height are
 * the window's size, pixel (x, y) of the arrays is frame pixel (x + tl_x, y + tl_y). */
typedef struct {
    pr_scene_proj view;
    uint32_t tl_x, tl_y;
} pr_scene_proj_crop;

#define PR_SCENE_PROJ      0
#define PR_SCENE_NN        1
#define PR_SCENE_PROJ_CROP 2      /* scene argument is a pr_scene_proj_crop */
#define PR_SCENE_GRID      3      /* scene argument is a pr_scene_grid */

/* Closest-point grid (no counterpart in the reference): a voxel field over the scene's volume whose every cell holds the index of the scene
 * point nearest to the cell's CENTRE -- built once per frame with the exact kd-tree search, after which a nearest-neighbour query of the ICP
 * is arithmetic, one 4-byte gather and one record gather.  All arithmetic below is float32 without contraction.
 *   cell of a point p, per axis a:  f = (p[a] - origin[a]) * inv_cell;  inside iff f >= 0.0f && f < (float)dim[a] (NaN, +-inf fail);
 *                                   i[a] = (int)f;  index = i[0] + dim[0] * (i[1] + dim[1] * i[2])
 *   centre of a cell:               origin[a] + ((float)i[a] + 0.5f) * cell
 *   build:  cell_point[index] = a k that minimises ((dx*dx + dy*dy) + dz*dz) between the centre and pcd[k] (pcd_scene.h:87-90; any k of a tie;
 *           the same inputs give the same bytes), or PR_GRID_NONE unless that minimum is < reach * reach
 *   query:  a point outside the grid or in a PR_GRID_NONE cell has no correspondence; else w = cell_point[index], (d, n) = rec[w], valid iff
 *           ((ex*ex + ey*ey) + ez*ez) < max_dist_diff * max_dist_diff with e = d - p; it then contributes like any other scene's correspondence
 *   bound:  with h = (sqrt(3) / 2) * cell, the point returned for a query inside the grid is at most 2 h farther away than the true nearest
 *           one, provided the centre's nearest point was within reach; with reach >= max_dist_diff + h no query with a true neighbour within
 *           max_dist_diff - h lands in a PR_GRID_NONE cell */
#define PR_GRID_NONE         0xFFFFFFFFu
#define PR_GRID_MAX_CELLS    (1u << 26)          /* 256 MB of indices */
typedef struct {
    float    origin[3];      /* corner of cell (0,0,0), metres, camera frame */
    float    cell;           /* edge length, > 0, finite */
    float    inv_cell;       /* 1.0f / cell, computed ONCE by pr_scene_grid_describe in float32; device and references read it, never recompute it */
    uint32_t dim[3];         /* each >= 1, product <= PR_GRID_MAX_CELLS */
    float    max_dist_diff;  /* acceptance radius of a correspondence, as Scene_nn (pcd_scene.h:127) */
    float    reach;          /* a cell whose centre is not nearer than this to any scene point holds PR_GRID_NONE */
    uint32_t n_points;
    const uint32_t *cell_point;   /* dev, dim[0]*dim[1]*dim[2], x fastest */
    const float    *rec;          /* dev, n_points * 8 floats: {px,py,pz,0, nx,ny,nz,0}, written by the build */
} pr_scene_grid;

/* where the 6x6 solve of every ICP iteration runs (icp.cu:207 does it on the host) */
#define PR_SOLVE_HOST   0
#define PR_SOLVE_DEVICE 1

/* ---- library / device ------------------------------------------------------------------------ */
const char *pr_last_error(void);
const char *pr_version(void);
int pr_abi_version(void);                        /* PR_ABI_VERSION the library was built with: compare with the header a caller was compiled against */
int pr_device_count(void);                       /* number of visible HIP devices (0 if none)              */
int pr_init(int device);                         /* bind the calling thread to the device's shared context, create its stream (test.cpp:12-20 warm-up) */
int pr_set_device(int device);                   /* same (cudaSetDevice, which test.cpp:14 leaves commented out)                 */
int pr_thread_context(int enable);               /* 1: private context for the calling thread on its current device; 0: release it */
int pr_shutdown(void);                           /* release the calling thread's context: workspaces, streams, communicator    */
int pr_sync(void);                               /* wait for the context's stream                                               */

/* device_vector_holder<T> storage: common.cu:3-40, renderer.cu:15-50 */
int pr_malloc(void **dev_ptr, size_t bytes);
int pr_free(void *dev_ptr);                     /* waits for what every context of the device has in flight (the caller's and, one at a time, the others') before the memory goes */
int pr_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes);
int pr_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes);
int pr_memcpy_d2d(void *dev_dst, const void *dev_src, size_t bytes);
int pr_fill_i32(int32_t *dev_dst, size_t count, int32_t value);   /* holder(size, init) fill ctor */
/* [dev_ptr, dev_ptr + bytes) was written behind the library's back (bytes = 0: the whole allocation) -- see "Caches" above */
int pr_invalidate(const void *dev_ptr, size_t bytes);

/* ---- host-side model / scene preparation (CPU in the reference too) --------------------------- */
/* Model::Model(fileName) / LoadModel renderer.cpp:11-104 + get_bounding_box :106-150.  The reference imports through assimp; here:
 * PLY (ASCII, binary little / big endian, typed properties) and Wavefront OBJ (single mesh, identity node transform), and glTF 2.0
 * (.gltf with external or base64 buffers, .glb) with its node hierarchy walked like recursive_render (renderer.cpp:69-104): node
 * transforms multiplied down the tree, one mesh per primitive, triangles transformed, vertices_out untransformed and faces_out
 * per-mesh indices exactly as the reference keeps them, the box over the TRANSFORMED vertices (get_bounding_box_for_node).
 * Faces with < 3 indices are dropped (renderer.cpp:78), polygons / strips / fans become triangles (assimp's aiProcess_Triangulate).
 * Any output pointer may be NULL; faces_out receives 3 vertex indices per triangle (Model::faces), vertices_out the file's vertex
 * list (Model::vertices), bbox_min / bbox_max the component-wise extremes of the vertices (Model::bbox_min / bbox_max). */
int pr_mesh_count(const char *path, size_t *n_triangles, size_t *n_vertices);
int pr_mesh_load(const char *path, pr_triangle *tris_out, size_t cap_triangles, size_t *n_triangles,
                 pr_vec3 *vertices_out, size_t cap_vertices, size_t *n_vertices, int32_t *faces_out,
                 float bbox_min[3], float bbox_max[3]);
/* triangles only (the hot path consumes nothing else) */
int pr_ply_count(const char *path, size_t *n_triangles, size_t *n_vertices);
int pr_ply_load(const char *path, pr_triangle *tris_out, size_t cap_triangles, size_t *n_triangles);
/* compute_proj renderer.cpp:161-185 */
void pr_compute_proj(const float K[9], int width, int height, float near_, float far_, pr_mat4 *proj_out);
/* get_normal common.cpp:17-107 (depth already uint16, mm) */
int pr_get_normal(const uint16_t *depth16, int width, int height, const float K[9], pr_vec3 *normals_out);
/* init_Scene_projective_cpu depth_scene.cpp:3-35: fills width*height pcd + normal host buffers */
int pr_scene_proj_prepare(const void *depth, int depth_is_i32, const float K[9], size_t width, size_t height,
                          pr_vec3 *pcd_out, pr_vec3 *normal_out);
/* SURVEY 8f rank 1 -- the same preparation entirely on the device (the reference's init_Scene_projective_cuda still runs it
 * on the CPU, depth_scene.cu:8, and its README names that as the remaining bottleneck): depth_dev -> pcd_dev, normal_dev.
 * Bit-identical to pr_scene_proj_prepare. */
int pr_scene_proj_prepare_dev(const void *depth_dev, int depth_is_i32, const float K[9], size_t width, size_t height,
                              pr_vec3 *pcd_dev_out, pr_vec3 *normal_dev_out);
/* A window of a prepared full-frame scene as arrays of its own (rows of `window`, window.width * window.height entries each) */
int pr_scene_proj_crop_dev(const pr_vec3 *pcd_full_dev, const pr_vec3 *normal_full_dev, size_t width, size_t height, pr_roi window,
                           pr_vec3 *pcd_out_dev, pr_vec3 *normal_out_dev);
/* init_Scene_nn_cpu pcd_scene.cpp:4-37 + KDTree_cpu::build_tree pcd_scene.cpp:45-184.
 * pcd_out/normal_out need width*height entries, nodes_out 2*width*height+1 entries (worst case). */
int pr_scene_nn_prepare(const void *depth, int depth_is_i32, const float K[9], int width, int height,
                        int max_leaf, pr_vec3 *pcd_out, pr_vec3 *normal_out, pr_kdnode *nodes_out,
                        size_t cap_nodes, uint32_t *n_points, uint32_t *n_nodes);
/* KDTree_cpu::build_tree on caller-provided points (reorders pcd/normal in place) */
int pr_kdtree_build(pr_vec3 *pcd, pr_vec3 *normal, size_t n_points, int max_leaf,
                    pr_kdnode *nodes_out, size_t cap_nodes, uint32_t *n_nodes);
/* SURVEY 8f rank 1 -- the same two functions on the device (bit-identical nodes, point order and normals): the level-order
 * build runs one workgroup per node and level (block scans reproduce the stable two-ended partition and its tie rule).
 * pcd/normal/nodes are device buffers sized like their host counterparts above. */
int pr_kdtree_build_dev(pr_vec3 *pcd_dev, pr_vec3 *normal_dev, size_t n_points, int max_leaf,
                        pr_kdnode *nodes_dev_out, size_t cap_nodes, uint32_t *n_nodes);
int pr_scene_nn_prepare_dev(const void *depth_dev, int depth_is_i32, const float K[9], int width, int height, int max_leaf,
                            pr_vec3 *pcd_dev_out, pr_vec3 *normal_dev_out, pr_kdnode *nodes_dev_out, size_t cap_nodes,
                            uint32_t *n_points, uint32_t *n_nodes);
/* Closest-point grid over the box [lo, hi]: origin = lo, dim[a] = the cells of edge `cell` needed to cover hi[a] - lo[a] (at least 1), inv_cell,
 * the two radii; the pointers and n_points are left null / 0 for the build.  Pure host code.  PR_ERR_INVALID: a cell, radius or corner that is
 * not finite (cell, radii: not positive), hi < lo on an axis, a dim beyond 32 bits or more than PR_GRID_MAX_CELLS cells. */
int pr_scene_grid_describe(const float lo[3], const float hi[3], float cell, float max_dist_diff, float reach, pr_scene_grid *out);
/* The build: cell_point_dev (dim[0]*dim[1]*dim[2] words) from the exact search of `scene`'s kd-tree, rec_dev (8 floats per scene point) from its
 * points and normals; sets grid->cell_point, grid->rec and grid->n_points.  The buffers are the caller's and nothing derived from them is
 * cached by address: a grid rebuilt in place needs no pr_invalidate. */
int pr_scene_grid_build_dev(const pr_scene_nn *scene, pr_scene_grid *grid, uint32_t *cell_point_dev, float *rec_dev);
/* eigen_slover_666 icp.cpp:29-45 (public in icp.h:54) */
void pr_solve_666(const float A[36], const float b[6], pr_mat4 *T_out);
/* Mat4x4f * Mat4x4f geometry.h:292-298 (entries summed over k = 3,2,1,0): what `result.transformation_ = extrinsic * result.transformation_`
 * (icp.cu:212) evaluates; C_out may alias A or B */
void pr_mat4_mul(const pr_mat4 *A, const pr_mat4 *B, pr_mat4 *C_out);

/* ---- renderer (cuda_renderer/renderer.cu) ------------------------------------------------------ */
/* render_cuda_keep_in_gpu renderer.cu:269-336: depth_dev_out[n_poses*rw*rh] int32 mm, 0 = empty.
 * tris_dev: device triangles (the device_vector_holder<Triangle> overloads); poses on the host. */
int pr_render(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, size_t n_poses,
              size_t width, size_t height, const pr_mat4 *proj, pr_roi roi, int32_t *depth_dev_out);
/* render_cuda renderer.cu:189-267: same, result copied to the host */
int pr_render_to_host(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, size_t n_poses,
                      size_t width, size_t height, const pr_mat4 *proj, pr_roi roi, int32_t *depth_host_out);

/* raw2depth_uint16_cuda / raw2mask_uint8_cuda / raw2depth_mask_cuda renderer.cu:338-439: the int32 depth stack of a render ->
 * uint16 depth (uint16_t(x)) and/or uint8 mask (x>0 ? 255 : 0) on the host; either output may be NULL. */
int pr_raw2depth_mask(const int32_t *raw_dev, size_t count, uint16_t *depth_host_out, uint8_t *mask_host_out);

/* ---- depth -> cloud (cuda_icp/icp.cu:228-291 depth2cloud_cuda<T>) ------------------------------ */
/* Allocates *cloud_dev_out (release with pr_free); points in row-major pixel order, metres. */
int pr_depth2cloud_i32(const int32_t *depth_dev, uint32_t width, uint32_t height, const float K[9],
                       uint32_t stride, uint32_t tl_x, uint32_t tl_y, pr_vec3 **cloud_dev_out, uint32_t *n_points);
int pr_depth2cloud_u16(const uint16_t *depth_dev, uint32_t width, uint32_t height, const float K[9],
                       uint32_t stride, uint32_t tl_x, uint32_t tl_y, pr_vec3 **cloud_dev_out, uint32_t *n_points);

/* ---- ICP (cuda_icp/icp.cu:156-223 ICP_Point2Plane_cuda<Scene>) --------------------------------- */
/* One cloud: mutates cloud_dev in place exactly like the reference. */
int pr_icp_proj(pr_vec3 *cloud_dev, uint32_t n_points, const pr_scene_proj *scene, pr_criteria crit, pr_result *result_out);
int pr_icp_nn(pr_vec3 *cloud_dev, uint32_t n_points, const pr_scene_nn *scene, pr_criteria crit, pr_result *result_out);
int pr_icp_grid(pr_vec3 *cloud_dev, uint32_t n_points, const pr_scene_grid *scene, pr_criteria crit, pr_result *result_out);
/* Many clouds against one scene in one launch per iteration (what the reference needs P host
 * threads + cudaStreamPerThread for, README.md:15): cloud i = clouds_dev[offsets[i] .. offsets[i+1]). */
int pr_icp_batch(pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind,
                 const void *scene, pr_criteria crit, pr_result *results_host);

/* ---- robust ICP: an M-estimator weight on the point-to-plane residual (no counterpart in the reference) ----------------------------------
 * The plain pass counts a correspondence fully (e^2 < max_dist_diff^2) or not at all.  A robust pass multiplies the terms of the normal
 * system (sums 0..26) of every VALID correspondence by a weight w(r) of its residual; which correspondence a point gets and whether it is
 * valid are exactly what they are in the plain pass -- the weight never changes association or acceptance.
 *   c       the scale, in metres (the unit of the clouds);  inv_c = 1.0f / c, computed ONCE in float32 by pr_robust_describe: the device and
 *           the references read it and never recompute it (the precedent: pr_scene_grid.inv_cell).  reserved is 0.
 *   r       the float32 residual as the pass forms it, (ex*nx + ey*ny) + ez*nz with e = d - p;  J[0..5] = (p x n, n) as in the plain pass.
 *   w       float32, every operation rounded on its own (no contraction):
 *             PR_ROBUST_NONE    w = 1.0f
 *             PR_ROBUST_HUBER   a = fabsf(r);  w = (a <= c) ? 1.0f : c / a                     (correctly rounded IEEE division)
 *             PR_ROBUST_TUKEY   u = r * inv_c; q = u * u;  w = (q < 1.0f) ? (1.0f - q) * (1.0f - q) : 0.0f
 *             PR_ROBUST_CAUCHY  u = r * inv_c; q = u * u;  w = 1.0f / (1.0f + q)
 *   terms   seven values are formed once per point: wJ[a] = w * J[a], a = 0..5, and wr = w * r.  Each of the 27 products takes exactly one
 *           of them as one factor -- THE FACTOR TABLE (tests/robust_ref.py: WEIGHTED_FACTOR reads the same 27 entries):
 *             sums  0..20  J[a]*J[b], a <= b, row-major:   wJ[a] * J[b]      (the weight rides on the factor with the LOWER index)
 *             sums 21..23  J[a]*r, a = 0, 1, 2:            wJ[a] * r         (the weight rides on J[a])
 *             sums 24..26  J[a]*r, a = 3, 4, 5:            J[a]  * wr        (the weight rides on r)
 *           (the pairs the packed kernel multiplies -- (J0, J1), (J2, r), (J3, J4), (J5, dz) -- times (w, w) are four packed multiplies; with
 *           this table every one of the sixteen packed accumulations reads its operands from those pairs without a register move.)
 *   sums 27 (e^2) and 28 (count) are NOT weighted: fitness, inlier_rmse and the convergence test (icp.cu:178-212) keep their meaning and
 *           stay comparable with plain runs; a Tukey correspondence with w == 0 still counts as an inlier.
 * Each term is added to the lane's running sum exactly as in the plain pass: same canonical tree, same points_per_block semantics, same
 * solve.  When w == 1.0f every weighted product equals the plain product bit for bit, so any kind with a scale so large that w rounds to 1
 * (c = 1.0e6f) returns the bytes of the plain call.  The last pass of a device-solve run forms sums 27 and 28 only and needs no weight.
 * kd-tree scenes: a robust call always takes the split route (search kernels, then the pass over the winners) whenever the scene has compact
 * records, whatever the nn_* options say; results do not depend on those options, as they do not depend on them in plain calls.
 * pr_robust_describe: host only, needs no device.  PR_ERR_INVALID for a null `out`, an unknown kind and -- for a kind other than
 * PR_ROBUST_NONE -- a c that is not finite or not positive (or whose 1.0f / c is not a positive finite float). */
#define PR_ROBUST_NONE   0
#define PR_ROBUST_HUBER  1
#define PR_ROBUST_TUKEY  2
#define PR_ROBUST_CAUCHY 3
typedef struct { uint32_t kind; float c; float inv_c; uint32_t reserved; } pr_robust;   /* 16 B */
int pr_robust_describe(uint32_t kind, float c, pr_robust *out);
/* pr_icp_batch with the weight of `robust` (one descriptor for the call; all four scene kinds).  It takes an armed pr_debug_trace_sums
 * recorder exactly as pr_icp_batch does.  PR_ERR_INVALID, before any device is touched and with nothing written, for a null robust, a
 * descriptor pr_robust_describe would not have produced (unknown kind, bad c, inv_c != 1.0f / c, reserved != 0) and pr_icp_batch's own
 * argument errors.  PR_ROBUST_NONE returns pr_icp_batch's bytes. */
int pr_icp_batch_robust(pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind,
                        const void *scene, pr_criteria crit, const pr_robust *robust, pr_result *results_host);

/* ---- fused hypothesis refinement: render -> cloud -> ICP for n_poses hypotheses --------------- */
/* test.cpp:143-172 for a whole batch, everything resident on the device; results on the host.
 * cloud_sizes_host (optional) receives the model-cloud size of every hypothesis.  The synchronous calls (pr_refine_batch, _dev, _roi) run on
 * whichever asynchronous slot of the context holds no unfinished batch; with both slots pending they return PR_ERR_INVALID. */
int pr_refine_batch(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                    uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9],
                    int scene_kind, const void *scene, pr_criteria crit,
                    pr_result *results_host, uint32_t *cloud_sizes_host);
/* same, results left on the device (for the RCCL gather of the sharded job): results_dev[n_poses] */
int pr_refine_batch_dev(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                        uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9],
                        int scene_kind, const void *scene, pr_criteria crit,
                        pr_result *results_dev, uint32_t *cloud_sizes_host);

/* The same with the hypotheses rendered only inside `roi` (renderer.h:199 ROI {x, y, width, height} in image rows, renderer.cu:106-113)
 * and the clouds extracted with tl_x = roi.x, tl_y = roi.y (icp.h:57-60): clouds hold the rendered pixels inside the window, with
 * the coordinates they have in the full frame.  roi.width / roi.height <= 0 means no ROI. */
int pr_refine_batch_roi(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                        uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9],
                        int scene_kind, const void *scene, pr_criteria crit, pr_roi roi,
                        pr_result *results_host, uint32_t *cloud_sizes_host);

/* Asynchronous form of the two calls above (no counterpart in the reference, whose ICP() blocks): pr_refine_submit
 * enqueues one batch on `slot` (0 or 1) and returns; pr_refine_wait(slot) blocks until that batch is finished and
 * fills results_host / cloud_sizes_host (results_dev is complete at that point as well).  Exactly one of results_host /
 * results_dev may be NULL.  poses_host is copied before the call returns; tris_dev, the scene arrays and every output
 * pointer must stay valid until the wait.  Two slots let a host enqueue batch k+1 while batch k runs.  Batches the
 * asynchronous path does not cover (host solve, instrumented and timed calls) run to completion inside pr_refine_submit. */
int pr_refine_submit(int slot, const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                     uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9],
                     int scene_kind, const void *scene, pr_criteria crit,
                     pr_result *results_host, pr_result *results_dev, uint32_t *cloud_sizes_host);
int pr_refine_submit_roi(int slot, const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                         uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9],
                         int scene_kind, const void *scene, pr_criteria crit, pr_roi roi,
                         pr_result *results_host, pr_result *results_dev, uint32_t *cloud_sizes_host);
int pr_refine_wait(int slot);

/* ---- verification: render-and-compare scoring of hypotheses against the scene depth ------------ */
/* Depth-consistency score of one hypothesis: its render compared pixel by pixel with a scene depth image (mm).
 * r = the hypothesis' rendered depth (pr_render's value at that pixel), s = the scene depth at the same frame pixel, tau = tau_mm.
 * Only pixels with r > 0 count. */
typedef struct {
    uint32_t visible;      /* pixels the hypothesis renders (== its cloud size in pr_refine_batch at the same pose / roi) */
    uint32_t inlier;       /* s > 0 and |r - s| <= tau                                                                   */
    uint32_t occluded;     /* s > 0 and s < r - tau : scene surface in front of the model                                */
    uint32_t violation;    /* s > 0 and s > r + tau : scene seen behind where the model would be (free-space violation)  */
    uint32_t missing;      /* s <= 0 : no measurement                                                                    */
    uint32_t reserved;     /* written as 0                                                                               */
    uint64_t abs_err_sum;  /* sum of |r - s| over the inlier pixels, mm (exact)                                          */
} pr_pose_score;           /* 32 B; visible == inlier + occluded + violation + missing                                  */

/* Renders every pose (inside `roi` only when one is given, as pr_refine_batch_roi does) and scores it against scene_depth_dev, a dense
 * width x height frame on the device: int32 when depth_is_i32 is set, uint16 otherwise (the flag of pr_scene_proj_prepare_dev).
 * scores_host receives n_poses records.  The scene is read on every call (nothing derived from it is kept).  Synchronous, on the
 * calling thread's context; a batch pending on an asynchronous slot is not disturbed.  PR_ERR_INVALID for tau_mm < 0, null pointers
 * with n_poses > 0 or a ROI outside the image; n_poses == 0 returns PR_OK and writes nothing.  The counts carry no ranking policy. */
int  pr_score_poses(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                    uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi,
                    const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, pr_pose_score *scores_host);
/* refined pose of hypothesis i = T'_i * pose_i, where T'_i is results[i].T with its translation (T[3], T[7], T[11]) times 1000.0f:
 * clouds are in metres (icp.cu:249, depth/1000), poses in mm.  Product in pr_mat4_mul's order.  Host only. */
void pr_refined_poses(const pr_result *results, const pr_mat4 *poses, uint32_t n, pr_mat4 *refined_out);

/* ---- mixed batches: hypotheses of several meshes in one call ----------------------------------------------------------------------
 * Hypothesis i is rendered with meshes[mesh_index_host[i]]; everything else is as in the single-mesh call.  For every i the depth image,
 * the record, the cloud size and the score are byte for byte what pr_render, pr_refine_batch_roi or pr_score_poses return for that mesh
 * and poses_host[i] with the same roi, scene, criteria and options.  Each mesh is its own device buffer (no concatenation); one pointer
 * may appear more than once, and an empty mesh (n_tris == 0) gives what the single-mesh calls give for one.  The library groups the
 * hypotheses by mesh (a stable sort), runs one batch -- one model-box pass over all meshes, one raster launch per chunk for all groups,
 * one ICP drive -- and returns the outputs in the caller's order.  The fused render always uses the box raster: option "raster_mode" = 1
 * (LDS bands) does not apply here (both modes give identical results).  Synchronous, on the calling thread's context; a batch pending on an
 * asynchronous slot is left alone.  PR_ERR_INVALID, with nothing written, for n_meshes == 0, a null pointer or mesh_index_host[i] >=
 * n_meshes with n_poses > 0, and for the single-mesh calls' frame, ROI and tau_mm checks; n_poses == 0 returns PR_OK and writes nothing. */
typedef struct { const pr_triangle *tris_dev; size_t n_tris; } pr_mesh_ref;   /* one mesh on the device (16 B) */
int  pr_render_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host, size_t n_poses,
                     size_t width, size_t height, const pr_mat4 *proj, pr_roi roi, int32_t *depth_dev_out);
int  pr_refine_batch_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                           uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9], int scene_kind,
                           const void *scene, pr_criteria crit, pr_roi roi, pr_result *results_host, uint32_t *cloud_sizes_host);
int  pr_score_poses_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                          uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                          int depth_is_i32, int32_t tau_mm, pr_pose_score *scores_host);

/* ---- coarse-to-fine refinement: a pyramid of strided clouds per hypothesis -------------------------------------------------------------
 * A pyramid is a table of 1 .. PR_PYRAMID_MAX_LEVELS levels, coarse first by convention (no order of the strides is imposed), each a stride
 * 1 .. PR_PYRAMID_MAX_STRIDE and the criteria of the ICP run on that level.  Let C1 be a hypothesis' stride-1 cloud exactly as
 * pr_refine_batch_roi builds it: the rendered pixels inside the ROI, row-major, back-projected with K at their frame coordinates.  The level
 * cloud of stride s is the subsequence of C1 whose FRAME pixel satisfies x % s == 0 && y % s == 0 -- the grid is anchored on the frame, not
 * on the ROI, so a window that contains the silhouette does not change the result; the points keep C1's bits and order.  (This is not the
 * reference's depth2cloud(stride), which back-projects grid indices and so needs the K of a down-sampled image: pr_depth2cloud_* keeps that
 * meaning.)  The render stays full-size; only the clouds are thinned.
 * With T_acc = I, level l takes its cloud, transforms it by T_acc when l > 0 (one transform of the original points, transform_pcd's
 * arithmetic), runs the ICP of pr_refine_batch on it with levels[l].crit -- same kernels, reduction tree, solve modes and early-exit rules --
 * which gives the level record (T_l, fitness_l, rmse_l), and T_acc = T_l * T_acc in pr_mat4_mul's order.  An empty level cloud, or a first
 * pass without a correspondence, gives the untouched record (identity, 0, 0) and T_acc carries over.  results_host[i] = T_acc with the
 * fitness and rmse of the LAST level, so pr_refined_poses and the pr_score_* family take it as they take pr_refine_batch's records.
 * level_results_host / level_sizes_host (either may be NULL): the records and cloud sizes of every level, [n_levels][n_poses].
 * One level of stride 1 returns pr_refine_batch_roi's records byte for byte.  Synchronous, on the calling thread's context; a batch pending
 * on an asynchronous slot finishes first and stays pending.  The level table is checked before any device is touched: PR_ERR_INVALID, with nothing written,
 * for n_levels == 0 or > PR_PYRAMID_MAX_LEVELS, a stride of 0 or > PR_PYRAMID_MAX_STRIDE, max_iteration < 0, and for levels or results_host
 * NULL with n_poses > 0; the frame, ROI and (multi) mesh-index checks of pr_refine_batch_roi / pr_refine_batch_multi apply as well.
 * n_poses == 0 returns PR_OK and writes nothing. */
#define PR_PYRAMID_MAX_LEVELS 4
#define PR_PYRAMID_MAX_STRIDE 16
typedef struct { uint32_t stride; pr_criteria crit; } pr_pyramid_level;   /* 16 B */
int  pr_refine_pyramid(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                       const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, const pr_pyramid_level *levels, uint32_t n_levels,
                       pr_roi roi, pr_result *results_host, pr_result *level_results_host, uint32_t *level_sizes_host);
int  pr_refine_pyramid_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                             uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9], int scene_kind,
                             const void *scene, const pr_pyramid_level *levels, uint32_t n_levels, pr_roi roi, pr_result *results_host,
                             pr_result *level_results_host, uint32_t *level_sizes_host);
/* The pyramid calls with robust weights (pr_robust above): n_robust == 1 is one descriptor for every level, n_robust == n_levels one per
 * level -- the annealing use, a wide c on the coarse level and a narrow one on the fine level; any other n_robust is PR_ERR_INVALID, as are
 * a null table and a descriptor pr_robust_describe would not have produced, all before any device is touched and with nothing written.
 * One level of stride 1 is the robust form of pr_refine_batch_roi.  With every descriptor PR_ROBUST_NONE the records are pr_refine_pyramid's
 * bytes.  Like the plain pyramid calls they neither record nor disarm pr_debug_trace_sums.  Synchronous only. */
int  pr_refine_pyramid_robust(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                              const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, const pr_pyramid_level *levels, uint32_t n_levels,
                              pr_roi roi, pr_result *results_host, pr_result *level_results_host, uint32_t *level_sizes_host,
                              const pr_robust *robust, uint32_t n_robust);
int  pr_refine_pyramid_robust_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                                    uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9], int scene_kind,
                                    const void *scene, const pr_pyramid_level *levels, uint32_t n_levels, pr_roi roi, pr_result *results_host,
                                    pr_result *level_results_host, uint32_t *level_sizes_host, const pr_robust *robust, uint32_t n_robust);

/* ---- pose observability: the information matrix of a hypothesis and its eigenvectors (no counterpart in the reference) -------------------
 * How well does the scene constrain a pose?  Per hypothesis: a cloud of n float32 points in the camera frame (metres; never modified), one scene
 * of any of the four kinds, an optional pr_robust (NULL: plain, w = 1), a centre c (three float32, camera frame) and a radius rho > 0 (float32,
 * metres).  Every point s that the plain pass would give a valid correspondence (d, n) -- same association, same acceptance -- contributes:
 *   float32   e = d - s;  r = (ex*nx + ey*ny) + ez*nz;  w = the weight of r (pr_robust above) -- exactly the pass' values
 *   float64   q = s - c;  a = (qy*nz - qz*ny, qz*nx - qx*nz, qx*ny - qy*nx) / rho;  J = (ax, ay, az, nx, ny, nz);  wJ[i] = w * J[i];  wr = w * r
 *             H[i][j] += wJ[i] * J[j]  (i <= j);   g[i] += wJ[i] * r;   sum_w += w;   sum_wr2 += wr * r;   sum_r2 += r * r
 * every operation rounded on its own (no contraction), '/' the correctly rounded division: tests/info_ref.py forms the same terms bit for bit.
 * The rotational half is divided by rho so that all six coordinates are metres of surface motion at distance rho from c and the eigenvalues
 * are comparable; rho = 1 gives plain radians.  Taking the moments about c (the object's centre) and not about the camera origin, and in
 * float64, is what separates "weak" from "unobservable": a direction the data do not constrain at all reads below 1e-15 of the largest
 * eigenvalue, against 1e-7 for float32 sums about the origin.
 * Order of addition: lane, wavefront and workgroup sums in a fixed tree, the workgroups' partial sums through memory in block order; no
 * floating-point atomics.  Two calls on the same inputs return the same bytes.
 * pr_pose_info (272 B): n_points 0 (the cloud's size), n_valid 4 (correspondences), n_zero_weight 8 (valid ones with w == 0.0f), reserved 12,
 *   c 16, rho 28, H 32 (21 doubles: i <= j, row-major -- the numbering of sums 0..20), g 200, sum_w 248, sum_wr2 256, sum_r2 264.
 * pr_pose_eig (344 B): lambda 0 (ascending), V 48 (row-major 6 x 6: V[6 * i + k] = component i of the unit eigenvector of lambda[k]; its
 *   component of largest magnitude is positive, the lowest index on a tie), sweeps 336, reserved 340.  The decomposition is of the symmetric
 *   6 x 6 filled from H, by cyclic Jacobi in float64:
 *     sweep      the 15 rotations (p, q), p < q, in row-major order
 *     rotation   skipped when A[p][q] == 0 exactly; else theta = (A[q][q] - A[p][p]) / (2 A[p][q]), t = sign(theta) / (|theta| +
 *                sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c
 *     stopping   before every sweep: done when max |A[p][q]| (p < q) <= 2^-56 max |A[p][p]|; at most PR_INFO_MAX_SWEEPS sweeps; `sweeps`
 *                is the number run (a diagonal matrix: 0)
 *   then the pairs sorted by a fixed 12-comparator network.
 * An empty cloud or n_valid == 0: every sum and count zero (n_points, c and rho as given), lambda zero, V the identity, sweeps 0. */
#define PR_INFO_MAX_SWEEPS 16
typedef struct {
    uint32_t n_points, n_valid, n_zero_weight, reserved;
    float c[3], rho;
    double H[21], g[6], sum_w, sum_wr2, sum_r2;
} pr_pose_info;                                                    /* 272 B */
typedef struct { double lambda[6]; double V[36]; uint32_t sweeps, reserved; } pr_pose_eig;      /* 344 B */
/* Cloud-level form, shaped like pr_icp_batch_robust: cloud i = clouds_dev[offsets_host[i] .. offsets_host[i + 1]), centre
 * centers_host[3 i .. 3 i + 2], radius radii_host[i]; info_host[n_clouds], eig_host[n_clouds] (or NULL: no decomposition).  All four scene
 * kinds.  kd-tree scenes with compact records are searched by the kernels an ICP pass uses (the pass reads their winners); a tree without them is
 * walked point by point with the reference's own ordered walk: the same records, several times the time.
 * PR_ERR_INVALID, before any device is touched and with nothing written: null offsets, centres, radii, info or scene (with n_clouds > 0), a
 * null cloud array with points, decreasing offsets, an unknown scene kind, a bad grid descriptor, a centre that is not finite, a radius that
 * is not finite or not positive, a descriptor pr_robust_describe would not have produced. */
int  pr_icp_information(const pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind, const void *scene,
                        const pr_robust *robust_or_null, const float *centers_host, const float *radii_host, pr_pose_info *info_host,
                        pr_pose_eig *eig_host_or_null);
/* Fused form: the render and cloud emission of pr_refine_batch_roi, then the information pass in place of the ICP loop -- the clouds are the
 * ones pr_refine_batch_roi would start from (cloud_sizes_host, optional, receives their sizes), the projective scene is read through its
 * packed record as there, and large batches run in the same chunks.  One centre and one radius for the mesh: center_model (three floats, model
 * frame and units) and radius (metres, the clouds' unit).  c_i = poses_host[i] applied to center_model in float64 on the host (rows 0..2:
 * ((m0*x + m1*y) + m2*z) + m3), divided by 1000.0 in float64 -- the cloud extraction's millimetres to metres -- and rounded to float32.
 * PR_ERR_INVALID as above, and for pr_refine_batch_roi's own argument errors and a null center_model. */
int  pr_pose_information(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                         const pr_mat4 *proj, const float K[9], int scene_kind, const void *scene, pr_roi roi, const pr_robust *robust_or_null,
                         const float *center_model, float radius, pr_pose_info *info_host, pr_pose_eig *eig_host_or_null,
                         uint32_t *cloud_sizes_host_or_null);
/* The same over a mesh table (pr_refine_batch_multi's): centers_model[3 m .. 3 m + 2] and radii[m] belong to mesh m.  Every record equals the
 * single-mesh call's. */
int  pr_pose_information_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                               uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, const float K[9], int scene_kind,
                               const void *scene, pr_roi roi, const pr_robust *robust_or_null, const float *centers_model, const float *radii,
                               pr_pose_info *info_host, pr_pose_eig *eig_host_or_null, uint32_t *cloud_sizes_host_or_null);
/* Covariance of the pose from one record pair.  Host only, needs no device.  rank = the number of k with lambda[k] > 0 and lambda[k] >
 * min_ratio * lambda[5];  cov = sigma2 * sum over those k of v_k v_k^T / lambda[k], in the scaled coordinates of J (cov21_out: i <= j,
 * row-major, H's numbering);  sigma2 = sigma * sigma when sigma > 0, otherwise (sum_wr2 / sum_w) * n_valid / (n_valid - 6).  cov21_out,
 * rank_out and sigma2_out may each be NULL.  PR_ERR_INVALID, nothing written: null info or eig, min_ratio negative or not finite, sigma not
 * finite, and sigma <= 0 with n_valid <= 6 or sum_w == 0. */
int  pr_info_covariance(const pr_pose_info *info, const pr_pose_eig *eig, double sigma, double min_ratio, double *cov21_out, uint32_t *rank_out,
                        double *sigma2_out);

/* ---- detections from a scored batch: which hypotheses explain the same scene pixels ------------------------------------------------------
 * The support of hypothesis i is the set of frame pixels pr_score_poses counts as `inlier` for it (rendered, s > 0, |r - s| <= tau_mm).
 * pr_score_overlap scores a batch exactly as pr_score_poses does -- scores_host is byte for byte the same -- and also returns
 * overlap_host[i * n_poses + j] = the number of frame pixels in the support of both i and j: symmetric, the diagonal equals
 * scores_host[i].inlier, rows and columns in the caller's pose order.  In a mixed batch (pr_score_overlap_multi, arguments as
 * pr_score_poses_multi) hypotheses of different meshes are compared like any other pair.  Argument checks, ROI, scene types and the
 * synchronous behaviour are those of pr_score_poses / pr_score_poses_multi; n_poses == 0 returns PR_OK and writes nothing; n_poses above
 * PR_OVERLAP_MAX_POSES is PR_ERR_INVALID.  The device keeps one bit per frame pixel and hypothesis while the call runs
 * (n_poses x height x ceil(width / 64) x 8 bytes) and the matrix (4 n_poses^2 bytes, once on the device and once in pinned memory). */
#define PR_OVERLAP_MAX_POSES 4096     /* a 64 MB matrix */
int  pr_score_overlap(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                      uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi,
                      const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, pr_pose_score *scores_host, uint32_t *overlap_host);
int  pr_score_overlap_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                            uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                            int depth_is_i32, int32_t tau_mm, pr_pose_score *scores_host, uint32_t *overlap_host);
/* Greedy selection, host only (needs no device).  order: n_order indices, best first, each < n_poses and none twice (else PR_ERR_INVALID);
 * overlap: an n_poses x n_poses matrix as above.  Walks order; skips i when overlap[i][i] == 0; accepts i unless an already accepted j has
 * overlap[i][j] * shared_den > shared_num * min(overlap[i][i], overlap[j][j]) (64-bit integers, no floats).  selected_out (room for n_order
 * indices) receives the accepted ones in acceptance order, *n_selected their number.  shared_den == 0 is PR_ERR_INVALID. */
int  pr_select_greedy(const uint32_t *order, uint32_t n_order, const uint32_t *overlap, uint32_t n_poses,
                      uint32_t shared_num, uint32_t shared_den, uint32_t *selected_out, uint32_t *n_selected);

/* ---- detections by cumulative cover: what does a hypothesis explain that the better ones have not? ---------------------------------------
 * pr_select_greedy asks every accepted hypothesis separately; a hypothesis that straddles two accepted detections can pass both tests
 * although no pixel of its support is new.  The cover rule looks at the accepted set as a whole.  All integers.  The support S_i is as
 * above: the frame pixels pr_score_poses counts as `inlier` for hypothesis i.  Inputs: order (n_order indices, best first, each < n_poses
 * and none twice), (new_num, new_den), min_new, max_keep.  Walk order with a claimed set C, empty at the start:
 *   - skip i when |S_i| == 0: state PR_COVER_EMPTY (whatever has been accepted so far);
 *   - once max_keep hypotheses are accepted nothing more is: every later i of the walk with |S_i| > 0 is PR_COVER_REJECTED with reason
 *     PR_COVER_REASON_CAP (max_keep == 0: all of them);
 *   - otherwise let fresh = |S_i \ C| and accept i when fresh >= min_new and (uint64)fresh * new_den >= (uint64)new_num * |S_i|; on
 *     acceptance C becomes C u S_i; a hypothesis that is not accepted is PR_COVER_REJECTED with reason PR_COVER_REASON_THRESHOLD.
 * C only grows, so fresh only shrinks: a hypothesis that fails against some C fails against every later one (the device walks in rounds
 * on the strength of this, and the bytes it returns do not depend on how).  With new_num == 0 and min_new == 1 a hypothesis is kept
 * exactly when it explains at least one new pixel.
 * Outputs: selected_out (room for n_order indices) = the accepted indices in acceptance order, *n_selected their number; one pr_pose_cover
 * per hypothesis of the batch, in the caller's pose order; one pr_cover_frame.  pr_pose_cover.fresh is the value at its acceptance for an
 * accepted hypothesis, 0 for an EMPTY one, and for every other one -- rejected for either reason, or not in order at all --
 * |S_i \ C_final|, counted after the walk against the final claimed set: how much of a dropped hypothesis the detections leave unexplained.
 * pr_score_cover renders and scores the batch exactly as pr_score_poses does -- scores_host is byte for byte the same -- and walks on
 * the device.  Argument checks, ROI, scene types, chunking and the synchronous behaviour are those of pr_score_poses
 * (pr_score_poses_multi for pr_score_cover_multi; hypotheses of different meshes claim pixels like any others).  PR_ERR_INVALID, with nothing
 * written, for new_den == 0, new_num > new_den, an index >= n_poses or one that appears twice in order, and a null order (with n_order >
 * 0), scores_host, cover_host, frame_host, selected_out or n_selected with n_poses > 0.  n_poses == 0 returns PR_OK, writes *n_selected
 * = 0 (when given) and nothing else; n_order == 0 is a walk that accepts nothing (every record NOT_IN_ORDER, fresh = support).
 * PR_OVERLAP_MAX_POSES does not apply: the device keeps one bit per frame pixel and hypothesis while the call runs (n_poses x height x
 * ceil(width / 64) x 8 bytes), one more such plane for C, and 24 bytes per hypothesis; a failed allocation is PR_ERR_NOMEM. */
#define PR_COVER_NOT_IN_ORDER      0u        /* pr_pose_cover.state & PR_COVER_STATE_MASK                                            */
#define PR_COVER_EMPTY             1u
#define PR_COVER_ACCEPTED          2u
#define PR_COVER_REJECTED          3u
#define PR_COVER_STATE_MASK        0xFFu
#define PR_COVER_REASON_THRESHOLD  0x100u    /* with PR_COVER_REJECTED: failed min_new or new_num / new_den                          */
#define PR_COVER_REASON_CAP        0x200u    /* with PR_COVER_REJECTED: max_keep hypotheses were accepted before the walk reached it */
#define PR_COVER_NO_POSITION       0xFFFFFFFFu
typedef struct {
    uint32_t support;          /* |S_i|, equal to scores_host[i].inlier                                                       */
    uint32_t fresh;            /* see above                                                                                   */
    uint32_t state;            /* PR_COVER_NOT_IN_ORDER, _EMPTY, _ACCEPTED, or _REJECTED | one PR_COVER_REASON_*              */
    uint32_t position;         /* the acceptance rank (index into selected_out), PR_COVER_NO_POSITION when not accepted       */
} pr_pose_cover;               /* 16 B */
typedef struct {
    uint32_t claimed;          /* |C_final|: the sum of fresh over the accepted hypotheses                                    */
    uint32_t n_selected;
    uint32_t reserved[2];      /* written as 0                                                                                */
} pr_cover_frame;              /* 16 B */
int  pr_score_cover(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                    uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi,
                    const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm,
                    const uint32_t *order, uint32_t n_order, uint32_t new_num, uint32_t new_den, uint32_t min_new, uint32_t max_keep,
                    pr_pose_score *scores_host, pr_pose_cover *cover_host, pr_cover_frame *frame_host,
                    uint32_t *selected_out, uint32_t *n_selected);
int  pr_score_cover_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                          uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                          int depth_is_i32, int32_t tau_mm,
                          const uint32_t *order, uint32_t n_order, uint32_t new_num, uint32_t new_den, uint32_t min_new, uint32_t max_keep,
                          pr_pose_score *scores_host, pr_pose_cover *cover_host, pr_cover_frame *frame_host,
                          uint32_t *selected_out, uint32_t *n_selected);
/* The same rule, host only (needs no device), on supports the caller brings as bit planes: planes[i * plane_words + w] is word w of
 * hypothesis i's plane, one bit per pixel in any layout the caller likes (the same for every hypothesis); |S_i| is its population count.
 * The small integer twin of the device walk, as pr_select_greedy is for the matrix.  Checks as above; also PR_ERR_INVALID for planes NULL
 * with n_poses > 0 and plane_words > 0, and for plane_words > 2^26 (a support must fit 32 bits). */
int  pr_select_cover_host(const uint64_t *planes, uint32_t n_poses, size_t plane_words, const uint32_t *order, uint32_t n_order,
                          uint32_t new_num, uint32_t new_den, uint32_t min_new, uint32_t max_keep,
                          pr_pose_cover *cover_out, pr_cover_frame *frame_out, uint32_t *selected_out, uint32_t *n_selected);

/* ---- contour check: do the depth edges of a hypothesis' render lie on depth edges of the scene? ------------------------------------------
 * pr_score_poses and the overlap matrix look at the interior of a render; a pose whose surface lies on scene surface (a face against a
 * wall, an object slid along the table) passes both although its silhouette is nowhere in the image.  All arithmetic is in integers
 * (differences in 64 bits), depth in mm.  A pixel is EMPTY when its depth is <= 0.  A pixel of a depth image is an EDGE pixel for jump_mm
 * when its depth d is > 0 and at least one of its four neighbours lies inside the image and is empty or farther by more than the jump
 * (d_n - d > jump_mm): the nearer side of a discontinuity, "no surface" counting as infinitely far.  Neighbours outside the image are
 * ignored (an object cut by the border has no contour there).  The image is the whole frame for the scene, and the frame -- or the ROI
 * window when one is given -- for a render.
 * pr_scene_edge_distance_dev writes D(x, y), the chessboard (L-infinity) distance from every frame pixel to the nearest scene edge pixel,
 * one uint8 per pixel, 255 when none lies within `radius` (0 <= radius <= PR_CONTOUR_MAX_RADIUS, jump_mm >= 0; else PR_ERR_INVALID).
 * scene_depth_dev is a dense width x height frame on the device, int32 when depth_is_i32 is set, uint16 otherwise; dist_dev_out holds
 * width * height bytes and belongs to the caller: the library keeps nothing by address.  Runs on the calling thread's context (three
 * kernels, no copy to or from the host) and returns when they are done. */
#define PR_CONTOUR_MAX_RADIUS 32
int  pr_scene_edge_distance_dev(const void *scene_depth_dev, int depth_is_i32, uint32_t width, uint32_t height, int32_t jump_mm,
                                uint32_t radius, uint8_t *dist_dev_out);
/* Contour record of one hypothesis, over the edge pixels c of its render: r = the rendered depth at c, s = the scene depth and D the
 * scene edge distance at the same frame pixel, tau = tau_mm. */
typedef struct {
    uint32_t contour;      /* edge pixels of the render                                                                  */
    uint32_t hit;          /* not occluded and D != 255                                                                  */
    uint32_t occluded;     /* s > 0 and r - s > tau (pr_pose_score's `occluded` test): no scene edge can be expected     */
    uint32_t miss;         /* not occluded and D == 255                                                                  */
    uint32_t reserved[2];  /* written as 0                                                                               */
    uint64_t dist_sum;     /* sum of D over the hit pixels (exact)                                                       */
} pr_pose_contour;         /* 32 B; contour == hit + occluded + miss                                                     */
/* pr_score_contours renders every pose once and returns, in the caller's pose order: scores_host, byte for byte what pr_score_poses
 * returns; contours_host, the records above for jump_mm against edge_dist_dev (pr_scene_edge_distance_dev's output for the same frame;
 * read on every call, as the scene is); and, when overlap_host is not NULL, pr_score_overlap's matrix (n_poses <= PR_OVERLAP_MAX_POSES
 * then).  Argument checks, ROI, scene types, chunking and the synchronous behaviour are those of pr_score_poses (pr_score_poses_multi for
 * pr_score_contours_multi); jump_mm < 0, or a null edge_dist_dev or contours_host with n_poses > 0, is PR_ERR_INVALID with nothing
 * written; n_poses == 0 returns PR_OK and writes nothing.  The counts carry no policy. */
int  pr_score_contours(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                       uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi,
                       const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, int32_t jump_mm, const uint8_t *edge_dist_dev,
                       pr_pose_score *scores_host, pr_pose_contour *contours_host, uint32_t *overlap_host);
int  pr_score_contours_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                             uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                             int depth_is_i32, int32_t tau_mm, int32_t jump_mm, const uint8_t *edge_dist_dev,
                             pr_pose_score *scores_host, pr_pose_contour *contours_host, uint32_t *overlap_host);

/* ---- contour alignment: the silhouette's normal equations in pr_pose_info's coordinates, and a pose step along the observable directions ------
 * The surface term (pr_pose_information) leaves free exactly the motions a face on a wall, a part slid along the table or a can spun about its
 * axis have; depth edges constrain them.  Edge pixels, the image and the occlusion test are the contour check's above.
 * Scene side, once per frame: pr_scene_edge_nearest_dev writes N(x, y) for every frame pixel: among the scene edge pixels (ex, ey) (the edge
 * pixels of pr_scene_edge_distance_dev for the same jump_mm) with |ex - x| <= radius and |ey - y| <= radius the one that minimises,
 * lexicographically, (dx^2 + dy^2, ey, ex), as the word ey << 16 | ex; PR_EDGE_NONE when the window holds no edge pixel -- so N != PR_EDGE_NONE
 * exactly where D != 255.  nearest_dev_out holds width * height words and belongs to the caller: the library keeps nothing by address.
 * Arguments, checks and behaviour otherwise as pr_scene_edge_distance_dev (three kernels).
 * Hypothesis side: pr_contour_information renders every pose once (pr_score_contours' arguments, with nearest_dev in place of the distance
 * image and no overlap matrix) and returns per hypothesis, in the caller's order: scores_host (may be NULL), byte for byte pr_score_poses'
 * records; fit_host, the record below; info_host, a pr_pose_info about c_i with radius rho, formed from K, center_model and radius exactly as
 * pr_pose_information forms them.  A render edge pixel at frame (x, y) with rendered depth r and scene depth s is OCCLUDED when s > 0 and
 * r - s > tau_mm, USED when it is not occluded and N(x, y) != PR_EDGE_NONE, and a MISS otherwise: contour, used, occluded, miss equal
 * pr_score_contours' contour, hit, occluded, miss.  sum_d2 = the sum over the used pixels of (ex - x)^2 + (ey - y)^2, exact.  Every used pixel
 * contributes two rows, in float64 with every operation rounded on its own, fx = K[0], cx = K[2], fy = K[4], cy = K[5] converted to double
 * once and x, y, ex, ey, r taken as integers:
 *     Z = r / 1000.0;  s = ((x - cx) * Z / fx, (y - cy) * Z / fy, Z);  q = s - c
 *     row 1:  n = (1, 0, -(x - cx) / fx),  res = (ex - x) * Z / fx          row 2:  n = (0, 1, -(y - cy) / fy),  res = (ey - y) * Z / fy
 *     a = (qy*nz - qz*ny, qz*nx - qx*nz, qx*ny - qy*nx) / rho;  J = (a, n);  H[i][j] += J[i] * J[j] (i <= j);  g[i] += J[i] * res
 *     sum_wr2 = sum_r2 = the sum of res * res;  sum_w = 2 * used;  n_points = contour, n_valid = used, n_zero_weight = 0
 * the linearised pinhole residuals in metres at the pixel's depth, with pr_pose_info's sign: solving H delta = g moves the render edge towards
 * the scene edge.  Order of addition as for pr_pose_info: lane, wavefront and workgroup sums in a fixed tree, the workgroups' partial sums
 * through memory in block order, no floating-point atomics; two calls return the same bytes, and a hypothesis' records depend neither on how
 * the batch is chunked nor on what else is in it.  An empty render or used == 0: every sum zero (c and rho as given).
 * Known limit: two rows per pixel count information ALONG a straight edge that the data do not hold (the nearest scene edge pixel says nothing
 * about a slide along the edge), so such a slide is damped, not free.  Point-to-line rows and a robust weight are not part of this call.
 * PR_ERR_INVALID, nothing written: pr_score_contours' argument errors (nearest_dev for edge_dist_dev, fit_host for contours_host), a null K,
 * center_model (centers_model, radii), or info_host with n_poses > 0, a K with a non-finite entry or K[0] or K[4] zero, a centre that is not
 * finite, a radius that is not finite or not positive.  n_poses == 0 returns PR_OK and writes nothing. */
#define PR_EDGE_NONE 0xFFFFFFFFu
int  pr_scene_edge_nearest_dev(const void *scene_depth_dev, int depth_is_i32, uint32_t width, uint32_t height, int32_t jump_mm,
                               uint32_t radius, uint32_t *nearest_dev_out);
typedef struct {
    uint32_t contour;      /* edge pixels of the render                                                                  */
    uint32_t used;         /* not occluded and N != PR_EDGE_NONE: two rows each                                          */
    uint32_t occluded;     /* s > 0 and r - s > tau                                                                      */
    uint32_t miss;         /* not occluded and N == PR_EDGE_NONE                                                         */
    uint32_t reserved[2];  /* written as 0                                                                               */
    uint64_t sum_d2;       /* sum over the used pixels of the squared pixel distance to N (exact)                        */
} pr_contour_fit;          /* 32 B; contour == used + occluded + miss                                                    */
int  pr_contour_information(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                            uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi,
                            const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, int32_t jump_mm, const uint32_t *nearest_dev,
                            const float K[9], const float *center_model, float radius,
                            pr_pose_score *scores_host_or_null, pr_contour_fit *fit_host, pr_pose_info *info_host);
int  pr_contour_information_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                                  uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                                  int depth_is_i32, int32_t tau_mm, int32_t jump_mm, const uint32_t *nearest_dev, const float K[9],
                                  const float *centers_model, const float *radii,
                                  pr_pose_score *scores_host_or_null, pr_contour_fit *fit_host, pr_pose_info *info_host);
/* Host only, float64, no device needed.
 * pr_info_combine: out = wa * a + wb * b for H, g, sum_w and sum_wr2 (each product rounded, then the sum); sum_r2 and the three counts are
 * added; c and rho are a's.  PR_ERR_INVALID, nothing written: a null pointer, c or rho not bitwise equal in a and b, a weight that is not
 * finite or is negative.  out may be a or b.
 * pr_info_eig: the decomposition of info->H exactly as specified for pr_pose_eig above (sweep order, rotation, stopping rule, sort, sign
 * rule), on the host.
 * pr_info_step: keep the eigenpairs k with lambda[k] > 0 and lambda[k] > min_ratio * lambda[5] (pr_info_covariance's rule; rank = their
 * number); delta = the sum over the kept k, ascending, of v_k * ((v_k . g) / lambda[k]), the dot product summed from component 0 to 5;
 * theta = delta[0..2] / rho, t = delta[3..5]; R = I + (sin a / a) [theta]x + ((1 - cos a) / a^2) [theta]x^2 with a = |theta| (R = I when
 * a == 0); E = [R | 1000 * (c - R c + t)] -- the twist about c in metres applied to a pose in millimetres; pose_out = E * pose_in (row 3:
 * pose_in's) in float64, rounded to float32 once.  rank 0 returns pose_in and delta = 0.  delta6_out and rank_out may be NULL; pose_out may
 * be pose_in.  PR_ERR_INVALID, nothing written: a null info, eig, pose_in or pose_out, min_ratio negative or not finite. */
int  pr_info_combine(const pr_pose_info *a, double wa, const pr_pose_info *b, double wb, pr_pose_info *out);
int  pr_info_eig(const pr_pose_info *info, pr_pose_eig *eig_out);
int  pr_info_step(const pr_pose_info *info, const pr_pose_eig *eig, double min_ratio, const pr_mat4 *pose_in, pr_mat4 *pose_out,
                  double *delta6_out, uint32_t *rank_out);

/* ---- normal agreement: does the surface of a hypothesis' render face the way the scene's surface does? --------------------------------------
 * The depth score, the overlap matrix and the contour check are blind to a pose whose surface lies within tau_mm of scene surface with the
 * wrong orientation or curvature (a box face laid on a wall, a curved part pressed against a table): it collects inliers.  Where the depths
 * agree, the normals should.  Both normals are estimated from depth, with the same estimator.
 * Depth is integer mm.  A pixel is empty when its depth is <= 0, or when the render drew nothing there.  Let h = step with
 * 1 <= h <= PR_NORMAL_MAX_STEP = 8.  Let J = jump_mm >= 0.  Take K row-major as everywhere: fx = K[0], cx = K[2], fy = K[4], cy = K[5],
 * each converted to double once.
 * Normal of image d at frame pixel (x, y).  It is defined iff all of these hold:
 *   - d(x, y) > 0;
 *   - the four pixels (x +- h, y) and (x, y +- h) lie inside the image;
 *   - those four pixels are non-empty;
 *   - each of them differs from d(x, y) by at most J.  The difference is taken in 64-bit integers.
 * The image is the whole frame for the scene.  For a render it is the frame, or the ROI window when one is given.  A neighbour outside the
 * image makes the normal undefined.  A neighbour inside the image but outside the render's packed box is empty by construction.
 * With gu = d(x + h, y) - d(x - h, y), gv = d(x, y + h) - d(x, y - h) and z = d(x, y), all converted to double, the normal is computed in
 * double in exactly this order with no contraction:
 *     a = -(fx * gu)
 *     b = -(fy * gv)
 *     c = ((2h) * z + (x - cx) * gu) + (y - cy) * gv
 * The normal is unnormalised and points away from the camera.  It is exact for a fronto-parallel plane.
 * Agreement.  Take the render normal (a_r, b_r, c_r) and the scene normal (a_s, b_s, c_s) at the same frame pixel.  Compute:
 *     dot = (a_r * a_s + b_r * b_s) + c_r * c_s
 *     q   = (a * a + b * b) + c * c          (once per image)
 *     m   = (double)cos_min
 * The pixel agrees iff dot >= 0 and dot * dot >= (m * m) * (q_r * q_s).  There is no square root and no division.
 * Record per hypothesis.  Counts run over the pixels pr_score_poses counts as `inlier`, with the same tau_mm test. */
#define PR_NORMAL_MAX_STEP 8
typedef struct {
    uint32_t tested;            /* inlier pixels where both normals are defined          */
    uint32_t agree;             /* tested pixels that agree                              */
    uint32_t disagree;          /* tested pixels that do not                             */
    uint32_t no_render_normal;  /* inlier pixels, render normal undefined                */
    uint32_t no_scene_normal;   /* inlier pixels, render normal defined, scene's not     */
    uint32_t reserved[3];       /* written as 0                                          */
} pr_pose_normal;               /* 32 B; tested == agree + disagree; scores.inlier == tested + no_render_normal + no_scene_normal */
/* pr_score_normals renders every pose once and returns, in the caller's pose order: scores_host, byte for byte what pr_score_poses
 * returns; normals_host, the records above; and, when overlap_host is not NULL, pr_score_overlap's matrix from the same render (n_poses
 * <= PR_OVERLAP_MAX_POSES then), exactly as pr_score_contours does it.  Argument checks, ROI, scene types, chunking and the synchronous
 * behaviour are those of pr_score_poses (pr_score_poses_multi for pr_score_normals_multi, which equals one single-mesh call per mesh, byte
 * for byte).  PR_ERR_INVALID with nothing written for a step of 0 or above PR_NORMAL_MAX_STEP, jump_mm < 0, cos_min outside [0, 1] or NaN
 * (all three checked before any device use), and for a null K or normals_host with n_poses > 0; n_poses == 0 returns PR_OK and writes
 * nothing.  The counts carry no policy. */
int  pr_score_normals(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                      uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev, int depth_is_i32,
                      int32_t tau_mm, const float K[9], uint32_t step, int32_t jump_mm, float cos_min,
                      pr_pose_score *scores_host, pr_pose_normal *normals_host, uint32_t *overlap_host);
int  pr_score_normals_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                            uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                            int depth_is_i32, int32_t tau_mm, const float K[9], uint32_t step, int32_t jump_mm, float cos_min,
                            pr_pose_score *scores_host, pr_pose_normal *normals_host, uint32_t *overlap_host);

/* ---- composition: the detections of a frame taken together -----------------------------------------------------------------------------
 * Everything above looks at a hypothesis on its own or at pairs.  pr_compose_detections renders a set of poses -- typically the few that
 * pr_select_greedy kept -- and composes them: all arithmetic in integers (differences in 64 bits), depth in mm.  r_i(q) is hypothesis i's
 * rendered depth at frame pixel q (pr_render's value; 0 where nothing is drawn), front(q) the minimum of the positive r_i(q), and owner(q)
 * the LOWEST index in the caller's pose order that attains it (so duplicates and ties have a defined owner, in mixed batches too).
 *   labels_dev_out[q] = owner(q), or PR_COMPOSE_NONE where no hypothesis renders;  depth_dev_out[q] = front(q), or 0.
 * Both are dense width x height frames in the caller's device memory (either may be NULL); with a ROI the pixels outside the window get
 * PR_COMPOSE_NONE and 0; every pixel of both is written by every call with n_poses > 0.
 *   scores_host  = byte for byte what pr_score_poses returns (each hypothesis on its own, as if the others were not there);
 *   visible_host = per hypothesis the frame pixels it owns, by pr_pose_score's four tests with r = r_i(q) = front(q) there;
 *   frame_host   = the frame (the ROI window when one is given) against the composite, r = front(q).
 * So scores.visible - owned is what other hypotheses hide of i, scores.inlier - owned_inlier the support it claims under another model;
 * the sum of owned over i equals covered, of owned_inlier explained, of owned_occluded behind, of owned_violation in_front, of
 * owned_missing unmeasured.  Argument checks, ROI, scene types, chunking and the synchronous behaviour are those of pr_score_poses
 * (pr_score_poses_multi for pr_compose_detections_multi); a batch pending on an asynchronous slot is left alone.  n_poses == 0 returns
 * PR_OK and writes nothing; n_poses > PR_COMPOSE_MAX_POSES is PR_ERR_INVALID (checked before anything else); a null scores_host,
 * visible_host or frame_host with n_poses > 0 is PR_ERR_INVALID with nothing written.  The device keeps 8 bytes per frame pixel between
 * calls (a grow-only workspace of the context).  Not offered: an asynchronous form, and re-scoring other hypotheses against the composite. */
#define PR_COMPOSE_NONE      0xFFFFu
#define PR_COMPOSE_MAX_POSES 65535u          /* a label is a uint16 */
typedef struct {
    uint32_t owned;            /* frame pixels whose front-most render is this hypothesis'                                    */
    uint32_t owned_inlier;     /* of those: s > 0 and |r - s| <= tau                                                          */
    uint32_t owned_occluded;   /* s > 0 and r - s > tau                                                                       */
    uint32_t owned_violation;  /* s > 0 and s - r > tau                                                                       */
    uint32_t owned_missing;    /* s <= 0                                                                                      */
    uint32_t reserved[3];      /* written as 0                                                                                */
} pr_pose_visible;             /* 32 B; owned == owned_inlier + owned_occluded + owned_violation + owned_missing              */
typedef struct {
    uint32_t window;           /* pixels of the frame, or of the ROI window                                                   */
    uint32_t measured;         /* of those: s > 0                                                                             */
    uint32_t covered;          /* of those: some hypothesis renders there                                                     */
    uint32_t explained;        /* covered, s > 0 and |front - s| <= tau                                                       */
    uint32_t in_front;         /* covered, s > 0 and s - front > tau: the composite lies before the measured surface          */
    uint32_t behind;           /* covered, s > 0 and front - s > tau: it lies behind the measured surface                     */
    uint32_t unmeasured;       /* covered and s <= 0                                                                          */
    uint32_t reserved;         /* written as 0                                                                                */
} pr_frame_explained;          /* 32 B; covered == explained + in_front + behind + unmeasured                                 */
int  pr_compose_detections(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses,
                           uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi,
                           const void *scene_depth_dev, int depth_is_i32, int32_t tau_mm, uint16_t *labels_dev_out, int32_t *depth_dev_out,
                           pr_pose_score *scores_host, pr_pose_visible *visible_host, pr_frame_explained *frame_host);
int  pr_compose_detections_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                                 uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, pr_roi roi, const void *scene_depth_dev,
                                 int depth_is_i32, int32_t tau_mm, uint16_t *labels_dev_out, int32_t *depth_dev_out,
                                 pr_pose_score *scores_host, pr_pose_visible *visible_host, pr_frame_explained *frame_host);

/* ---- pose distances: how far apart are two poses? ---------------------------------------------------------------------------------------
 * Everything above compares a pose with an image.  pr_pose_distance compares poses with each other, by the displacement of the model's
 * surface points between them (the BOP family of pose errors): its mean (ADD), its maximum (MSSD) and its maximum in the image (MSPD), each
 * minimised over a finite set of symmetry transforms of the model.  Poses are pr_mat4, row-major, in mm, as everywhere; points are pr_vec3
 * in model coordinates.  For one pair (A, B) and the candidates k = 0 .. n-1, S_0 .. S_(n-1) = syms_host (n_syms == 0: the identity alone,
 * which gives the bytes of n_syms == 1 with an identity matrix):
 *   1. matrices, in double: As = A * S_k, rows 0..2, every entry summed in pr_mat4_mul's order (0 + a3 s3 + a2 s2 + a1 s1 + a0 s0), and
 *      D = As - B.  Both are rounded to float32 once.  Forming the difference of the MATRICES first keeps near-identical poses accurate: a
 *      0.03 mm shift at 320 mm gives a maximum of 0.0300007 mm (truth 0.03000069) and a mean of 1966 * 2^-16 = 0.0299988 mm (half a quantum
 *      off); the difference of two transformed float32 points loses that with |t|.
 *   2. per point v = (x, y, z), float32, no contraction: d_r = ((D[r][0]*x + D[r][1]*y) + D[r][2]*z) + D[r][3], d2 = (d_0*d_0 + d_1*d_1) + d_2*d_2.
 *   3. sum_k  = sum over v of (uint64) min(rintf(sqrtf(d2) * 65536.0f), 2^40): the summed displacement in units of 2^-16 mm, an exact integer
 *      that does not depend on the order of summation (sqrtf correctly rounded; a NaN term counts as 2^40).
 *   4. maxd_k = max over v of d2, float32, mm^2 (from 0; a NaN d2 is passed over).
 *   5. only with K: a = As v and b = B v in the three-term form of 2., u = K[0]*X/Z + K[2], w = K[4]*Y/Z + K[5] for both, and
 *      maxp_k = max over v of (ua-ub)^2 + (wa-wb)^2, px^2 -- or +inf if any point of either pose has Z <= 0.  Two float32 projections are
 *      subtracted here: the absolute accuracy is about 1e-4 px (5e-5 px measured on the benchmark's hypotheses), whatever the poses.
 *   6. the record: each of the three minima over k on its own, the lowest k on a tie.
 * Points must be finite (they cannot be checked without a pass over them), and so must every float32 intermediate be for the maxima to mean
 * anything: |t| up to 2e7 mm merely saturates the sum's terms.  n_points <= PR_POSE_DIST_MAX_POINTS keeps the sum inside 64 bits.
 * all_pairs == 0: n_a == n_b and out_host[i] compares a_host[i] with b_host[i].  all_pairs != 0: out_host[i * n_b + j] compares a_host[i]
 * with b_host[j]; n_b == 1 is "everything against one ground truth".  points_dev is device memory (n_points x 12 bytes), read on every call.
 * Synchronous, on the calling thread's context; a batch pending on an asynchronous slot is not disturbed.  PR_ERR_INVALID, with nothing
 * written and BEFORE any device is touched (so also on a machine without one), for: n_a or n_b > PR_POSE_DIST_MAX_POSES, n_syms >
 * PR_POSE_DIST_MAX_SYMS, n_a != n_b without all_pairs; and, with pairs to compute: n_points == 0 or > PR_POSE_DIST_MAX_POINTS, a null
 * points_dev, a_host, b_host, out_host (or syms_host with n_syms > 0), a non-finite entry in any pose, symmetry or K, K[0] == 0 or K[4] == 0.
 * No pairs: PR_OK, nothing written, no device needed.  While a call runs the device holds 96 bytes per (a, symmetry) and 48 per b, and the
 * host as much pinned memory; larger calls run as several launches of at most 2^18 candidates (pair x symmetry). */
#define PR_POSE_DIST_MAX_SYMS   64
#define PR_POSE_DIST_MAX_POSES  4096
#define PR_POSE_DIST_MAX_POINTS (1u << 24)
typedef struct {
    uint64_t disp_sum_q16;   /* min_k sum_k: mean displacement = disp_sum_q16 / 65536 / n_points mm                              */
    float    max_disp_sq;    /* min_k maxd_k, mm^2                                                                             */
    float    max_proj_sq;    /* min_k maxp_k, px^2; 0 when K == NULL                                                           */
    uint16_t sym_sum, sym_disp, sym_proj;   /* the k of each minimum; sym_proj 0 when K == NULL                               */
    uint16_t reserved;       /* written as 0                                                                                   */
    uint32_t n_points;
    uint32_t reserved2;      /* written as 0                                                                                   */
} pr_pose_dist;              /* 32 B                                                                                           */
int  pr_pose_distance(const pr_vec3 *points_dev, uint32_t n_points, const pr_mat4 *a_host, uint32_t n_a, const pr_mat4 *b_host, uint32_t n_b,
                      int all_pairs, const pr_mat4 *syms_host, uint32_t n_syms, const float K[9] /* may be NULL */, pr_pose_dist *out_host);
/* Greedy merging of duplicates in pose space, host only (needs no device); the shape of pr_select_greedy.  order: n_order indices, best
 * first, each < n_poses and none twice (else PR_ERR_INVALID); dist: the n_poses x n_poses matrix of an all_pairs call of the poses with
 * themselves.  Walks order; keeps i unless an already kept j has dist[i][j].max_disp_sq <= max_disp_mm^2 OR dist[j][i].max_disp_sq <=
 * max_disp_mm^2 (the square formed in float32) -- with symmetries the matrix is not exactly symmetric, because a model's vertex set is only
 * approximately invariant under them, so both entries are asked.  kept_out (room for n_order indices) receives the kept ones in that
 * order, *n_kept their number; rep_out (n_poses entries, or NULL) receives for every i in order the kept hypothesis that absorbed it -- the
 * first such j in kept order, i itself if kept; entries of hypotheses outside order are not written.  A negative or non-finite
 * max_disp_mm is PR_ERR_INVALID. */
int  pr_cluster_greedy(const uint32_t *order, uint32_t n_order, const pr_pose_dist *dist, uint32_t n_poses, float max_disp_mm,
                       uint32_t *kept_out, uint32_t *n_kept, uint32_t *rep_out);

/* ---- visible surface discrepancy (VSD): do an estimate and the truth show the same surface in the measured frame? --------------------------
 * The third member of the BOP family of pose errors, next to pr_pose_distance's MSSD and MSPD.  Both poses of a pair are rendered, each is
 * asked where it is visible in the scene depth frame, and the pixels of the two visible surfaces that disagree are counted.  This is the
 * BOP-2019 convention ("bop19" visibility, step cost) restated from memory: the toolkit was not at hand when this was written, so nothing
 * here pins it beyond this text.
 * One mesh; n_est estimated and n_gt ground-truth poses: n_gt == n_est compares est_host[i] with gt_host[i], n_gt == 1 compares every
 * estimate with the one truth (rendered once per depth chunk, not once per estimate); anything else is invalid.  proj as pr_render takes it;
 * scene_depth_dev is a dense width x height frame on the device in mm, int32 when depth_is_i32 is set, uint16 otherwise, read on every
 * call; K = 9 intrinsics or NULL; delta_mm = the visibility tolerance, taus_mm[n_taus] the misalignment tolerances (non-decreasing).  There
 * is no ROI: an evaluation is full-frame.
 * For frame pixel (x, y), y the image row as the scene frame stores it, e and g = pr_render's values of the estimate and the truth there,
 * s = the scene value; everything float32, no contraction, '/' and sqrtf correctly rounded:
 *   1. ray factor: with K, xn = ((float)x - K[2]) / K[0], yn = ((float)y - K[5]) / K[4], c = sqrtf((xn*xn + yn*yn) + 1.0f); with K == NULL
 *      c = 1.0f -- distances are then depths, and every quantity below is an integer as long as delta, the taus and the depths are integers
 *      below 2^24.
 *   2. distances: E = e > 0 ? (float)e * c : 0, G from g likewise, T = s > 0 ? (float)s * c : 0 (s <= 0: no measurement).
 *   3. visibility: vg = G > 0 && (T == 0 || G - T <= delta);  ve = E > 0 && (T == 0 || E - T <= delta || vg).
 *   4. inter = vg && ve, uni = vg || ve, and for every k: far_k = inter && fabsf(G - E) >= tau_k.
 * The record counts these over the frame; being integers, the counts are exact in any order of summation.  BOP's error for tau_k is
 * (far[k] + uni - inter) / uni, or 1 when uni == 0; that division is the caller's.
 * Synchronous, on the calling thread's context and its own stream and workspaces; a batch pending on an asynchronous slot is not disturbed;
 * nothing derived from the scene is kept.  PR_ERR_INVALID, with nothing written and BEFORE any device is touched (so also on a machine
 * without one), for: n_gt neither n_est nor 1; n_taus > PR_VSD_MAX_TAUS; delta_mm or a tau negative or not finite; taus not non-decreasing;
 * a non-finite entry of K, K[0] == 0 or K[4] == 0; width or height 0 or a frame beyond the scoring calls' size limit; and, with pairs to
 * compute: a non-finite pose entry, a null proj, est_host, gt_host, scene_depth_dev, out_host, taus_mm (n_taus > 0) or tris_dev (n_tris > 0).
 * n_est == 0 returns PR_OK, writes nothing and needs no device.
 * pr_pose_vsd_multi: estimate i and its truth are rendered with meshes[mesh_index_host[i]] (the mesh table of the mixed batches above);
 * n_gt == n_est only; records in the caller's order, each byte for byte what the single-mesh call gives that pair; a mesh index out of
 * range, n_meshes == 0 or a null table is PR_ERR_INVALID.  Not offered: an asynchronous form, a ROI, the "tlinear" cost, keeping the
 * truth's render between calls. */
#define PR_VSD_MAX_TAUS 12
typedef struct {
    uint32_t visib_gt;     /* pixels with vg                                                                                  */
    uint32_t visib_est;    /* pixels with ve                                                                                  */
    uint32_t inter;        /* vg && ve                                                                                        */
    uint32_t uni;          /* vg || ve                                                                                        */
    uint32_t far[PR_VSD_MAX_TAUS];   /* inter && |G - E| >= taus_mm[k]; entries at and beyond n_taus are written as 0        */
} pr_vsd_counts;           /* 64 B; the record of one pair                                                                    */
int  pr_pose_vsd(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *est_host, uint32_t n_est, const pr_mat4 *gt_host, uint32_t n_gt,
                 uint32_t width, uint32_t height, const pr_mat4 *proj, const void *scene_depth_dev, int depth_is_i32,
                 const float K[9] /* may be NULL */, float delta_mm, const float *taus_mm, uint32_t n_taus, pr_vsd_counts *out_host);
int  pr_pose_vsd_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *est_host, uint32_t n_est,
                       const pr_mat4 *gt_host, uint32_t n_gt, uint32_t width, uint32_t height, const pr_mat4 *proj, const void *scene_depth_dev,
                       int depth_is_i32, const float K[9] /* may be NULL */, float delta_mm, const float *taus_mm, uint32_t n_taus,
                       pr_vsd_counts *out_host);

/* ---- interpenetration: do two detections claim the same space? ---------------------------------------------------------------------------
 * The pixel rules above cannot tell an object that lies BEHIND another (thousands of shared pixels, no shared volume: legitimate) from two
 * refinements that sank into each other (fewer shared pixels, a lot of shared volume: impossible).  Per pixel a closed mesh occupies the depth
 * interval [near, far] along the ray, near the nearest and far the farthest fragment the raster produces there; two hypotheses interpenetrate
 * at a pixel exactly where their intervals overlap.  Everything is integer millimetres.
 *
 * pr_render_span: pr_render with a second output.  near_dev_out is byte for byte what pr_render writes for the same arguments (0 where nothing
 * was drawn); far_dev_out[q] is the largest fragment depth at q -- the maximum of the very int32 values whose minimum is near -- and 0 where
 * no fragment fell.  Both are n_poses images of the frame (or of the ROI).  Argument checks are pr_render's; far_dev_out == NULL (or
 * near_dev_out == NULL) with n_poses > 0 is PR_ERR_INVALID.
 *
 * pr_pose_penetration: the P x P matrix of pr_pair_solid records of n_poses hypotheses of one mesh, rows and columns in the caller's order.
 * For frame pixel q and hypotheses i, j, with near / far as the raster leaves them:
 *   both:   near_i(q) and near_j(q) are both rendered (> 0 and not "nothing drawn");
 *   len:    min(far_i(q), far_j(q)) - max(near_i(q), near_j(q)), a 64-bit difference;
 *   inter:  both && len > slack_mm;   sum_mm = the sum of len, max_mm the largest len, over the inter pixels.
 * The matrix is symmetric.  The diagonal is a hypothesis with itself: both = its rendered pixels, sum_mm = the sum of its own thickness,
 * its "volume" in mm x pixels; hence sum_mm[i][j] <= min(sum_mm[i][i], sum_mm[j][j]).  Integer sums and maxima with one writer per record:
 * the same bytes on every call and for every order of the batch (permuted with it).  No scene and no ROI; synchronous, on the calling
 * thread's context and its own stream and workspaces; a batch pending on an asynchronous slot is not disturbed.
 * Limits of the definition: the interval is the HULL of the solid along the ray -- exact for objects that are convex along the viewing rays,
 * an over-estimate for a cup or a bracket with something inside it; silhouette pixels with one fragment have thickness 0; an open mesh has
 * no volume (its far surface is its near surface where only one sheet is seen).
 * PR_ERR_INVALID, with nothing written and BEFORE any device is touched (so also on a machine without one), with a message that names the
 * numbers, for: slack_mm < 0; n_poses > PR_PENETRATION_MAX_POSES; width or height 0 or a frame beyond the scoring calls' size limit;
 * 2 x n_poses renders of the frame beyond the scoring calls' depth workspace bound (4 GiB: the near and far boxes of a call are resident
 * together, there is no chunking); and, with n_poses > 0, a null proj, poses_host, pairs_host or tris_dev (n_tris > 0).  n_poses == 0
 * returns PR_OK and writes nothing.
 * pr_pose_penetration_multi: hypothesis i is rendered with meshes[mesh_index_host[i]] (the mesh table of the mixed batches above); the
 * matrix in the caller's order, a one-mesh batch byte for byte the single-mesh call's; a mesh index out of range, n_meshes == 0 or a null
 * table is PR_ERR_INVALID.  Not offered: exact solids for objects concave along the ray, a ROI, batches beyond one resident workspace. */
int  pr_render_span(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, size_t n_poses, size_t width, size_t height,
                    const pr_mat4 *proj, pr_roi roi, int32_t *near_dev_out, int32_t *far_dev_out);
#define PR_PENETRATION_MAX_POSES 1024
typedef struct {
    uint32_t both;      /* frame pixels where i and j both render                                                              */
    uint32_t inter;     /* of those: len = min(far_i, far_j) - max(near_i, near_j) > slack_mm   (64-bit differences)           */
    uint32_t max_mm;    /* largest len over the inter pixels, 0 when inter == 0                                                */
    uint32_t reserved;  /* written as 0                                                                                        */
    uint64_t sum_mm;    /* exact sum of len over the inter pixels                                                              */
} pr_pair_solid;        /* 24 B; the record of one pair                                                                        */
int  pr_pose_penetration(const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses_host, uint32_t n_poses, uint32_t width, uint32_t height,
                         const pr_mat4 *proj, int32_t slack_mm, pr_pair_solid *pairs_host /* n_poses x n_poses */);
int  pr_pose_penetration_multi(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host, const pr_mat4 *poses_host,
                               uint32_t n_poses, uint32_t width, uint32_t height, const pr_mat4 *proj, int32_t slack_mm,
                               pr_pair_solid *pairs_host /* n_poses x n_poses */);
/* Greedy selection of detections that can coexist, host only (needs no device); the shape of pr_select_greedy.  order: n_order indices, best
 * first; pairs: pr_pose_penetration's n_poses x n_poses records.  i is kept unless an already kept j has
 *   pairs[i][j].sum_mm * den > num * min(pairs[i][i].sum_mm, pairs[j][j].sum_mm)          (128-bit products)
 * i.e. shares more than num / den of the smaller of the two volumes; in a matrix of the device a hypothesis without volume never conflicts.
 * selected_out: room for n_order indices.  PR_ERR_INVALID, with nothing written: an index out of range or twice in order, den == 0, a null
 * pointer that is needed. */
int  pr_select_disjoint(const uint32_t *order, uint32_t n_order, const pr_pair_solid *pairs, uint32_t n_poses, uint32_t num, uint32_t den,
                        uint32_t *selected_out, uint32_t *n_selected);

/* ---- hypotheses from the scene: point-pair-feature (PPF) voting (Drost et al. 2010) --------------------------------------------------------
 * Everything above starts from poses somebody supplies.  These entry points make that list from a depth frame and a mesh alone: the model's
 * oriented surface points are hashed once by the feature of every ordered pair, every scene reference point pairs with the other scene
 * points, looks up the model pairs with the same feature and votes for (model point, rotation angle); the peaks of a reference's accumulator
 * are poses.  Votes are integer counts, so every accumulator is exact in any order.  All lengths in mm, normals as they are (not normalised
 * here).  Every integer below is fixed by this text; float32 arithmetic without contraction, + - * / and the correctly rounded sqrtf only, no
 * trigonometric function per pair: angles are binned by comparisons against the tables pr_ppf_describe computes ONCE, on the host, in double
 * (device and references read the tables of the descriptor and never recompute them -- the rule of pr_scene_grid.inv_cell).
 *   dot(a, b) = (ax*bx + ay*by) + az*bz;   len(a) = sqrtf(dot(a, a));   a value is "good" when it is finite, a length when also > 0.
 *   frame of an oriented point (p, n): e = the coordinate axis of the smallest |component| of n (the lowest index on a tie);  w = e x n
 *     (e = x: (0, -nz, ny), y: (nz, 0, -nx), z: (-ny, nx, 0));  u = w / len(w), component by component;  v = n x u =
 *     (ny*uz - nz*uy, nz*ux - nx*uz, nx*uy - ny*ux).  No frame (and no pair) when len(w) is not good.
 *   ordered pair, reference (p_r, n_r) with frame (u, v) and other point (p_i, n_i):  d = p_i - p_r, L = len(d), t = L * inv_dist_step;
 *     c1 = dot(n_r, d) / L, c2 = dot(n_i, d) / L, c3 = dot(n_r, n_i);  y = dot(d, u), z = dot(d, v), r = sqrtf(y*y + z*z);  the pair's
 *     angle is the unit vector (y / r, z / r).  The pair is SKIPPED unless L and r are good, t < n_dist and c1, c2, c3 are finite (a point
 *     paired with itself or with a coincident one has L == 0).
 *   angle bin of c: the number of k in 1 .. n_angle-1 with c <= cos_edge[k] (0 .. n_angle-1; clamps by itself for |c| slightly above 1).
 *   key = ((b_d*A + b1)*A + b2)*A + b3, b_d = (int)t, b1..b3 the angle bins of c1..c3, A = n_angle;  key < n_keys = n_dist * A^3.
 *   vote angle alpha = (scene pair's angle) - (model pair's angle), the rotation about the frames' common x axis (the normal) that carries the
 *     model pair's other point onto the scene pair's, as a complex product of the unit vectors (cs, ss) and (cm, sm):
 *     ca = cs*cm + ss*sm, sa = ss*cm - cs*sm, q = sqrtf(ca*ca + sa*sa) (no vote unless good), cn = ca / q,
 *     h = the number of k in 1 .. n_alpha/2-1 with cn <= alpha_edge[k];  bin = h when sa >= 0.0f, else n_alpha-1-h.
 *     The boundary rule: sa == 0 of either sign is the UPPER half-plane, so alpha = 0 falls into bin 0 and alpha = pi into bin n_alpha/2-1;
 *     bin b covers [b, b+1) * 2 pi / n_alpha up to the rounding of cn, its centre is (b + 0.5) * 2 pi / n_alpha.
 *   pose of a peak (model point m, scene point s, alpha bin b), in DOUBLE from the float32 inputs, rounded to float32 once:  for either
 *     oriented point nh = n / sqrt(dot(n, n)), e chosen as above on the float32 n, w = e x nh, u = w / sqrt(dot(w, w)), v = nh x u,
 *     B = rows (nh, u, v);  with (c, s) = (alpha_cos[b], alpha_sin[b]):  M = rows (Bm_0, c*Bm_1 - s*Bm_2, s*Bm_1 + c*Bm_2),
 *     R[i][j] = (Bs[0][i]*M[0][j] + Bs[1][i]*M[1][j]) + Bs[2][i]*M[2][j]  (R = Bs^T Rx(centre) Bm),  t[i] = p_s[i] - dot(R[i], p_m);
 *     the matrix is [R t; 0 0 0 1].
 * pr_ppf_describe: dist_step = dist_step_mm, inv_dist_step = 1.0f / dist_step, n_dist = ceil(diameter / dist_step) in double (1 ..
 * PR_PPF_MAX_DIST_BINS), n_angle 2 .. PR_PPF_MAX_ANGLE_BINS with cos_edge[k] = (float)cos(k pi / n_angle), k = 0 .. n_angle, n_alpha even, 2 ..
 * PR_PPF_MAX_ALPHA_BINS, with alpha_edge[k] = (float)cos(k 2 pi / n_alpha), k = 0 .. n_alpha/2 (the edges in [0, pi]) and the double cosine
 * and sine of every bin centre.  PR_ERR_INVALID with nothing written for anything else (a non-finite or non-positive length, a null out).
 * Host only.  Every entry point below that takes a descriptor checks it against these rules (not the tables' values).
 * pr_ppf_model_sample (host only): oriented points of a mesh at spacing step_mm.  Per triangle, N = max(1, ceil(longest edge / step)) and the
 * lattice v0 + (i/N)(v1 - v0) + (j/N)(v2 - v0), i = 0 .. N, j = 0 .. N-i (i outer), in double, rounded to float32; of the points of all
 * triangles in (triangle, lattice) order the FIRST in every voxel (floor(coordinate / step) per axis, in double, of the rounded point) is kept.
 * The normal is (v1 - v0) x (v2 - v0) normalised in double, negated when flip_normals, rounded; triangles whose normal has no good length are
 * skipped.  points_out / normals_out: room for PR_PPF_MAX_MODEL_POINTS; *n_out = the number of points found; more than the cap (the walk stops
 * there, *n_out = the cap + 1), a triangle that needs more than 10^6 subdivisions, a non-finite or non-positive step or a null pointer:
 * PR_ERR_INVALID (the caller coarsens the step).
 * pr_ppf_model_build_dev: the direct-addressed table of the model, no hash function: offsets_dev_out[n_keys + 1] and one 12-byte entry per
 * ordered pair (ref, other), ref != other, that is not skipped, in bucket key: entries [offsets[key], offsets[key+1]).  The SET of a bucket
 * is fixed by the text above, the order inside it is not (votes do not depend on it).  entries_dev_out: room for n_model * (n_model - 1).
 * *n_entries_out = offsets[n_keys].  1 <= n_model <= PR_PPF_MAX_MODEL_POINTS.
 * pr_ppf_scene_points_dev: the pixels (x, y) with x % stride == 0 and y % stride == 0 of a pr_scene_proj (dense pcd and normal, metres) whose
 * normal has a non-zero component and whose pcd z is > 0, compacted in row-major pixel order: point = pcd * 1000.0f per component, normal as it
 * is.  points_dev_out / normals_dev_out: room for PR_PPF_MAX_SCENE_POINTS.  *n_out = the number kept; more than the cap: PR_ERR_INVALID with
 * nothing emitted (raise the stride).  stride 1 .. PR_PPF_MAX_STRIDE.  The same frame gives the same bytes.
 * pr_ppf_vote: reference j = scene point ref_first + j * ref_stride, j < n_refs (all < n_scene).  Its accumulator acc[m * n_alpha + bin]
 * counts, over every scene point i that forms a pair with it and every entry (m, other, cm, sm) of that pair's bucket, one vote in the bin
 * above.  n_model * n_alpha <= PR_PPF_MAX_CELLS (the accumulator lives in one workgroup's LDS).  Peaks: the n_peaks (1 .. PR_PPF_MAX_PEAKS) first
 * cells in the order (votes descending, cell index ascending) among the cells with votes > 0; peaks_host[j * n_peaks + k], an unused slot has
 * votes = 0, model_ref = alpha_bin = 0 and an all-zero pose.  n_pairs: the scene points that formed a pair with the reference.  poses_host:
 * the pose of every peak by the formula above, from one read-back of the peaks and the references; model_points_host / model_normals_host are
 * the sampler's HOST arrays.  acc_dev_out (may be NULL; tests and tools): n_refs x n_model x n_alpha uint32.  No float atomics anywhere.
 * The device entry points are synchronous, on the calling thread's context; a batch pending on an asynchronous slot is not disturbed.  Every
 * argument is checked BEFORE any device is touched (PR_ERR_INVALID also on a machine without one): a bad descriptor, a cap exceeded, a null
 * pointer, n_peaks outside 1 .. 4, ref_stride == 0, a reference at or beyond n_scene.  n_refs == 0: PR_OK, nothing written.
 * pr_ppf_peak_pose: the formula for one peak, host only.  PR_ERR_INVALID (nothing written) for a null pointer, alpha_bin >= n_alpha or a
 * normal without a frame.
 * pr_ppf_vote_multi: a table of models (at most PR_PPF_MAX_MODELS) over one scene sample, in one call: the outputs are those of pr_ppf_vote
 * called once per model with the same scene arguments, concatenated in table order -- peaks_host[(k * n_refs + j) * n_peaks + p] and poses_host
 * likewise for model k, reference j, peak p; acc_dev_out (may be NULL): model k's n_refs * n_model_k * n_alpha_k words, starting at the sum of
 * the sizes of the models before it.  Every byte equals the single call's; the same model listed twice gives the same bytes twice.  A
 * pr_ppf_model names a model as pr_ppf_vote's arguments do: the descriptor (host), pr_ppf_model_build_dev's two outputs, the sampler's host arrays
 * and n_model; models may differ in every field of their descriptors and in n_model.  A model with n_model == 1 has no pairs and returns no peak
 * (entries_dev may be NULL for it).  n_models == 0 or n_refs == 0: PR_OK, nothing written, no device used.  Checked before any device is touched,
 * PR_ERR_INVALID with nothing written: n_models > PR_PPF_MAX_MODELS, a model that fails pr_ppf_vote's checks of a descriptor, n_model or
 * PR_PPF_MAX_CELLS (the message names the model's index), reserved != 0, a null pointer, and pr_ppf_vote's checks of the scene, the peaks and the
 * references.  One launch -- a workgroup per (model, reference), its dynamic LDS sized by the table's largest n_model * n_alpha -- one stream
 * synchronise and one read-back per call; option "ppf_walk" selects the bucket walk as in pr_ppf_vote.
 * Not offered: votes spread to neighbouring bins, averaged cluster poses, an asynchronous form, colour or edge point pairs, keeping a scene
 * sample between calls, a mixed pr_pose_distance for merging the hypotheses of several models in one call. */
#define PR_PPF_MAX_DIST_BINS    64
#define PR_PPF_MAX_ANGLE_BINS   32
#define PR_PPF_MAX_ALPHA_BINS   64
#define PR_PPF_MAX_KEYS         (1u << 21)
#define PR_PPF_MAX_MODEL_POINTS 2048
#define PR_PPF_MAX_SCENE_POINTS 16384
#define PR_PPF_MAX_CELLS        32768        /* n_model * n_alpha: 128 KiB of the CU's 160 KiB of LDS */
#define PR_PPF_MAX_PEAKS        4
#define PR_PPF_MAX_STRIDE       256
typedef struct {
    float    diameter, dist_step, inv_dist_step;
    uint32_t n_dist, n_angle, n_alpha, n_keys, flip_model_normals;
    float    cos_edge[PR_PPF_MAX_ANGLE_BINS + 1];         /* [0 .. n_angle], the rest 0                                          */
    float    alpha_edge[PR_PPF_MAX_ALPHA_BINS / 2 + 1];   /* [0 .. n_alpha/2], the rest 0                                        */
    double   alpha_cos[PR_PPF_MAX_ALPHA_BINS];            /* bin centres; only the pose formula reads them                       */
    double   alpha_sin[PR_PPF_MAX_ALPHA_BINS];
} pr_ppf_params;               /* 1320 B */
typedef struct { uint32_t pair; float cos_m, sin_m; } pr_ppf_entry;      /* 12 B; pair = ref << 16 | other                        */
typedef struct {
    uint32_t votes;
    uint16_t model_ref, alpha_bin;
    uint32_t scene_ref;        /* index into the scene points                                                                    */
    uint32_t n_pairs;
} pr_ppf_peak;                 /* 16 B */
int  pr_ppf_describe(float diameter_mm, float dist_step_mm, uint32_t n_angle, uint32_t n_alpha, int flip_model_normals, pr_ppf_params *out);
int  pr_ppf_model_sample(const pr_triangle *tris_host, size_t n_tris, float step_mm, int flip_normals, pr_vec3 *points_out, pr_vec3 *normals_out,
                         uint32_t *n_out);
int  pr_ppf_model_build_dev(const pr_ppf_params *params, const pr_vec3 *points_dev, const pr_vec3 *normals_dev, uint32_t n_model,
                            uint32_t *offsets_dev_out, pr_ppf_entry *entries_dev_out, uint32_t *n_entries_out);
int  pr_ppf_scene_points_dev(const pr_scene_proj *scene, uint32_t stride, pr_vec3 *points_dev_out, pr_vec3 *normals_dev_out, uint32_t *n_out);
int  pr_ppf_vote(const pr_ppf_params *params, const uint32_t *offsets_dev, const pr_ppf_entry *entries_dev, const pr_vec3 *model_points_host,
                 const pr_vec3 *model_normals_host, uint32_t n_model, const pr_vec3 *scene_points_dev, const pr_vec3 *scene_normals_dev,
                 uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks, pr_ppf_peak *peaks_host,
                 pr_mat4 *poses_host, uint32_t *acc_dev_out /* may be NULL */);
int  pr_ppf_peak_pose(const pr_ppf_params *params, const pr_vec3 *model_point, const pr_vec3 *model_normal, const pr_vec3 *scene_point,
                      const pr_vec3 *scene_normal, uint32_t alpha_bin, pr_mat4 *pose_out);
#define PR_PPF_MAX_MODELS 32
typedef struct {
    const pr_ppf_params *params;                           /* host                                                              */
    const uint32_t      *offsets_dev;                      /* pr_ppf_model_build_dev's outputs                                  */
    const pr_ppf_entry  *entries_dev;                      /* may be NULL when n_model == 1                                     */
    const pr_vec3       *points_host, *normals_host;       /* the sampler's arrays, for the pose formula                        */
    uint32_t             n_model, reserved;                /* reserved = 0                                                      */
} pr_ppf_model;                /* 48 B */
int  pr_ppf_vote_multi(const pr_ppf_model *models, uint32_t n_models, const pr_vec3 *scene_points_dev, const pr_vec3 *scene_normals_dev,
                       uint32_t n_scene, uint32_t ref_first, uint32_t ref_stride, uint32_t n_refs, uint32_t n_peaks, pr_ppf_peak *peaks_host,
                       pr_mat4 *poses_host, uint32_t *acc_dev_out /* may be NULL */);

/* ---- support planes: the dominant planes of a depth frame, peeled one after another ---------------------------------------------------------
 * The voting above assumes a frame in which the object is most of what there is.  A real frame has a table, a bin floor or a wall behind the
 * parts: at stride 4 it holds more samples than PR_PPF_MAX_SCENE_POINTS, most pairs are plane-plane pairs, and the refiner feels the plane.
 * These entry points find the planes, label their pixels and clear them from the depth frame; the cleared frame goes unchanged into
 * pr_scene_proj_prepare_dev, pr_scene_nn_prepare_dev, the sampler above and the scorers.  The method is a consensus over candidates that already
 * carry a normal: ONE oriented scene point defines a plane, so a candidate costs nothing to make and the work is counting its support.  Every
 * integer below is fixed by this text; per-sample arithmetic is float32 without contraction in the stated order, + - * only, no transcendental
 * function; the refit is exact integer arithmetic up to one conversion to double.  dot(a, b) = (ax*bx + ay*by) + az*bz as above; a pixel "has a
 * normal" when a component of its normal is != 0.
 *   sample: the pixels (x, y) with x % stride == 0 and y % stride == 0 of a full-frame pr_scene_proj (dense pcd and normal, metres) that have
 *     a normal, pcd z > 0 and pcd.z * 1000.0f <= 65535.0f, in row-major order: point = pcd * 1000.0f per component (mm), normal as it is, and the
 *     pixel's index y * width + x.  More than PR_PLANE_MAX_SAMPLES: PR_ERR_INVALID with nothing written (raise the stride).
 *   candidates: candidate c is sample c * cand_stride, c < n_candidates = ceil(n_samples / cand_stride).  More than PR_PLANE_MAX_CANDIDATES:
 *     PR_ERR_INVALID with nothing written (raise cand_stride).  A sample is ALIVE while its pixel's label is 0.
 *   the normal test of (a, b):  cos_min == -2.0f (the test is off), or dot(a, b) >= cos_min.
 *   support of an alive candidate (p_c, n_c): the number of alive samples (p_j, m_j), itself included, with
 *     r = dot(n_c, p_j - p_c) (the difference component by component first), fabsf(r) <= tau_mm, and the normal test of (n_c, m_j).
 *     A dead candidate has support 0.
 *   winner of a round: the largest support, the lowest candidate index on a tie.  Support below min_support (or no support at all), or a
 *     refit that pr_plane_from_moments refuses, ends the peel: fewer planes than asked for, not an error.
 *   refit: over the winner's inliers (the same two tests) q = (int64) rint((double) coordinate * 16.0) per coordinate and the ten moments
 *     n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz as exact 64-bit integer sums (any order gives the same bytes; no float atomics anywhere).
 *     pr_plane_from_moments: the scatter matrix C_ab = n * S_ab - S_a * S_b exactly in 128-bit integers, each entry converted to double once
 *     (n^2 times the covariance, in 1/16 mm units); cyclic Jacobi in float64 on the symmetric 3 x 3 with V = I at the start: at most
 *     PR_PLANE_MAX_SWEEPS sweeps; before each, off = the largest |C[i][j]|, i < j, diag = the largest |C[i][i]|, stop when off <= 2^-56 * diag;
 *     a sweep rotates (p, q) = (0,1), (0,2), (1,2) by pr_info_eig's rotation (skipped when C[p][q] == 0: theta = (C[q][q] - C[p][p]) /
 *     (2 C[p][q]), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) with sign(0) = +1, c = 1 / sqrt(t^2 + 1), s = t c; C[p][p] -= t C[p][q],
 *     C[q][q] += t C[p][q], C[p][q] = 0; for the third index k: (C[k][p], C[k][q]) <- (c C[k][p] - s C[k][q], s C[k][p] + c C[k][q]), mirrored;
 *     for every row k of V likewise).  lambda[i] = C[i][i]; the plane's eigenvalue is the smallest, the lowest index on a tie; its column of V,
 *     divided by sqrt(dot) of itself, is the normal nu.  offset = dot(nu, (Sx, Sy, Sz)) / n / 16 in double (mm; dot as above), and the plane is
 *     the points with dot(nu, p) == offset.  Orientation, towards the camera: offset <= 0 -- when offset > 0, or offset == 0 and the first
 *     non-zero component of nu is positive, nu and offset are negated.  rms = sqrt(max(lambda_min, 0)) / n / 16 (mm).  PR_ERR_INVALID for
 *     n < 3, an all-zero scatter matrix or a column without a length.  pr_plane holds normal and offset_mm ROUNDED ONCE to float32.
 *     eig_out (may be NULL, as rms_mm_out): the plane's eigenvalue first, then the other two in index order.
 *   labels, one uint8 per pixel of the full-resolution frame: pcd z <= 0: PR_PLANE_NO_DEPTH.  Otherwise, in round k = 1, 2, ... with the
 *     round's float32 plane (nu, offset): h = dot(nu, pcd * 1000.0f) - offset (the products per component first); a pixel whose label is
 *     still 0 takes k when fabsf(h) <= label_tau_mm and, if it has a normal, the normal test of (nu, its normal) holds; else, in round 1 only
 *     and when drop_behind is set, PR_PLANE_BEHIND when h < -label_tau_mm (farther from the camera than plane 1: under the table, behind the
 *     wall); else it stays 0.  Round k + 1 runs over the samples that are still alive.
 *   cleared depth: depth_out[i] = labels[i] == 0 ? depth_in[i] : 0 (int32 or uint16 by depth_is_i32); depth_out may be depth_in.
 * pr_plane_describe (host only): fills and checks the parameters.  PR_ERR_INVALID with nothing written: stride 0 or > PR_PPF_MAX_STRIDE,
 * cand_stride 0, a tau that is not finite or < 0, cos_min neither -2 nor in [-1, 1], min_support < 3, n_planes outside 1 ..
 * PR_PLANE_MAX_PLANES, a null out.  Every entry point below checks its pr_plane_params against these rules.
 * pr_scene_planes_dev: planes_host[PR_PLANE_MAX_PLANES is enough; n_planes are needed], *n_found of them filled (candidate and support: the
 * winner; labelled / behind: the pixels the round gave k / PR_PLANE_BEHIND).  moments_host (may be NULL): 10 int64 per found plane.
 * support_dev_out (may be NULL; tests and tools): n_planes rows of PR_PLANE_MAX_CANDIDATES uint32, row k the supports of round k + 1 in its
 * first n_candidates words; everything else 0 (the row of a round that ended the peel is kept, the rows behind it are 0).
 * labels_dev_out: width * height uint8.  depth_dev_out may be NULL (no cleared depth).  Synchronous, on the calling thread's context; one
 * stream synchronise and one small pinned read-back for the sample's size, one per round and one at the end; no hipMemcpy on the path.  An
 * empty sample: PR_OK, *n_found = 0, every measured pixel labelled 0, the depth copied.  Checked before any device is touched: the
 * parameters, null pointers, the frame's size.  The same frame gives the same bytes.
 * pr_scene_planes_host: the same over host arrays (pcd and normal as pr_scene_proj_prepare leaves them), from the same shared code: the CPU
 * twin the device is held to; it runs without a GPU.  support_out: host, same layout.
 * Not offered: RANSAC over point triples (a candidate is one oriented point), cylinders and spheres, an
 * asynchronous form, a refit iterated to convergence. */
#define PR_PLANE_MAX_SAMPLES    65536
#define PR_PLANE_MAX_CANDIDATES 4096
#define PR_PLANE_MAX_PLANES     4
#define PR_PLANE_MAX_SWEEPS     16
#define PR_PLANE_BEHIND         254
#define PR_PLANE_NO_DEPTH       255
typedef struct {
    uint32_t stride, cand_stride;
    float    tau_mm, label_tau_mm, cos_min;
    uint32_t min_support, n_planes, drop_behind;
} pr_plane_params;             /* 32 B */
typedef struct {
    float    normal[3], offset_mm;     /* dot(normal, p_mm) == offset_mm, offset_mm <= 0                                              */
    uint32_t candidate, support;       /* the winner and its support                                                                  */
    uint32_t labelled, behind;         /* pixels of the frame this round labelled k / PR_PLANE_BEHIND                                 */
    float    rms_mm;
    uint32_t reserved[3];
} pr_plane;                    /* 48 B */
int  pr_plane_describe(uint32_t stride, uint32_t cand_stride, float tau_mm, float label_tau_mm, float cos_min, uint32_t min_support, uint32_t n_planes,
                       int drop_behind, pr_plane_params *out);
int  pr_plane_from_moments(const int64_t moments[10], double normal_out[3], double *offset_mm_out, double *rms_mm_out, double eig_out[3]);
int  pr_scene_planes_dev(const pr_scene_proj *scene, const void *depth_dev, int depth_is_i32, const pr_plane_params *params, uint8_t *labels_dev_out,
                         void *depth_dev_out /* may be NULL */, pr_plane *planes_host, int64_t *moments_host /* may be NULL */,
                         uint32_t *support_dev_out /* may be NULL */, uint32_t *n_found);
int  pr_scene_planes_host(const float *pcd, const float *normal, const void *depth, int depth_is_i32, size_t width, size_t height,
                          const pr_plane_params *params, uint8_t *labels_out, void *depth_out /* may be NULL */, pr_plane *planes_out,
                          int64_t *moments_out /* may be NULL */, uint32_t *support_out /* may be NULL */, uint32_t *n_found);

/* ---- scene segments: the depth-connected components of a frame -----------------------------------------------------------------------------
 * With the support planes cleared, what is left of a frame is a handful of parts with nothing measured between them.  These entry points cut the
 * frame into its connected blobs: a label image, one record per blob with its pixel box, and a depth frame that keeps chosen blobs only.  That
 * frame goes unchanged into pr_scene_proj_prepare_dev, pr_scene_nn_prepare_dev, the PPF sampler and the scorers, and the box (pr_segment_roi) is
 * the pr_roi that pr_refine_batch_roi, pr_refine_pyramid*, the scorers and pr_compose_detections take.  Integers only; every output byte is fixed
 * by this text, on the device and on the host.
 *   frame: width x height depths, uint16 or int32 (depth_is_i32), 1 <= width, height <= 65535 and width * height <= 2^26; otherwise
 *     PR_ERR_INVALID.  A pixel's index is y * width + x.
 *   measured pixel: depth > 0 (a negative int32 is not measured).
 *   link: two measured pixels that are 4-neighbours (left / right / up / down) are linked when |d_a - d_b| <= jump_mm, the difference formed
 *     without overflow (the larger minus the smaller, as unsigned 32-bit integers).
 *   component: a class of the transitive closure of the links; its ROOT is the lowest pixel index in it.  *n_components counts all of them.
 *   qualifying component: pixels >= min_pixels.  More than PR_SEGMENT_MAX_ROOTS qualifying components: PR_ERR_INVALID with no output written
 *     (raise min_pixels).
 *   order: the qualifying components by pixels descending, the lower root first on a tie; n_found = min(qualifying, max_segments), and segment
 *     k (1-based) is the k-th of that order.
 *   labels, one uint16 per pixel: 0 where nothing is measured, k in 1 .. n_found on the pixels of segment k, PR_SEGMENT_DROPPED on the measured
 *     pixels of every other component (too small, or beyond max_segments).
 *   pr_segment, one per found segment: root, pixels, the inclusive pixel box x0 <= x <= x1, y0 <= y <= y1, the smallest and largest depth, and the
 *     exact sums of x, y and depth over its pixels; reserved = 0.
 * pr_segment_describe (host only): fills and checks the parameters.  PR_ERR_INVALID with nothing written: min_pixels == 0, max_segments outside
 * 1 .. PR_SEGMENT_MAX, jump_mm > 2^31 - 1, a null out.  Every entry point below checks its pr_segment_params against these rules (and reserved == 0).
 * pr_scene_segments_dev: depth_dev and labels_dev_out (width * height uint16) on the device; roots_dev_out (may be NULL; tests and tools): one
 * uint32 per pixel, the root of the pixel's component, 0xFFFFFFFF where nothing is measured.  segments_host: room for max_segments records,
 * *n_found of them filled.  n_qualifying and n_components may be NULL.  Synchronous, on the calling thread's context: two stream synchronises and
 * two pinned read-backs (the qualifying roots, then the records), no hipMemcpy on the path; the number of launches and synchronisations does not
 * depend on the frame's content.  Checked before any device is touched: the parameters, null pointers, the frame's size.  The same frame gives
 * the same bytes on every call.
 * pr_scene_segments_host: the same over host arrays, from the same shared code: the CPU twin the device is held to; it runs without a GPU.
 * pr_segment_depth_dev: depth_out[i] = (labels[i] < n_keep && keep_host[labels[i]]) ? depth_in[i] : 0 over n_px pixels (int32 or uint16 by
 * depth_is_i32); keep_host: n_keep bytes indexed by label, n_keep <= PR_SEGMENT_MAX + 1; labels 0 and PR_SEGMENT_DROPPED are never kept;
 * depth_out may be depth_in.  n_px == 0 or > 2^26, n_keep > PR_SEGMENT_MAX + 1, a null pointer (keep_host may be NULL when n_keep == 0): PR_ERR_INVALID.
 * pr_segment_roi (host only): the segment's box grown by margin pixels on every side and clipped to the frame, as a pr_roi (x, y, width, height).
 * PR_ERR_INVALID for a null pointer, a frame outside the limits above or a box that does not lie in the frame.
 * Not offered: 8-connectivity, a 3-D Euclidean or normal criterion for a link, an asynchronous form. */
#define PR_SEGMENT_MAX        4096
#define PR_SEGMENT_MAX_ROOTS  65536
#define PR_SEGMENT_DROPPED    65535
typedef struct {
    uint32_t jump_mm, min_pixels, max_segments, reserved;
} pr_segment_params;           /* 16 B */
typedef struct {
    uint32_t root, pixels;             /* the component's lowest pixel index; its pixel count                                         */
    uint16_t x0, y0, x1, y1;           /* the inclusive pixel box                                                                     */
    uint32_t depth_min, depth_max;
    uint64_t sum_x, sum_y, sum_depth;  /* exact                                                                                       */
    uint64_t reserved[2];
} pr_segment;                  /* 64 B */
int  pr_segment_describe(uint32_t jump_mm, uint32_t min_pixels, uint32_t max_segments, pr_segment_params *out);
int  pr_scene_segments_dev(const void *depth_dev, int depth_is_i32, size_t width, size_t height, const pr_segment_params *params,
                           uint16_t *labels_dev_out, uint32_t *roots_dev_out /* may be NULL */, pr_segment *segments_host, uint32_t *n_found,
                           uint32_t *n_qualifying /* may be NULL */, uint32_t *n_components /* may be NULL */);
int  pr_scene_segments_host(const void *depth, int depth_is_i32, size_t width, size_t height, const pr_segment_params *params, uint16_t *labels_out,
                            uint32_t *roots_out /* may be NULL */, pr_segment *segments_out, uint32_t *n_found, uint32_t *n_qualifying /* may be NULL */,
                            uint32_t *n_components /* may be NULL */);
int  pr_segment_depth_dev(const uint16_t *labels_dev, const void *depth_in_dev, int depth_is_i32, size_t n_px, const uint8_t *keep_host, uint32_t n_keep,
                          void *depth_out_dev);
int  pr_segment_roi(const pr_segment *segment, size_t width, size_t height, uint32_t margin, pr_roi *roi_out);

/* ---- depth conditioning: fuse frames, drop flying pixels, median, fill holes -----------------------------------------------------------------
 * The stage in front of all the others, for a frame that comes from a camera and not from a renderer: the values a sensor reports between
 * foreground and background at a depth jump (flying pixels), per-pixel noise and holes.  The cleaned frame keeps the caller's depth type and
 * goes unchanged into pr_scene_proj_prepare_dev, pr_scene_nn_prepare_dev, pr_scene_planes_dev, pr_scene_segments_dev, the PPF sampler and every
 * scorer.  Integers only; every output byte is fixed by this text, on the device and on the host.  Every output value is one of the input
 * values, so the depth type never overflows.
 *   frame: width x height depths, uint16 or int32 (depth_is_i32), 1 <= width, height <= 65535 and width * height <= 2^26; otherwise
 *     PR_ERR_INVALID.  A pixel's index is y * width + x.  A pixel outside the frame is not measured.
 *   D0[p]: the depth as an unsigned 32-bit value; a non-positive int32 is 0, which means not measured (pr_scene_segments_dev's rule).
 *   lower median of a non-empty multiset of k values: element (k - 1) / 2 (integer division) of its ascending order.
 *   |a - b|: the larger minus the smaller, as unsigned 32-bit integers (no overflow).
 * pr_depth_fuse_dev: the per-pixel median over 1 <= n_frames <= PR_DEPTH_FUSE_MAX frames of ONE view, 1 <= min_frames <= n_frames.  Per pixel: M =
 * the multiset of the D0 values that are not 0 over the frames, count = |M| (count_out_dev, one uint8 per pixel, may be NULL), out = the lower
 * median of M when count >= min_frames, else 0.  frames: a HOST array of n_frames device pointers (they travel as kernel arguments; two entries may
 * be the same pointer); n_px: 1 .. 2^26 pixels.  depth_out_dev may be one of the frames: the operation is element-wise, every value of a pixel is
 * read before the pixel is written.  One launch, one stream synchronise, no hipMemcpy.  PR_ERR_INVALID with nothing written: a null table, entry or
 * output, n_frames, min_frames or n_px outside their limits.
 * pr_depth_filter_dev: four stages; each reads only the stage before it, over the whole frame, so the result depends on no order.
 *   tol(d) = tol_mm + floor(d * tol_permille / 1000), the product formed in 64 bits; the sum fits 32 bits.
 *   gate:   G[p] = D0[p] when D0[p] != 0, D0[p] >= min_mm and (max_mm == 0 or D0[p] <= max_mm); otherwise 0.
 *   flying: support(p) = the number of the 8 neighbours q of p inside the frame with G[q] != 0 and |G[q] - G[p]| <= tol(G[p]) (a corner pixel has
 *     three neighbours, a border pixel five).  F[p] = G[p] when G[p] != 0 and (fly_min_support == 0 or support(p) >= fly_min_support); otherwise 0.
 *   median, where F[p] != 0: S = { F[q] : q in the frame, |qx - px| <= radius, |qy - py| <= radius, F[q] != 0, |F[q] - F[p]| <= tol(F[p]) } (S holds
 *     F[p]); out[p] = the lower median of S.  radius == 0: out[p] = F[p].  Values across a depth jump are never mixed.
 *   fill, only where D0[p] == 0 (a gated or flying pixel is never filled back) and fill_min > 0: C = { F[q] : q in the window, F[q] != 0 }.  When
 *     |C| >= fill_min: m = the lower median of C, A = { c in C : |c - m| <= tol(m) }, out[p] = m when |A| >= fill_min, else 0.  Filled values
 *     feed no other pixel.
 *   every other pixel: out[p] = 0.
 *   flags (flags_dev_out, one uint8 per pixel, may be NULL), exclusive and exhaustive: PR_DEPTH_UNMEASURED D0 == 0, out == 0; PR_DEPTH_KEPT
 *     out == D0 != 0; PR_DEPTH_SMOOTHED D0 != 0, out != 0, out != D0; PR_DEPTH_GATED D0 != 0, G == 0; PR_DEPTH_FLYING G != 0, F == 0;
 *     PR_DEPTH_FILLED D0 == 0, out != 0.
 *   pr_depth_filter_counts (counts_host, may be NULL): n[c] = the number of pixels with flag c; reserved = 0.
 * pr_depth_filter_describe (host only): fills and checks the parameters.  PR_ERR_INVALID with nothing written: min_mm, max_mm or tol_mm above
 * 2^31 - 1; max_mm != 0 and min_mm > max_mm; tol_permille > 1000; fly_min_support > 8; radius > PR_DEPTH_FILTER_MAX_RADIUS; fill_min != 0 with
 * radius == 0 or fill_min > (2 radius + 1)^2 - 1; a null out.  Every entry point checks its parameters against these rules (and reserved == 0).
 * depth_out_dev must not be depth_in_dev (a stencil): PR_ERR_INVALID.  Parameters, null pointers and the frame's size are checked before any
 * device is touched, and a refused call writes no output.  Synchronous, on the calling thread's context: the control words cleared, the stencil
 * kernel, one stream synchronise and one pinned read-back of the counts, no hipMemcpy on the path; the same frame gives the same bytes on every call.
 * pr_depth_fuse_host / pr_depth_filter_host: the same over host arrays, from the same shared code: the CPU twins the device is held to.
 * Not offered: a bilateral or mean filter (values would no longer be input values), speckle removal (pr_scene_segments_dev with min_pixels does
 * that), an asynchronous form.  Frames from different views are brought into one view by pr_depth_reproject_dev (below), not here. */
#define PR_DEPTH_FUSE_MAX           8
#define PR_DEPTH_FILTER_MAX_RADIUS  2
#define PR_DEPTH_UNMEASURED  0
#define PR_DEPTH_KEPT        1
#define PR_DEPTH_SMOOTHED    2
#define PR_DEPTH_GATED       3
#define PR_DEPTH_FLYING      4
#define PR_DEPTH_FILLED      5
typedef struct {
    uint32_t min_mm, max_mm;           /* the range gate; max_mm == 0: no upper gate                                                  */
    uint32_t tol_mm, tol_permille;     /* tol(d) = tol_mm + floor(d * tol_permille / 1000)                                            */
    uint32_t fly_min_support;          /* 0 .. 8 supporting neighbours needed to keep a pixel; 0 = stage off                          */
    uint32_t radius;                   /* 0 .. 2: the window's half-width; 0 = no median and no fill                                  */
    uint32_t fill_min;                 /* 0 = off; else 1 .. (2 radius + 1)^2 - 1 neighbours needed to fill a hole                    */
    uint32_t reserved;
} pr_depth_filter_params;      /* 32 B */
typedef struct {
    uint32_t n[6];                     /* pixels per flag code PR_DEPTH_UNMEASURED .. PR_DEPTH_FILLED                                 */
    uint32_t reserved[2];
} pr_depth_filter_counts;      /* 32 B */
int  pr_depth_filter_describe(uint32_t min_mm, uint32_t max_mm, uint32_t tol_mm, uint32_t tol_permille, uint32_t fly_min_support, uint32_t radius,
                              uint32_t fill_min, pr_depth_filter_params *out);
int  pr_depth_fuse_dev(const void *const *frames /* host array of n_frames device pointers */, uint32_t n_frames, int depth_is_i32, size_t n_px,
                       uint32_t min_frames, void *depth_out_dev, uint8_t *count_out_dev /* may be NULL */);
int  pr_depth_fuse_host(const void *const *frames /* host array of n_frames host pointers */, uint32_t n_frames, int depth_is_i32, size_t n_px,
                        uint32_t min_frames, void *depth_out, uint8_t *count_out /* may be NULL */);
int  pr_depth_filter_dev(const void *depth_in_dev, int depth_is_i32, size_t width, size_t height, const pr_depth_filter_params *params,
                         void *depth_out_dev, uint8_t *flags_dev_out /* may be NULL */, pr_depth_filter_counts *counts_host /* may be NULL */);
int  pr_depth_filter_host(const void *depth_in, int depth_is_i32, size_t width, size_t height, const pr_depth_filter_params *params,
                          void *depth_out, uint8_t *flags_out /* may be NULL */, pr_depth_filter_counts *counts_out /* may be NULL */);

/* ---- reprojection: depth frames of other cameras and bare point clouds into the depth frame of one target camera ---------------------------
 * Every stage above takes a depth frame of ONE camera.  A rig of calibrated depth cameras, a depth camera beside the colour camera in whose frame
 * a detector's boxes and masks live, and a scanner or LiDAR that delivers points have no such frame.  This stage makes it: up to
 * PR_REPROJECT_MAX_SOURCES sources, each a depth frame of another camera or a bare cloud, go sample by sample through a rigid transform and a
 * pinhole into a z-buffer of the target camera.  The output is a depth frame of the caller's depth type and goes unchanged into everything
 * that takes one.  All float32 arithmetic is without contraction, with correctly rounded division; from the depth and the footprint on, integers
 * only; every output byte is fixed by this text, on the device and on the host.
 *   target: width x height pixels, 1 <= width, height <= 65535 and width * height <= 2^26; intrinsics fx, fy, cx, cy (finite, fx, fy > 0); depth
 *     type uint16 or int32 (depth_is_i32).  A pixel's index is y * width + x; its centre is at its integer coordinates (pr_depth2cloud's rule).
 *   sources: a HOST table of 1 <= n_sources <= PR_REPROJECT_MAX_SOURCES pr_reproject_source records (they travel as kernel arguments; two may share a
 *     pointer).  kind PR_SRC_DEPTH_U16 / PR_SRC_DEPTH_I32: data = width x height depths (the target's limits), intrinsics fx, fy, cx, cy (finite,
 *     fx, fy > 0), n_points = 0.  kind PR_SRC_CLOUD: data = 1 <= n_points <= 2^26 pr_vec3 in metres; width, height and the intrinsics are not read.
 *     data is aligned to its element (2 or 4 bytes).  T: row-major 4 x 4 float32, source camera to target camera, finite, its last row exactly
 *     (0, 0, 0, 1), the translation in metres.  reserved = 0.
 *   sample of a frame source, pixel (x, y): D0 = the depth as unsigned 32-bit, a non-positive int32 is 0.  D0 == 0: no sample.  D0 > 2^28 - 1:
 *     the sample is counted `range`.  Otherwise z = (float)D0 / 1000.0f, p = (((float)x - cx) / fx * z, ((float)y - cy) / fy * z, z): the
 *     expression of pr_depth2cloud, so the cloud it makes of the frame gives the same samples bit for bit.
 *   sample of a cloud source: p = the point; a component that is not finite: counted `invalid`.
 *   transform: q.c = ((T[c][0] * p.x + T[c][1] * p.y) + T[c][2] * p.z) + T[c][3] for c = 0, 1, 2.  Counted `invalid` unless q is finite and q.z > 0.
 *   depth: df = floorf(q.z * 1000.0f + 0.5f).  Counted `range` unless lo <= df <= hi, compared exactly (df is an integer value or +inf), with
 *     lo = max(1, min_mm) and hi = the smallest of max_mm (when non-zero), 65535 for a uint16 output and 2^28 - 1.  d = (uint32_t)df.
 *   footprint: splat s in { 1, 2, 3 } is the side of the square of pixels a sample writes; h = 0.5f * (float)(2 - s), exactly 0.5, 0 or -0.5.
 *     u = q.x / q.z * fx + cx, v = q.y / q.z * fy + cy (the target's intrinsics); x0f = floorf(u + h), y0f = floorf(v + h).  Counted `outside` unless
 *     x0f > -4.0f && x0f < (float)width and likewise in y, compared in float before any conversion (a NaN fails).  The square is x0 .. x0 + s - 1
 *     by y0 .. y0 + s - 1, clipped to the frame; an empty intersection is counted `outside`.  s = 1: the nearest pixel; s = 2: the four pixels
 *     around the continuous position; s = 3: the nearest pixel and its 8 neighbours.
 *   z-buffer: key = (d << 3) | source_index (unsigned 32-bit); KEY[p] = the minimum over every sample whose square holds p: the nearest surface,
 *     the lowest source index on a tie.  A minimum depends on no order of sources, samples or launches.  Z[p] = KEY[p] >> 3, 0 where no sample
 *     landed; S[p] = KEY[p] & 7.
 *   visibility (optional; it takes out background seen through the gaps between foreground samples, which a sparse cloud or a magnifying
 *     reprojection leaves and which pr_depth_filter_dev cannot remove, those pixels being measured): tol(d) = tol_mm + floor(d * tol_permille / 1000)
 *     (depth conditioning's).  front(p) = the number of pixels q != p inside the frame with |qx - px| <= occl_radius, |qy - py| <= occl_radius,
 *     Z[q] != 0 and Z[q] + tol(Z[p]) < Z[p].  A measured pixel is hidden when occl_min_front > 0 and front(p) >= occl_min_front.  The stage reads
 *     only Z, over the whole frame.
 *   out[p] = Z[p] where Z[p] != 0 and p is not hidden, else 0 (a hidden pixel is a hole for pr_depth_filter_dev's fill).
 *   source_dev_out (one uint8 per pixel, may be NULL): S[p] of a kept pixel, PR_REPROJECT_HIDDEN of a hidden one, PR_REPROJECT_NONE where nothing
 *     landed.
 *   pr_reproject_counts (counts_host, may be NULL): per source samples, invalid, range, outside, drawn = samples - invalid - range - outside, and
 *     won = the kept pixels with that S; per frame covered (Z != 0), hidden, kept = covered - hidden; entries of sources beyond n_sources and
 *     reserved = 0.
 * pr_reproject_describe (host only): fills and checks the parameters.  PR_ERR_INVALID with nothing written: splat outside 1 .. 3; min_mm, max_mm or
 * tol_mm above 2^31 - 1; max_mm != 0 and min_mm > max_mm; tol_permille > 1000; occl_radius > PR_REPROJECT_MAX_RADIUS; occl_min_front != 0 with
 * occl_radius == 0 or occl_min_front > (2 occl_radius + 1)^2 - 1; a null out.  Every entry point checks its parameters against these rules (and
 * reserved == 0).
 * pr_depth_reproject_dev: PR_ERR_INVALID, with nothing written and before any device is touched, for a null table, entry pointer, parameter block
 * or output; counts, sizes or an alignment outside the limits above; an unknown kind; intrinsics that are not finite or not positive; a T that is
 * not finite or whose last row is not (0, 0, 0, 1); depth_out_dev equal to a source pointer.  Synchronous, on the calling thread's context:
 * three launches (the library-owned key plane set to 0xFFFFFFFF and the control words cleared; the scatter, an atomic minimum per pixel of a
 * sample's square; the resolve, a workgroup per 64 x 16 tile), one stream synchronise and one pinned read-back of the counts, which the tile that
 * finishes last writes; no hipMemset or hipMemcpy on the path.  The same call gives the same bytes every time.
 * pr_depth_reproject_host: the same over host arrays, from the same shared code: the CPU twin the device is held to.
 * Order of use: condition every source in its own view first (pr_depth_filter_dev with the flying-pixel stage: a flying pixel reprojected into
 * another view becomes a streak), reproject, then pr_depth_filter_dev with fill_min on the result closes rounding gaps and hidden pixels.
 * Not offered: triangulated (meshed) reprojection, lens distortion, colour, an asynchronous form. */
#define PR_REPROJECT_MAX_SOURCES  8
#define PR_REPROJECT_MAX_RADIUS   2
#define PR_SRC_DEPTH_U16  0
#define PR_SRC_DEPTH_I32  1
#define PR_SRC_CLOUD      2
#define PR_REPROJECT_HIDDEN  254
#define PR_REPROJECT_NONE    255
typedef struct {
    const void *data;                  /* the frame's depths or the cloud's pr_vec3 (device memory for _dev, host memory for _host)   */
    uint64_t n_points;                 /* a cloud's points; 0 for a frame                                                             */
    uint32_t kind;                     /* PR_SRC_*                                                                                    */
    uint32_t width, height;            /* a frame's size; not read for a cloud                                                        */
    uint32_t reserved;
    float    fx, fy, cx, cy;           /* a frame's intrinsics; not read for a cloud                                                  */
    float    T[16];                    /* row-major, source camera to target camera                                                   */
} pr_reproject_source;         /* 112 B */
typedef struct {
    uint32_t splat;                    /* 1 .. 3: the side of a sample's square                                                       */
    uint32_t min_mm, max_mm;           /* the gate on the reprojected depth; max_mm == 0: no upper gate but the depth type's          */
    uint32_t tol_mm, tol_permille;     /* tol(d) = tol_mm + floor(d * tol_permille / 1000)                                            */
    uint32_t occl_radius;              /* 0 .. 2: the visibility window's half-width                                                  */
    uint32_t occl_min_front;           /* 0 = off; else 1 .. (2 occl_radius + 1)^2 - 1 nearer neighbours that hide a pixel            */
    uint32_t reserved;
} pr_reproject_params;         /* 32 B */
typedef struct {
    struct { uint32_t samples, invalid, range, outside, drawn, won, reserved[2]; } source[PR_REPROJECT_MAX_SOURCES];      /* 32 B each */
    uint32_t covered, hidden, kept;
    uint32_t reserved[5];
} pr_reproject_counts;         /* 288 B */
int  pr_reproject_describe(uint32_t splat, uint32_t min_mm, uint32_t max_mm, uint32_t tol_mm, uint32_t tol_permille, uint32_t occl_radius,
                           uint32_t occl_min_front, pr_reproject_params *out);
int  pr_depth_reproject_dev(const pr_reproject_source *sources /* host table, device data pointers */, uint32_t n_sources, size_t width, size_t height,
                            float fx, float fy, float cx, float cy, int depth_is_i32, const pr_reproject_params *params, void *depth_out_dev,
                            uint8_t *source_dev_out /* may be NULL */, pr_reproject_counts *counts_host /* may be NULL */);
int  pr_depth_reproject_host(const pr_reproject_source *sources /* host table, host data pointers */, uint32_t n_sources, size_t width, size_t height,
                             float fx, float fy, float cx, float cy, int depth_is_i32, const pr_reproject_params *params, void *depth_out,
                             uint8_t *source_out /* may be NULL */, pr_reproject_counts *counts_out /* may be NULL */);

/* ---- scenes from point clouds: exact k nearest neighbours over the scene's own kd-tree, and a PCA normal per point -------------------------
 * Every other preparation starts from a depth frame; a sensor that delivers points (a scanner, a LiDAR, a merged or cropped cloud) has no pixel
 * grid for pr_get_normal's stencil.  These entries make the one missing array -- a normal per scene point -- from the points and the tree alone,
 * after which the scene is a pr_scene_nn with cam_magic = 0 like any other.  No counterpart in the reference.
 *
 * Neighbours of scene point i.  The scene is n >= 1 points in tree order; points must be finite (the entries do not check).  All float32
 * arithmetic is without contraction.
 *   candidates:   every j in [0, n), i itself included
 *   d2(i, j)    = ((dx*dx + dy*dy) + dz*dz) with dx = p_j.x - p_i.x, dy and dz likewise: the search's own expression and order (pcd_scene.h:88-91)
 *   admissible:   d2 <= r2, where r2 = max_radius * max_radius is computed ONCE in float32 by pr_cloud_describe (max_radius = INFINITY: no limit)
 *   the list:     the m_i = min(k, number admissible) smallest keys (d2, j), compared lexicographically, in ascending order -- a tie in distance
 *                 goes to the lower index, so the result does not depend on the order in which the tree is visited.  1 <= k <= PR_KNN_MAX_K.
 *   outputs:      idx[i*k + t] = the t-th neighbour, PR_KNN_NONE for t >= m_i;  d2[i*k + t] = its d2, 0.0f for an unused slot;  count[i] = m_i
 * The search is the ordered stackless walk of Scene_nn::query with `best` replaced by the current bound: r2 until the list holds k entries, then the
 * k-th d2; a far child is entered iff the distance to its box is <= the bound (<=, not <: an equal distance with a lower index still displaces).
 * The box distance adds its x, y, z terms in d2's order, which is what keeps it a lower bound of the float32 d2.
 *
 * Normal of point i, from its list.  float64 throughout, in list order, every product formed and then added (no contraction):
 *   c     = (sum over t of (double)p_jt) / m_i, per component
 *   S     = the six sums of (p_jt - c)(p_jt - c)^T: xx, xy, xz, yy, yz, zz (not divided by m_i)
 *   eigen:  the cyclic Jacobi of pr_plane_from_moments on S (V = I, PR_PLANE_MAX_SWEEPS, the 2^-56 stop), statement for statement
 *   lo    = the index of the smallest diagonal entry (the lowest index on a tie), mid = the same rule over the two that remain, hi = the last
 *   n     = column lo of V, negated iff ((n.x*v.x + n.y*v.y) + n.z*v.z) < 0 with v = (double)viewpoint - (double)p_i; each component rounded to
 *           float32 once
 * The point gets the normal (0, 0, 0) -- this library's "no normal" everywhere -- when m_i < min_neighbours (min_neighbours >= 3), or when
 * lambda_mid <= line_ratio * lambda_hi: the neighbours coincide or lie on a line (an all-zero S is that case too).  0 <= line_ratio < 1.
 * variation[i] (optional) = (float)(lambda_lo / ((lambda_lo + lambda_mid) + lambda_hi)), the surface variation; 0 where there is no normal.
 * pr_cloud_counts: the points, those with a normal, those with too few neighbours, the degenerate ones (the last three add up to the first).
 *
 * pr_cloud_describe: host only; PR_ERR_INVALID for k outside 1 .. PR_KNN_MAX_K, a max_radius that is NaN or not positive, min_neighbours < 3, a
 * line_ratio outside [0, 1) or a viewpoint that is not finite.
 * pr_cloud_knn_dev: over any built kd-tree scene (scene->normal is not read); d2_dev and count_dev may be NULL.  One lane per
 * scene point; its list lives in LDS as [entry][lane].
 * pr_cloud_normals_dev: the same walk with the normal formed in the same kernel from the list in LDS.  normal_dev_out may be the scene's own
 * normal array (the kernel reads points and tree only); the write is announced like every write through this library, so no cached form of a
 * scene that holds those normals survives it.  variation_dev_out and counts_out may be NULL.
 * pr_scene_nn_from_cloud_dev: pr_kdtree_build_dev on the points (reordered in place), then the normals in tree order; the caller fills a
 * pr_scene_nn with cam_magic = 0 from the three buffers.  nodes_dev_out: cap_nodes entries (2 n + 1 always suffice).
 * pr_cloud_knn_host / pr_cloud_normals_host: the same source on host points and a host pr_kdnode array (pr_kdtree_build), byte for byte.
 * pr_ppf_cloud_points_dev: the scene sample of the PPF vote from a kd-tree scene -- the points 0, stride, 2 stride, ... of tree order whose
 * normal has a non-zero component, in index order, point = pcd * 1000.0f per component, normal as it is.  Room for PR_PPF_MAX_SCENE_POINTS;
 * more than that: PR_ERR_INVALID with nothing emitted and *n_out = the number found (raise the stride).  stride >= 1.
 * Not offered: voxel down-sampling, radius-only (unbounded k) neighbourhoods.  Clouds are merged, and moved between sensor frames, on their way
 * into a depth frame by pr_depth_reproject_dev (above); a merged cloud as such is not offered. */
#define PR_KNN_MAX_K  32
#define PR_KNN_NONE   0xFFFFFFFFu
typedef struct {
    uint32_t k;                /* 1 .. PR_KNN_MAX_K                                                                                   */
    uint32_t min_neighbours;   /* >= 3: fewer admissible neighbours give no normal                                                    */
    float    max_radius;       /* metres (the scene's unit), > 0; INFINITY: no limit                                                  */
    float    r2;               /* max_radius * max_radius in float32, computed once by pr_cloud_describe                              */
    float    line_ratio;       /* [0, 1): lambda_mid <= line_ratio * lambda_hi gives no normal                                        */
    float    viewpoint[3];     /* normals face it                                                                                     */
} pr_cloud_params;             /* 32 B */
typedef struct { uint32_t points, with_normal, too_few, degenerate; } pr_cloud_counts;      /* 16 B */
int  pr_cloud_describe(uint32_t k, float max_radius, uint32_t min_neighbours, float line_ratio, const float viewpoint[3], pr_cloud_params *out);
int  pr_cloud_knn_dev(const pr_scene_nn *scene, const pr_cloud_params *params, uint32_t *idx_dev, float *d2_dev /* may be NULL */,
                      uint32_t *count_dev /* may be NULL */);
int  pr_cloud_normals_dev(const pr_scene_nn *scene, const pr_cloud_params *params, pr_vec3 *normal_dev_out, float *variation_dev_out /* may be NULL */,
                          pr_cloud_counts *counts_out /* may be NULL */);
int  pr_scene_nn_from_cloud_dev(pr_vec3 *pcd_dev, size_t n_points, int max_leaf, const pr_cloud_params *params, pr_vec3 *normal_dev_out,
                                pr_kdnode *nodes_dev_out, size_t cap_nodes, uint32_t *n_nodes, pr_cloud_counts *counts_out /* may be NULL */);
int  pr_cloud_knn_host(const pr_vec3 *pcd, size_t n_points, const pr_kdnode *nodes, size_t n_nodes, const pr_cloud_params *params, uint32_t *idx_out,
                       float *d2_out /* may be NULL */, uint32_t *count_out /* may be NULL */);
int  pr_cloud_normals_host(const pr_vec3 *pcd, size_t n_points, const pr_kdnode *nodes, size_t n_nodes, const pr_cloud_params *params,
                           pr_vec3 *normal_out, float *variation_out /* may be NULL */, pr_cloud_counts *counts_out /* may be NULL */);
int  pr_ppf_cloud_points_dev(const pr_scene_nn *scene, uint32_t stride, pr_vec3 *points_dev_out, pr_vec3 *normals_dev_out, uint32_t *n_out);

/* ---- sharding of a hypothesis batch over ranks (contiguous blocks) ---------------- */
void pr_shard_range(uint32_t n_items, uint32_t rank, uint32_t world, uint32_t *first, uint32_t *count);

/* ---- the job's one collective: gather of the solved transforms over RCCL / xGMI -- */
/* The reference is single-GPU (test.cpp:14).  Hypotheses are independent, so ranks never exchange data on the path itself;
 * the P/G x 72-byte RegistrationResult records of every rank are gathered once.  librccl is opened on first use.
 *   one process, one host thread per GPU:  pr_comm_init_all(G) once, then thread d: pr_set_device(d) ... pr_gather_results(...)
 *   one process per GPU:  rank 0 calls pr_comm_id and hands the 128 bytes to the others (any channel), all call pr_comm_init_rank */
#define PR_COMM_ID_BYTES 128
int pr_comm_id(unsigned char id_out[PR_COMM_ID_BYTES]);                                   /* ncclGetUniqueId */
int pr_comm_init_rank(const unsigned char id[PR_COMM_ID_BYTES], int rank, int world);     /* the calling thread's context becomes rank `rank` */
int pr_comm_init_all(int n_devices);                                                      /* shared contexts of devices 0..n-1, rank = device */
int pr_comm_rank(int *rank, int *world);
int pr_comm_destroy(void);
/* rank r sends its pr_shard_range(n_total, r, world) block (n_local records, device memory); recv_dev (root only, n_total
 * records) receives all blocks in global hypothesis order.  Enqueued on the context's stream: pr_sync / pr_memcpy_d2h order after it. */
int pr_gather_results(const pr_result *send_dev, uint32_t n_local, uint32_t n_total, int root, pr_result *recv_dev);

/* ---- options / instrumentation ----------------------------------------------------------------- */
/* pr_set_option names (all int; defaults in brackets).  None of them changes a result bit, except "points_per_block", which
 * selects the reduction tree and therefore the last bits of the sums (DESIGN.md "canonical tree").
 *   "solve"            [PR_SOLVE_HOST] PR_SOLVE_HOST = reference-style host solve per iteration, PR_SOLVE_DEVICE = loop on the device
 *   "points_per_block" [3072]  points per workgroup of the correspondence pass (multiple of 1024)
 *   "fused_solve"      [1]     the workgroup that delivers a hypothesis' last partial sum finalizes in the tail of the pass kernel instead of
 *                              a second launch: device solve = finalize + 6x6 solve there; host solve = the 29 totals stored into pinned host memory
 *   "pose_groups"      [0]     streams the batch is split over (1..4; 0 = 2): device solve = one group's solve tail under another's pass;
 *                              host solve = software pipeline (the host solves one group while another group's pass runs)
 *   "graph"            [1]     device solve, one pose group, synchronous path: replay the loop as a hipGraph
 *   "sub_batch"        [512]   asynchronous path: hypotheses per sub-batch (cache residency of the clouds)
 *   "overlap_pass"     [-1]    asynchronous path: the other slot's render may start after this pass of a slot's loop (-1 = chosen per batch)
 *   "raster_mode"      [0]     fused render: 0 = global atomicMin inside the pose's pixel box, 1 = LDS depth bands (synchronous path)
 *   "mesh_order"       [1]     asynchronous path: the raster reads a library-owned copy of the triangle buffer in spatial order (made once per
 *                              buffer, on its second batch in a row, checked against the caller's buffer by every batch; 36 bytes per triangle of device memory); 0 = the caller's buffer
 *   "tight_box"        [1]     asynchronous path: each hypothesis' pixel box is the hull of the mesh's projected vertices (a kernel over the library's
 *                              list of the buffer's distinct vertices, made and checked with the ordered copy; 16 bytes per distinct vertex) instead of
 *                              the hull of the projected corners of the mesh's box; 0 = the latter.  Same results either way
 *                              ("stat_tight_batches", read-only: asynchronous batches of this process that ran on tight boxes)
 *   "box_bands"        [1]     asynchronous path: a hypothesis' depth box interleaves four image rows column by column, so that a 64-byte segment
 *                              holds a 4x4-pixel patch and the raster's depth atomics make fewer requests; 0 = row-major boxes.  Same results either
 *                              way ("stat_band_batches", read-only: asynchronous batches of this process that ran on banded boxes; "box_pack",
 *                              read-only: the ints a box's slot is rounded up to)
 *   "resident_loop"    [1]     asynchronous path, projective scene, device solve with "fused_solve", no timed call: every pass of a sub-batch runs in
 *                              ONE launch, a workgroup per hypothesis that meets once per pass in LDS -- 512 lanes, two workgroups to a compute unit, for a sub-batch
 *                              with at least one hypothesis per compute unit, 1024 lanes for a smaller one ("loop_waves"); 0 = one launch per pass and pose group
 *                              everywhere.  Same results either way.  A plan whose blocks would need more than 64 KiB of LDS (over 127 blocks per hypothesis)
 *                              keeps the multi-launch loop ("stat_resident_batches", read-only: sub-batches of this process whose loop ran as one launch)
 *   "loop_lds_blocks"  [-1]    "resident_loop": blocks of "points_per_block" points at the head of every cloud that the workgroup keeps in its compute unit's LDS
 *                              over the whole loop instead of moving them through memory every pass; -1 = as many as fit in 160 KiB behind the loop's own
 *                              rows (four of 3072 points), 0 = none, n > 0 = at most n.  Same results either way ("stat_loop_lds_blocks", read-only: the
 *                              number the most recent such launch ran with)
 *   "loop_lds_tables"  [-1]    "resident_loop": the scene's column and row tables (width + height floats) are copied once per hypothesis into the
 *                              workgroup's LDS, behind the loop's rows and ahead of the cloud's blocks ("loop_lds_blocks" gets what is left), and two
 *                              of the three scene reads per point and pass come from there; 0 = from memory, 1 = in LDS whenever they fit beside the
 *                              rows, -1 = the library's choice (in LDS for 8-wave workgroups, in memory for 16-wave ones); other values are clamped
 *                              to -1 .. 1.  Same results either way ("stat_loop_lds_tables", read-only: the bytes of tables the most recent such
 *                              launch kept in LDS, 0 when it read them from memory)
 *   "loop_waves"       [0]     "resident_loop": wavefronts per workgroup, 16 (1024 lanes, one workgroup per compute unit) or 8 (512 lanes, two per
 *                              compute unit, each within 80 KiB of LDS); 0 = the library's choice, which is 16 for a sub-batch with fewer hypotheses
 *                              than the device has compute units; any other value is refused.  Same results either way ("stat_loop_waves",
 *                              read-only: what the most recent such launch ran with)
 *   "nn_stack"         [1]     kd-tree query: per-lane LDS stack (1) or the reference's stackless walk (0)
 *   "nn_compact"       [1]     stack query on 32-byte node records with 16-bit outward-rounded boxes (0: exact 64-byte records)
 *   "host_worker"      [1]     host solve: a batch given to pr_refine_submit runs on a library-owned helper thread of its slot (private context: its own
 *                              workspaces and scene caches -- about as much device memory again per slot in use); 0: inside the call, on the caller's thread
 *   "blocking_wait"    [0]     pr_refine_wait sleeps on the slot's event (hipEventBlockingSync) instead of spinning; takes effect for slots created afterwards
 *   "nn_wide"          [1]     queued tree searches walk 128-byte lines (wide nodes of eight subtree boxes, one line per leaf) in nearest-first
 *                              order; a query whose minimum is attained by more than one point is repeated by the ordered binary walk (0: binary walk only)
 *   "nn_seed"          [1]     compact records: start every search from the previous pass' / previous point's winner distance
 *   "nn_split"         [1]     compact records: the search runs in a kernel of its own (adjacent lanes = adjacent cloud points, a workgroup
 *                              takes "nn_run" [8] chunks of 256 points: 1..8, other values are clamped and read back clamped) and the pass gathers
 *                              its winners in canonical order
 *   "nn_count"         [0]     instrumented runs: the search kernel counts its work (pr_nn_counters)
 *   "nn_grid"          [1]     fused refinement with a kd-tree scene made from a depth image: scene points are also indexed by pixel
 *                              (first bounds, and an exact window scan once the bound is a few pixels wide)
 *   "nn_lds_nodes"     [1024]  stackless query inside the pass (plain and robust): leading nodes of the tree staged in LDS, 16 bytes each; negative = 0, at
 *                              most the tree, at most 8192 (128 KiB).  More than 4064 (64 KiB less the pass kernel's 512 static bytes) needs the device's
 *                              opt-in for dynamic LDS beyond 64 KiB, asked for once per device; where it is refused the launch stages 4064 and runs
 *   "nn_lds_records"   [0]     the same for the 64-byte records of the stack query without compact records: at most 504 beside 16-entry stacks, 248 beside
 *                              24-entry ones (stacks, records and the 512 static bytes together are 64 KiB: no opt-in on this route)
 *   "stat_nn_lds_nodes", "stat_nn_stack_depth"  (read-only) what the most recent kd-tree search INSIDE a pass (no "nn_split" search kernel) ran with,
 *                              after every limit above: entries or records staged (0 with compact records) and stack entries per lane, 0 = the
 *                              stackless walk.  "stat_nn_pass_launches" (read-only) counts those launches in this process; a replayed graph
 *                              reports what it captured and counts nothing.  Same results at every setting
 *   "profile"          [0]     see below;  "sample_period" [32]: profile 2 times one call in this many
 *   "scene_cache"      [1]     keep derived scene data between calls (see "Caches" at the top)
 *   "pose_dist_chunk"  (read-only) model points a workgroup of pr_pose_distance stages at a time: where its point loop has its seams
 *   "ppf_walk"         [1]     pr_ppf_vote[_multi]: 1 = a wavefront walks the buckets of its 64 scene pairs together (entry t of their concatenation goes to lane
 *                              t % 64, so lanes stay busy whatever the bucket lengths), 0 = every lane walks its own pair's bucket.  Same bytes either way */
int  pr_set_option(const char *name, int value);
int  pr_get_option(const char *name, int *value);
/* HIP-event timing of the correspondence kernel on the library stream: option "profile" = 1 times every launch (all calls run
 * synchronously as one pose group), 2 does so for one call in `sample_period` (the other calls are unaffected), 3 times every launch
 * of pr_refine_submit batches WITHOUT making them synchronous: a timed batch renders under the other slot's loop as usual, its own loop
 * waits until the other slot's batch is complete, runs as one pose group and holds the other slot's next render back until it has
 * finished -- the timed launches have the chip to themselves, the figures appear with that batch's pr_refine_wait.
 * Accumulated since the last reset: launches timed, model points they processed, and their algorithmic bytes (36 B/point on
 * the first pass of a cloud and on the score-only last pass, 48 B/point in between). */
/* Work counters of the kd-tree search kernel, collected while option "nn_count" is 1 (instrumented runs; SURVEY 8d "count its own
 * visits"): out[pass * 8 + k] for ICP passes 0..passes-1 (<= 64), k = 0 queries, 1 settled by the pixel window, 2 handed to the tree,
 * 3 pyramid descents, 4 tree nodes visited, 5 leaves scanned, 6 leaf points tested, 7 window cells read.  Reading resets the counters. */
int  pr_nn_counters(uint64_t *out, uint32_t passes);
int  pr_profile_reset(void);
int  pr_profile_read(double *kernel_ms, uint64_t *launches, uint64_t *points, uint64_t *algorithmic_bytes,
                     double *render_ms, double *cloud_ms);
/* The timed launches one by one, in microseconds, in the order they were read back (at most 8192 since the last reset): *n = how many
 * there are, the first min(*n, capacity) are copied.  What a min / median / max over the sampled launches is made from. */
int  pr_profile_launches(float *launch_us, uint32_t capacity, uint32_t *n);
/* A kd-tree correspondence pass is four kernels (search, bound + window, task walk, reduce over the winners: Scene_nn::query of
 * pcd_scene.h:60-136 inside thrust__pcd2Ab, icp.h:128-209).  Timed asynchronous batches (profile 3) put events between them:
 * part_ms[0..3] = accumulated time of each kernel, *passes = passes that contributed.  Reset by pr_profile_reset. */
int  pr_profile_nn(double part_ms[4], uint64_t *passes);
/* Audit entry: the 29 per-point terms of ONE correspondence pass -- thrust__pcd2Ab's Vec29f, icp.h:128-209: the 21
 * upper-triangle products J_i J_j row by row, the 6 products J_i r, r^2, and 1 -- for every point of one cloud, zeros where the query
 * found no correspondence.  update16 (a row-major 4x4, or NULL) is applied to the cloud first and written back, exactly as the fused pass
 * applies the pending update of the previous iteration (transform_pcd_cuda, icp.cu:142-153).  want_packed != 0 looks the projective scene
 * up through the packed 16-byte record the fused path uses.  contrib_host receives n_points x 29 floats.  A caller that adds the rows in
 * point order reproduces the reference's single-thread summation (icp.cpp:139-148), which the product kernel replaces by its fixed tree. */
int  pr_debug_contrib29(pr_vec3 *cloud_dev, uint32_t n_points, int scene_kind, const void *scene, const float *update16, int want_packed,
                        float *contrib_host);
/* Audit entry: pr_debug_contrib29 with the WEIGHTED terms of `robust` (pr_robust above) in contrib_host (n_points x 29: columns 0..26
 * weighted by the factor table, 27 and 28 plain).  corr_host, unless NULL, receives n_points x 8 floats: {dx, dy, dz, valid ? 1.0f : 0.0f,
 * nx, ny, nz, w} -- the correspondence the pass found for the point and its weight; rows are zero where there is no valid correspondence.
 * With PR_ROBUST_NONE contrib_host equals pr_debug_contrib29's bytes and w is written as 1.0f.  Null pointers with n_points > 0 and a bad
 * descriptor are PR_ERR_INVALID before any device is touched, with nothing written. */
int  pr_debug_robust_terms(pr_vec3 *cloud_dev, uint32_t n_points, int scene_kind, const void *scene, const float *update16, int want_packed,
                           const pr_robust *robust, float *contrib_host, float *corr_host);
/* Audit entry: pr_icp_information with the projective scene read through its packed 16-byte record when want_packed != 0 (the form the fused
 * calls use), as pr_debug_contrib29 selects it.  want_packed == 0 is pr_icp_information itself. */
int  pr_debug_icp_information(const pr_vec3 *clouds_dev, const uint32_t *offsets_host, uint32_t n_clouds, int scene_kind, const void *scene,
                              int want_packed, const pr_robust *robust_or_null, const float *centers_host, const float *radii_host,
                              pr_pose_info *info_host, pr_pose_eig *eig_host_or_null);
/* Audit entry: ONE iteration of icp.cu:178-212 for n hypotheses whose 29 sums are given (n x 29 floats in the pass's order: the 21
 * upper-triangle entries of A row by row, b[6], r^2, count).  on_device != 0: the wavefront iteration the fused pass tail and
 * icp_finalize_solve_kernel run (one wavefront per hypothesis); 0: the host-solve loop's iteration (needs no device).  state: in/out
 * (T, rmse, fitness as the previous iteration left them); update_out: n x 16 (the update E; zeros where the hypothesis stops);
 * finished_out: n x uint32 (1 = the hypothesis stops here). */
int  pr_debug_pose_iteration(const float *sums, const uint32_t *n_points, uint32_t n, pr_criteria crit, uint32_t iter, int on_device,
                             pr_result *state, float *update_out, uint32_t *finished_out);
/* Audit entry: the 29 sums of EVERY pass, as the product path delivered them to the host-solve loop.  Arms a recorder on the calling
 * thread (and so on the context that thread is bound to) for its next synchronous ICP call -- pr_icp_batch, pr_icp_batch_robust, pr_icp_proj,
 * pr_icp_nn, pr_refine_batch, pr_refine_batch_roi -- and for that call only: the recorder is gone when the call returns, error or not.
 * rows_host = NULL disarms.  While it is armed the loop copies the 29 floats of hypothesis i at iteration it to
 * rows_host[(it * n_hyp + i) * 29 ..], exactly what the iteration of icp.cu:178-212 is about to consume (layout: see
 * pr_debug_pose_iteration), whichever way the sums reached the host (options fused_solve, host_poll, pose_groups).  Rows of hypotheses
 * that are skipped (empty cloud) or already finished are not written: prefill the array to tell them apart.  The traced call returns
 * PR_ERR_INVALID before it launches anything when the solve is on the device (option solve), when its batch is not n_hyp hypotheses,
 * or when max_iteration + 1 > n_passes; nothing outside n_passes * n_hyp * 29 floats is ever written.  A traced call is one run of the
 * loop: a pr_icp_batch list of more than 32768 clouds, or a pr_refine_batch whose depth images do not fit one chunk (4 GiB), is refused
 * the same way.  Every other entry point (pr_refine_submit, pr_refine_batch_dev, the pyramid and multi calls) neither records nor
 * disarms: the recorder stays armed until one of the calls above, or a NULL call, takes it, and rows_host must stay alive until then.
 * Arming needs no device. */
int  pr_debug_trace_sums(float *rows_host, uint32_t n_hyp, uint32_t n_passes);
/* Audit entries (no device needed) for the library's ordered copy of a triangle buffer (option "mesh_order"): perm_out[k] = index of the
 * triangle the copy holds at place k -- a permutation of 0..n_tris-1, a pure function of the triangle data (Morton code of the
 * centroids, stable; non-finite centroids last) -- and the order-independent 64-bit fingerprint of a buffer (wrapping sum of a mixing
 * hash of each triangle's nine words) that every asynchronous batch re-derives from the caller's buffer on the device. */
int  pr_debug_mesh_order(const pr_triangle *tris_host, size_t n_tris, uint32_t *perm_out);
int  pr_debug_mesh_fingerprint(const pr_triangle *tris_host, size_t n_tris, uint64_t *fingerprint_out);
/* Audit entry (no device needed) for the tight pixel box of the asynchronous path (option "tight_box"): box_out = {x0, y0, x1, y1} in raster
 * coordinates (y not yet flipped: image row = height - 1 - y), inclusive, empty when x1 < x0 or y1 < y0 -- the hull of the projected
 * distinct vertices of the soup, padded by 2 pixels, intersected with the box of the projected corners of the mesh's axis-aligned box (the
 * loose box, which carries the frame and ROI clamps; loose_out, optional, receives it).  The same source as pose_tight_box_kernel, compiled
 * for the host: a vertex at or behind the camera plane (z <= 1e-3) or a non-finite coordinate leaves the loose box. */
int  pr_debug_tight_box(const pr_triangle *tris_host, size_t n_tris, const pr_mat4 *pose, const pr_mat4 *proj, uint32_t width, uint32_t height,
                        pr_roi roi, int32_t box_out[4], int32_t loose_out[4]);
/* Audit entry (no device needed) for the layout of a depth box in the asynchronous path's workspace (option "box_bands"): *slot_out = the ints
 * the pixel box `box` ({x0, y0, x1, y1}, raster coordinates, inclusive; inside a width x height frame, or empty) occupies, rounded up as the
 * packed layout rounds it (0 for an empty box), and offsets_out[i] = the int offset, from the start of that slot, of pixel (xs[i], image row
 * rows[i]) -- which must lie inside the box.  bands != 0: four consecutive image rows interleaved column by column, bands aligned to image rows;
 * 0: row-major, pitch = the box's width.  The same source as the kernels that fill, raster, count and emit a box, compiled for the host. */
int  pr_debug_box_layout(const int32_t box[4], uint32_t width, uint32_t height, int bands, const int32_t *xs, const int32_t *rows, size_t n,
                         uint32_t *slot_out, uint32_t *offsets_out);
/* Audit entry: the bytes the kd-tree searches would read for `scene` -- the traversal data the library derives from the caller's nodes and
 * points, copied to the host.  The scene is resolved exactly as an ICP call resolves it (the same cache sets, the same waiting for a batch
 * in flight that reads a set about to be rebuilt, the same rounds of wide levels): a read neither rebuilds what a search would have
 * reused nor the other way round.  cam_k = {fx, fy, cx, cy} with cam_w x cam_h is the camera of the pixel grid; cam_k == NULL: no grid is
 * reported (grid_w = grid_h = 0).  Every member of `out` may be NULL (skipped), and so may `out` itself -- a first call that only fills
 * `counts` tells how large the arrays have to be:
 *   topo   n_nodes x int4     leaf {first point, end point, -1, w}, internal {split value bits, child1, child2, w}; w = (parent + 1) | dim << 30
 *   bmin   n_nodes x float4   box minimum; .w = "size" of child1 (squared box diagonal, -1: a leaf).  bmax: the maximum, .w = size of child2
 *   rec64  n_nodes x 64 bytes {topo.x, topo.y, topo.z, dim | 0}, then child1's and child2's boxes {min.xyz, max.xyz} x 2
 *   rec32  n_nodes x 32 bytes {split | first point, child1 | dim << 30 (leaf: end point | 3 << 30), 12 x uint16 boxes in the frame info[2..7]}
 *   desc   n_nodes x 8 bytes  the first two words of rec32
 *   pts    n_points x float4  {x, y, z, 0}
 *   info   24 words           [0] depth [1] rec32 usable [2..4] frame origin [5..7] frame scale [8] wide usable [9] wide nodes
 *                             [16..18] wide frame origin [19] wide scale [20] wide frame admits the integer box test; the rest is the cache's
 *   wide   n_wide x 128 bytes the wide nodes in the paired layout of the task walk (n_wide = info[9])
 *   cell_idx  grid_w x grid_h x int32   point of a pixel, -1: none (with a camera only)
 *   grid   grid_cells x float4          {x, y, z, point index bits}: the pixels, then the three coarser levels (with a camera only)
 * grid_w = 0 also when the library builds no grid for this scene (no compact records, option nn_grid 0, more than 2^24 pixels);
 * grid_usable = every point owns a cell: the grid's contents mean nothing otherwise.  A tree the searches refuse (links that do not form a
 * tree) returns their error and writes nothing, `counts` included. */
typedef struct {
    uint32_t n_nodes, n_points, n_wide, grid_w, grid_h, grid_usable;
    uint64_t grid_cells;
} pr_nn_records_counts;
typedef struct {
    void *topo, *bmin, *bmax, *rec64, *rec32, *desc, *pts, *info, *wide, *cell_idx, *grid;
} pr_nn_records_out;
int  pr_debug_nn_records(const pr_scene_nn *scene, uint32_t cam_w, uint32_t cam_h, const float *cam_k, pr_nn_records_counts *counts,
                         const pr_nn_records_out *out);
/* Two things the library does silently for correctness, counted per context since it was created: asynchronous batches that
 * pr_refine_wait ran a SECOND time because the device-side checks found a stale model box, a triangle buffer whose content changed, or a scene array that no longer matches its
 * cached form (a caller who sees this grow writes to its buffers behind the library's back: pr_invalidate is the cheap cure), and timed
 * spans / batches whose HIP-event timing was dropped because an event could not be created or recorded (the work itself ran). */
int  pr_stats(uint64_t *batches_repeated, uint64_t *timings_dropped);
/* HIP-event time of the pr_gather_results exchanges issued while option "profile" was non-zero (events on the context's stream around
 * the grouped send / receive; accumulated since pr_profile_reset).  Waits for the stream.  New in this library -- the reference has
 * no multi-device code (test.cpp:14). */
int  pr_gather_profile(double *gather_ms, uint64_t *gathers);

#ifdef __cplusplus
}
#endif
#endif /* POSE_REFINE_H */
