// pr_runtime.h -- the host-side runtime behind the C ABI, shared by its translation units: contexts and their registry, workspaces, the write
// log of caller-owned memory, options, slots, profiling spans, and what every route of the fused batch path shares: its job record (RefineJob,
// make_job), the mesh argument and the grouped batch of the calls that take a mesh table (MeshArg, Batch), the layouts of a slot's pinned blocks, the pose-group lanes and the device-solve iteration loop.  pr_context.cpp (contexts, memory, options, profiling entry points),
// pr_scene.cpp (scene caches and device-side scene preparation), pr_icp.cpp (the batched ICP driver: device and host solve loops),
// pr_refine.cpp (render, cloud, the fused batch path with its two asynchronous slots and helper threads), pr_comm.cpp (RCCL gather).
#pragma once
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>          // types and prototypes only: librccl is opened on first use (pr_comm_*), never linked
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "pr_internal.h"
#include "pr_tuning.h"
#include "pose_box.h"
#include "contour_fit.h"

namespace prh {
extern thread_local std::string g_err;
void set_error(const char *fmt, ...);
}  // namespace prh

namespace prr {

using prh::set_error;

// PR_TRACE=<file>: host-side time stamps of the batch path (who waits for whom when a step stalls), dumped at process exit.  Off: one load and a branch.
void trace_mark(const char *tag);


#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            (void)hipGetLastError();          /* the runtime's sticky copy of this error must not be found by the next launch's check */ \
            return PR_ERR_HIP;                                                                  \
        }                                                                                       \
    } while (0)
#define PR_TRY(expr) do { int rc_ = (expr); if (rc_ != PR_OK) return rc_; } while (0)

struct DevBuf {                      // grow-only device workspace
    void *p = nullptr; size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return PR_OK;
        if (p) { hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); p = nullptr; return PR_ERR_NOMEM; }
        cap = want;
        return PR_OK;
    }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return static_cast<T *>(p); }
};
struct PinBuf {                      // grow-only pinned host staging; `dev` = the same bytes as kernels address them (stage_words / copy_words pull from and push to it)
    void *p = nullptr, *dev = nullptr; size_t cap = 0;
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return PR_OK;
        release();
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess && (e = hipHostGetDevicePointer(&dev, p, 0)) != hipSuccess) hipHostFree(p);
        if (e != hipSuccess) { set_error("hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e)); p = dev = nullptr; return PR_ERR_NOMEM; }
        cap = want;
        return PR_OK;
    }
    void release() { if (p) hipHostFree(p); p = dev = nullptr; cap = 0; }
    template <class T> T *as() const { return static_cast<T *>(p); }
    template <class T> T *dev_as() const { return static_cast<T *>(dev); }
};

// ---- which device ranges were written through this library, and when --------------------------------
// Derived data (the packed projective scene, the kd traversal records, the host copy of a model box) is cached by the address
// of the caller's buffers.  A cache entry remembers the write generation it was built at and is dropped as soon as a later
// write through the library (pr_memcpy_*, pr_fill_i32, pr_free, the *_prepare_dev / *_build_dev functions, pr_render) or a
// pr_invalidate() call overlaps one of its source ranges.  Writes the library cannot see (raw HIP calls, the caller's own
// kernels) must be announced with pr_invalidate -- include/pose_refine.h states that contract.
struct WriteLog {
    std::mutex mu;
    struct W { uintptr_t lo, hi; };
    static constexpr uint64_t kRing = 128;
    W ring[kRing];
    uint64_t gen = 0;                                            // writes recorded so far; write k (1-based) sits in ring[k % kRing]
    void note(const void *p, size_t bytes)
    {
        if (!p) return;
        uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
        if (bytes == 0) {                                        // unknown extent: the whole allocation that contains p
            void *base = nullptr; size_t size = 0;
            if (hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t *>(&base), &size, const_cast<void *>(p)) == hipSuccess && base) { lo = reinterpret_cast<uintptr_t>(base); hi = lo + size; }
            else { (void)hipGetLastError(); lo = 0; hi = ~(uintptr_t)0; }
        }
        std::lock_guard<std::mutex> lk(mu);
        ++gen;
        ring[gen % kRing] = W{ lo, hi };
    }
    uint64_t now() { std::lock_guard<std::mutex> lk(mu); return gen; }
    // may [p, p+bytes) have been written after generation `since`?
    bool written_since(uint64_t since, const void *p, size_t bytes)
    {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
        std::lock_guard<std::mutex> lk(mu);
        if (gen - since >= kRing) return true;                   // older writes have left the ring: assume the worst
        for (uint64_t k = since + 1; k <= gen; ++k) { const W &w = ring[k % kRing]; if (w.lo < hi && lo < w.hi) return true; }
        return false;
    }
};
extern WriteLog g_writes;
extern std::atomic<uint64_t> g_tight_batches;     // asynchronous batches whose pixel boxes came from pose_tight_box_kernel (process-wide; read-only option "stat_tight_batches": tests tell the tight path from the loose one by it)
extern std::atomic<uint64_t> g_band_batches;      // asynchronous batches whose depth boxes were banded (option box_bands; read-only option "stat_band_batches": tests tell the banded path from the row-major one by it)
extern std::atomic<uint64_t> g_resident_batches;  // asynchronous sub-batches whose whole loop ran as one launch (option resident_loop; read-only option "stat_resident_batches": tests tell the resident route from the multi-launch one by it)
extern std::atomic<uint32_t> g_loop_waves;        // wavefronts per workgroup of the most recent resident launch (option loop_waves; read-only option "stat_loop_waves")
extern std::atomic<uint32_t> g_loop_lds_tables;   // bytes of colf / rowf that the most recent resident launch kept in LDS, 0 when it read them from memory (option loop_lds_tables; read-only option "stat_loop_lds_tables")
extern std::atomic<uint32_t> g_loop_lds_blocks;   // blocks of every cloud's head that the most recent resident launch kept in LDS (option loop_lds_blocks; read-only option "stat_loop_lds_blocks": tests tell a launch with an LDS image from one that quietly ran without)
// what the most recent in-pass kd-tree launch (launch_icp_pass_nn: enqueued, or replayed in a cached graph) ran with, after nn_route and the launcher's own limits:
// nodes staged in LDS and stack entries per lane, 0 = the stackless walk (read-only options "stat_nn_lds_nodes", "stat_nn_stack_depth": tests tell a walk that
// read staged nodes from one that quietly staged none, or took another route); g_nn_pass_launches counts those launches (a captured graph notes whether it holds one)
extern std::atomic<uint32_t> g_nn_lds_nodes, g_nn_stack_depth;
extern std::atomic<uint64_t> g_nn_pass_launches;
extern std::atomic<uint64_t> g_flag_overtook;   // PR_SOLVE_HOST: group flags that reached the host before all of their rows (process-wide; expected 0; read-only option "stat_flag_overtook")

// ---- process-wide options (pr_set_option): plain ints, shared by every context ---------------------
constexpr int kSlots = PR_SLOTS;            // asynchronous slots per context (pr_tuning.h)
struct Options {
    int pose_groups = 0;             // split the batch over this many streams (1..4); 0 = two, for either scene kind (pose_groups_for below has the measurements);
                                     // launches of different groups overlap, so timed calls fall back to one group
    int solve_mode = PR_SOLVE_HOST;
    int host_worker = 1;             // PR_SOLVE_HOST batches of pr_refine_submit run on the slot's helper thread (0: on the caller's thread, inside the call)
    int steps = 3;                   // 1024-point steps per workgroup -> 3072 points per workgroup (round 3: 3-5 % faster than 2048 / 4096).  Round 6, with the write-back issued behind the gathers, option points_per_block = 4096 pipelines 2 % better (286.5 / 287.3 k against 280.6 / 281.4 k, 100 steps, same box; 273.6 against 271.6 k at 20 steps; 5120: 282 k, 6144: 277 k, 8192: 242-262 k; kd-tree and host solve within noise) but a LONE 256-hypothesis launch takes 39.6 instead of 37.7 us (six longer chains per hypothesis instead of eight): the default stays, the option is there (it selects another summation tree: a quarter of the bench's hypotheses end in a different basin, the oracle follows)
    int profile = 0;
    int sample_period = 32;          // profile 2: one timed (synchronous, single-group) call in this many
    int nn_lds_nodes = 1024;         // stackless walk in the pass: leading 16-byte topology entries staged in LDS (<= tree, <= 8192; beyond 4064 by the per-device opt-in of launch_icp_pass_nn)
    int nn_lds_records = 0;          // stack traversal: leading 64-byte node records staged in LDS; measured 0/64/128/256/512 -> 42.2/41.6/45.2/45.4/58.2 ms per step (occupancy lost to the extra LDS outweighs the saved L1 lookups).  Capped at 504 / 248 records beside 16- / 24-entry stacks (nn_route); tests/test_nn_lds_gpu.py runs 0, 1, 64, 127, 247-249, 255-257, 503-505 and 511-513
    int nn_seed = 1;                 // compact kd records: start every search from the previous pass' winner distance
    int nn_compact = 1;              // stack traversal: 32-byte node records with 16-bit outward-rounded child boxes (half the L1 traffic)
    int blocking_wait = 0;           // pr_refine_wait sleeps on the slot's event instead of spinning (set before the first asynchronous batch)
    int nn_wide = 1;                 // queued tree searches: order-free walk over 128-byte lines (eight subtree boxes per wide node, one line per leaf); ties go to the binary walk
    int nn_stack = 1;                // kd-tree query: per-lane LDS stack (1) or the reference's stackless walk (0)
    int nn_split = 1;                // kd-tree scenes on compact records: search kernel (runs of consecutive points, grid window) + winners pass
    int nn_run = 8;                  // 256-point chunks a workgroup of the search kernel walks (1..8).  Since the window scans left that kernel (round 4) it is a light
                                     // streaming pass and fewer, longer workgroups are a little better: 38.9 k (2) against 39.3 k (8) poses/s over five runs each
    int nn_grid = 1;                 // fused path: pixel grid of the scene points (seeds + window search); 0 = tree only
    int host_poll = 1;               // PR_SOLVE_HOST with the sums stored straight into pinned memory: 1 = the host polls ONE flag per pose group (stored by the workgroup that delivers the group's last hypothesis) and solves the group while its launch winds down; 0 = it waits for the stream, then solves the group (rounds 2-5)
    int nn_count = 0;                // instrumented runs: the search kernel counts its work per pass (pr_nn_counters)
    int start_overlap = -1;          // asynchronous path, a batch submitted while the other slot is idle: the pass after which the next batch's render may start.
                                     // -1 = the per-batch rule of a running pipeline.  Rounds 2-3 released the next render at pass 0 here; with the roofline
                                     // sample out of the timed region that reads 239 / 240 / 251 k against 253 / 253 / 256 k poses/s for the rule in three
                                     // alternating 20-step runs on one box: batches 1 and 2 then finish together and the third finds an empty chip
    int overlap_pass = -1;           // asynchronous path: the other slot's render may start once this slot has issued this pass of its loop; -1 = chosen per batch
                                     // (release_pass_for: with 13 passes to go while both slots' clouds fit the Infinity Cache, later by the render's weight when
                                     // they do not; kd-tree scenes: pass 0)
    int sub_batch = 512;             // asynchronous fused path: hypotheses per sub-batch (cache residency of the clouds)
    int fused_solve = 1;             // PR_SOLVE_DEVICE: the workgroup delivering a hypothesis' last partial sum also runs its finalize + solve (no second launch per iteration)
    int resident_loop = 1;           // asynchronous fused path, packed projective scene, fused device solve, untimed: all passes of a sub-batch in ONE launch, a workgroup per hypothesis (icp_loop_cu_kernel, 1024 lanes, or icp_loop_cu8_kernel, 512 lanes and two to a compute unit, for a sub-batch of at least one hypothesis per compute unit: option loop_waves; icp_pass.hip); 0 = the multi-launch loop everywhere.  Same bytes either way (profiles/resident_cu/README.md has the measurement)
    int loop_lds_tables = -1;        // resident loop: the scene's colf / rowf tables (width + height floats) copied once per hypothesis into the workgroup's LDS behind rows and header and ahead of the cloud's blocks, so that two of the three gathers per point and pass are LDS reads; 0 = read from memory (the kernel without the option), 1 = in LDS whenever they fit beside rows and header, -1 = the library's choice: in LDS for the 8-wave form, in memory for the 16-wave one.  Same bytes either way (profiles/loop_share/README.md has the measurement)
    int loop_waves = 0;              // resident loop: wavefronts per workgroup, 16 (one workgroup per compute unit) or 8 (two); 0 = the library's choice: 16 for a sub-batch with fewer hypotheses than the device has compute units, PR_LOOP_CU_FULL_CHIP_WAVES (pr_tuning.h) from there on.  Same bytes either way
    int loop_lds_blocks = -1;        // resident loop: blocks of every cloud's head kept in the workgroup's LDS over the whole loop instead of moving through memory every pass; -1 = as many as fit in the compute unit's 160 KiB behind rows and header (four of 3072 points), 0 = none (every instruction path of a pass is then the one without the option), n > 0 = at most n.  Same bytes either way (profiles/loop_lds/README.md has the measurement)
    int use_graph = 1;             // PR_SOLVE_DEVICE, single pose group only (the runtime serialises the branches of a captured multi-stream
                                     // graph, which forfeits the overlap): capture the whole iteration loop in a hipGraph and replay it
    int eager_streams = 1;           // asynchronous path: create the streams of both slots in one run (see slot_streams)
    int raster_mode = 0;             // fused path: 0 = global atomicMin inside the per-pose pixel box (reference scheme), 1 = LDS depth bands (int32); pr_set_option refuses anything else
    int mesh_order = 1;              // asynchronous fused path: raster the library's spatially ordered copy of the triangle buffer (ensure_model_box); 0 = the caller's buffer
    int tight_box = 1;               // asynchronous fused path: pixel boxes from the mesh's projected vertices (pose_tight_box_kernel over the library's list of distinct vertices, ensure_model_box) instead of the projected corners of its box; 0 = the latter
    int box_bands = 1;               // asynchronous fused path: a hypothesis' depth box interleaves four image rows column by column (pose_box.h, band_box: a 64-byte segment is a 4x4-pixel patch, fewer atomic requests per raster wave instruction); 0 = row-major boxes.  Same results either way
    int ppf_walk = 1;                // pr_ppf_vote: 1 = wave-cooperative bucket walk (a wavefront expands the buckets of its 64 scene pairs over its lanes), 0 = a lane per pair.  Same votes either way (profiles/ppf/README.md)
    int scene_cache = 1;             // keep the packed projective scene / kd traversal records of the latest scene between calls (pr_scene_invalidate)
};
extern Options opt;
// streams a batch is split over: the option, or two.  (Round 3 ran kd-tree scenes as three groups: with 8 workgroups per hypothesis and five
// waves per SIMD the search kernels left gaps a third group filled, +1.5 %.  With round 4's 12 workgroups and six waves two groups are
// enough and the third only costs launches: 34.4 / 34.9 k against 32.2 / 31.9 k poses/s on configs[2], same box; one group 29.8 k, four 31.2 k.
// Projective scenes with 16 hardware queues: three groups 174 k against 247 k.)
inline uint32_t pose_groups_for(int scene_kind) { (void)scene_kind; return opt.pose_groups > 0 ? (uint32_t)opt.pose_groups : 2u; }

// packed projective scene (one 16-byte record per pixel + the two back-projection tables) of the latest scene it was built for
// Its one allocation, in bytes: [w * h] float4 | colf[w] | rowf[h] | (on 16 bytes) ProjTail.  No HIP call in here: tools/job_sanitize.cpp checks it.
struct ProjTail { uint32_t exact; prk::FpWords fp; uint32_t pad[3]; };   // exact: the pcd array is what dep2pcd produces (pack_proj_scene_kernel); fp: of pcd and normal
static_assert(sizeof(ProjTail) == 32, "ProjTail: the 32 bytes behind the tables");
struct PackedLayout { size_t colf, rowf, tail, bytes; };
inline PackedLayout packed_layout(size_t w, size_t h)
{
    PackedLayout l{};
    l.colf = w * h * sizeof(float4); l.rowf = l.colf + w * sizeof(float);
    l.tail = l.colf + (((w + h) * sizeof(float) + 15) & ~(size_t)15); l.bytes = l.tail + sizeof(ProjTail);
    return l;
}
struct PackedCache {
    DevBuf rec;                      // as packed_layout(w, h) lays it out
    template <class T> T *at(size_t offset) const { return reinterpret_cast<T *>(static_cast<unsigned char *>(rec.p) + offset); }
    const void *pcd = nullptr, *normal = nullptr;
    uint64_t w = 0, h = 0; float k[4] = { 0, 0, 0, 0 }; uint32_t tl[2] = { 0, 0 };
    uint64_t gen = 0;
    bool valid = false, exact = false;
};
// ---- the description of one fused batch (render -> cloud -> ICP) -----------------------------------
// Everything of a batch but what varies from run to run (poses, their number, where the results go on the host), by value: the caller's
// structs may go away after pr_refine_submit returns, a slot's helper thread runs the batch later, and refine_wait runs it again when the
// model box it assumed turns out stale.  make_job builds it at the entry points; everything below them takes it as it is.
// (the raster packs pixel coordinates into 13 bits each and enumerates a triangle's candidate pixels with 24-bit arithmetic;
// contour.hip: kMaxFrameSide restates the 8192 -- its 32-bit per-workgroup sum is sized by it)
inline bool frame_size_ok(size_t W, size_t H)
{
    if (W > 8192 || H > 8192 || W * H > ((size_t)1 << 24)) { set_error("frames larger than 8192 on a side or 2^24 pixels are not supported (got %zux%zu)", W, H); return false; }
    return true;
}
// a frame as the frame stages' entry points take it (fn: the entry point's name): not empty, and of a size frame_size_ok lets pass
inline int frame_ok(const char *fn, size_t W, size_t H)
{
    if (W == 0 || H == 0) { set_error("%s: bad arguments (an empty frame)", fn); return PR_ERR_INVALID; }
    return frame_size_ok(W, H) ? PR_OK : PR_ERR_INVALID;
}
inline bool roi_ok(pr_roi roi, uint32_t W, uint32_t H)
{
    if (roi.width <= 0 || roi.height <= 0) return true;            // no ROI
    if (roi.x < 0 || roi.y < 0 || (size_t)roi.x + (size_t)roi.width > W || (size_t)roi.y + (size_t)roi.height > H) {
        set_error("roi out of image");                               // renderer.cu:202-203 asserts
        return false;
    }
    return true;
}
// pr_render, pr_render_span (span) and pr_render_multi's (multi) checks, all but a mixed batch's mesh table (plan_meshes), in the order and with the
// messages the three have always had: the frame's under pr_render's name, then -- for P > 0 -- the entry point's own arrays under its own; pr_render
// itself asks for its arrays with the frame.  An empty model has no array, no hypotheses need none.  No HIP call in here.
inline int render_args_ok(const char *fn, bool multi, bool span, const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses, size_t P, size_t W, size_t H,
                          const pr_mat4 *proj, pr_roi roi, const int32_t *near_dev, const int32_t *far_dev)
{
    const bool missing = P && (!poses || !near_dev || (span && !far_dev));
    if ((!multi && !tris_dev && n_tris > 0) || (missing && !multi && !span) || !proj || W == 0 || H == 0) { set_error("pr_render: bad arguments"); return PR_ERR_INVALID; }
    if (!frame_size_ok(W, H)) return PR_ERR_INVALID;
    if (!roi_ok(roi, (uint32_t)W, (uint32_t)H)) { set_error("pr_render: roi out of image"); return PR_ERR_INVALID; }
    if (missing) { set_error("%s: bad arguments", fn); return PR_ERR_INVALID; }
    if (multi && P > 0xffffffffull) { set_error("%s: more than 2^32 hypotheses", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
// A closest-point grid as a caller hands it over: every check that needs no device (make_job, make_scene, pr_scene_grid_build_dev; `built` = with the
// arrays the build fills in).  No HIP call in here.
inline int grid_desc_ok(const char *fn, const pr_scene_grid *gs, bool built)
{
    if (!gs) { set_error("%s: null pr_scene_grid", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(gs->cell) || !(gs->cell > 0.0f)) { set_error("%s: pr_scene_grid: cell must be finite and positive (got %g)", fn, (double)gs->cell); return PR_ERR_INVALID; }
    if (!(gs->inv_cell == 1.0f / gs->cell)) { set_error("%s: pr_scene_grid: inv_cell is not 1.0f / cell (pr_scene_grid_describe computes it)", fn); return PR_ERR_INVALID; }
    for (int a = 0; a < 3; ++a) if (!std::isfinite(gs->origin[a])) { set_error("%s: pr_scene_grid: origin[%d] is not finite", fn, a); return PR_ERR_INVALID; }
    uint64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        if (gs->dim[a] == 0 || gs->dim[a] > PR_GRID_MAX_CELLS) { set_error("%s: pr_scene_grid: dim[%d] = %u (1 .. PR_GRID_MAX_CELLS)", fn, a, gs->dim[a]); return PR_ERR_INVALID; }
        cells *= gs->dim[a];
        if (cells > PR_GRID_MAX_CELLS) { set_error("%s: pr_scene_grid: more than PR_GRID_MAX_CELLS = %u cells", fn, (uint32_t)PR_GRID_MAX_CELLS); return PR_ERR_INVALID; }
    }
    if (!std::isfinite(gs->max_dist_diff) || !(gs->max_dist_diff > 0.0f) || !std::isfinite(gs->reach) || !(gs->reach > 0.0f)) {
        set_error("%s: pr_scene_grid: max_dist_diff and reach must be finite and positive (got %g, %g)", fn, (double)gs->max_dist_diff, (double)gs->reach); return PR_ERR_INVALID;
    }
    if (built) {
        if (!gs->cell_point || !gs->rec) { set_error("%s: pr_scene_grid: cell_point or rec is null (pr_scene_grid_build_dev sets them)", fn); return PR_ERR_INVALID; }
        if (gs->n_points == 0 || gs->n_points >= (1u << 27)) { set_error("%s: pr_scene_grid: n_points must be 1 .. 2^27 - 1 (got %u)", fn, gs->n_points); return PR_ERR_INVALID; }
    }
    return PR_OK;
}
// A robust-weight descriptor as a caller hands it over (pr_robust, include/pose_refine.h): what pr_robust_describe would have produced.  No HIP call in here.
inline int robust_desc_ok(const char *fn, const pr_robust *rb)
{
    if (!rb) { set_error("%s: null pr_robust", fn); return PR_ERR_INVALID; }
    if (rb->kind > PR_ROBUST_CAUCHY) { set_error("%s: pr_robust: unknown kind %u", fn, rb->kind); return PR_ERR_INVALID; }
    if (rb->reserved != 0) { set_error("%s: pr_robust: reserved must be 0", fn); return PR_ERR_INVALID; }
    if (rb->kind == PR_ROBUST_NONE) return PR_OK;
    if (!std::isfinite(rb->c) || !(rb->c > 0.0f)) { set_error("%s: pr_robust: c must be finite and positive (got %g)", fn, (double)rb->c); return PR_ERR_INVALID; }
    if (!(rb->inv_c == 1.0f / rb->c) || !std::isfinite(rb->inv_c) || !(rb->inv_c > 0.0f)) { set_error("%s: pr_robust: inv_c is not the positive finite 1.0f / c (pr_robust_describe computes it)", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
// a robust table of a call with n_levels levels: one descriptor for all of them, or one each
inline int robust_table_ok(const char *fn, const pr_robust *robust, uint32_t n_robust, uint32_t n_levels)
{
    if (!robust) { set_error("%s: null pr_robust table", fn); return PR_ERR_INVALID; }
    if (n_robust != 1 && n_robust != n_levels) { set_error("%s: n_robust must be 1 or n_levels = %u (got %u)", fn, n_levels, n_robust); return PR_ERR_INVALID; }
    for (uint32_t l = 0; l < n_robust; ++l) PR_TRY(robust_desc_ok(fn, robust + l));
    return PR_OK;
}
// ---- mixed batches (pr_*_multi): the hypotheses of several meshes in one call ---------------------------------------------------
// The hypotheses grouped by mesh: a stable counting sort of the caller's indices.  Every mesh that has hypotheses is one group (in mesh
// order); the batch runs in group order and its outputs go back to the caller's order.  Results do not depend on how a batch is composed
// (each hypothesis equals its single-pose run), so the grouped batch gives every hypothesis what the single-mesh call gives it.
struct MeshPlan {
    std::vector<uint32_t> order;          // position in the grouped batch -> the caller's index
    std::vector<uint32_t> box;            // position -> its group (= which of the groups' model boxes it uses)
    std::vector<pr_mesh_ref> mesh;        // group -> mesh
    std::vector<uint32_t> start;          // group -> first position; one more entry: the batch size
};
// No HIP call in here (nor in MeshArg and Batch below): tools/job_sanitize.cpp runs them under ASan / UBSan.
inline int plan_meshes(const char *fn, const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index, size_t P, MeshPlan &pl)
{
    if (!meshes || n_meshes == 0 || !mesh_index) { set_error("%s: bad arguments (mesh table or mesh index missing)", fn); return PR_ERR_INVALID; }
    for (uint32_t m = 0; m < n_meshes; ++m)
        if (!meshes[m].tris_dev && meshes[m].n_tris > 0) { set_error("%s: mesh %u has %zu triangles and no array", fn, m, meshes[m].n_tris); return PR_ERR_INVALID; }
    std::vector<uint32_t> first(n_meshes + 1, 0);
    for (size_t i = 0; i < P; ++i) {
        if (mesh_index[i] >= n_meshes) { set_error("%s: mesh_index[%zu] = %u, but there are %u meshes", fn, i, mesh_index[i], n_meshes); return PR_ERR_INVALID; }
        first[mesh_index[i] + 1]++;
    }
    for (uint32_t m = 0; m < n_meshes; ++m) {
        if (first[m + 1] > 0) { pl.mesh.push_back(meshes[m]); pl.start.push_back(first[m]); }
        first[m + 1] += first[m];
    }
    pl.start.push_back((uint32_t)P);
    std::vector<uint32_t> group_of(n_meshes, 0);
    for (uint32_t k = 0, m = 0; m < n_meshes; ++m) if (first[m + 1] > first[m]) group_of[m] = k++;
    pl.order.resize(P); pl.box.resize(P);
    for (size_t i = 0; i < P; ++i) { const uint32_t j = first[mesh_index[i]]++; pl.order[j] = (uint32_t)i; pl.box[j] = group_of[mesh_index[i]]; }
    return PR_OK;
}
// the mesh as the C arguments name it: one triangle buffer for every hypothesis, or a mesh table and every hypothesis' index into it
struct MeshArg {
    const pr_triangle *tris = nullptr; size_t n_tris = 0;
    bool multi = false; const pr_mesh_ref *meshes = nullptr; uint32_t n_meshes = 0; const uint32_t *mesh_index = nullptr;
    static MeshArg one(const pr_triangle *tris_dev, size_t n_tris) { MeshArg a; a.tris = tris_dev; a.n_tris = n_tris; return a; }
    static MeshArg table(const pr_mesh_ref *meshes, uint32_t n_meshes, const uint32_t *mesh_index_host) { MeshArg a; a.multi = true; a.meshes = meshes; a.n_meshes = n_meshes; a.mesh_index = mesh_index_host; return a; }
};
// what model_boxes and render_chunk (pr_refine.cpp) draw: one mesh for every hypothesis, or a mixed batch in its plan's order
struct MeshSource { const pr_triangle *tris = nullptr; size_t n_tris = 0; const MeshPlan *plan = nullptr; };
// What every core runs on: the hypotheses in RUN order -- a mesh table's grouped by mesh, one mesh's as the caller has them -- and the way between that
// order and the caller's.  One mesh has no plan (it is not a one-group plan: its path keeps the single-mesh launches) and all four operations
// are the identity for it: gather hands the caller's pointer back, temp the caller's array, and a scatter of an array onto itself copies nothing.
struct Batch {
    bool mixed = false; MeshPlan pl;                             // a mesh table: the plan
    MeshSource src;                                              // as model_boxes and render_chunk take it
    size_t P = 0;
    const pr_mat4 *poses = nullptr;                              // in run order: the grouped copy, or the caller's pointer
    std::vector<pr_mat4> grouped;
    // a mesh table's checks and the grouping -- the one caller of plan_meshes -- and the poses in run order
    int make(const char *fn, const MeshArg &mesh, const pr_mat4 *poses_host, size_t n)
    {
        mixed = mesh.multi; P = n; src = MeshSource{ mesh.tris, mesh.n_tris, nullptr };
        if (mixed) { PR_TRY(plan_meshes(fn, mesh.meshes, mesh.n_meshes, mesh.mesh_index, n, pl)); src.plan = &pl; }
        poses = gather(poses_host, grouped);
        return PR_OK;
    }
    uint32_t caller(size_t j) const { return mixed ? pl.order[j] : (uint32_t)j; }          // position -> the caller's index ...
    const uint32_t *order() const { return mixed ? pl.order.data() : nullptr; }            // ... as a table for the device (null: the identity)
    std::vector<uint32_t> inverse() const { std::vector<uint32_t> where(P); for (size_t j = 0; j < P; ++j) where[caller(j)] = (uint32_t)j; return where; }   // the caller's index -> position
    // a per-hypothesis input in the caller's order -> run order (`store` keeps the copy)
    template <class T> const T *gather(const T *in, std::vector<T> &store) const
    {
        if (!mixed) return in;
        store.resize(P);
        for (size_t j = 0; j < P; ++j) store[j] = in[caller(j)];
        return store.data();
    }
    // where `count` records of a core land: a mixed batch's in a temporary, scattered once the call has succeeded (nothing reaches a caller's
    // array before); one mesh's straight in the caller's array
    template <class T> T *temp(std::vector<T> &store, size_t count, T *out) const { if (!mixed) return out; store.resize(count); return store.data(); }
    // per-hypothesis records back to the caller's order: `rows` blocks of P (the pyramid's [level][hypothesis]); out: null = not wanted
    template <class T> void scatter(const T *run, T *out, size_t rows = 1) const
    {
        if (!out || out == run) return;
        for (size_t r = 0; r < rows; ++r)
            for (size_t j = 0; j < P; ++j) out[r * P + caller(j)] = run[r * P + j];
    }
    // a P x P matrix back: rows and columns
    template <class T> void scatter_matrix(const T *run, T *out) const
    {
        if (!out || out == run) return;
        for (size_t a = 0; a < P; ++a)
            for (size_t b = 0; b < P; ++b) out[(size_t)caller(a) * P + caller(b)] = run[a * P + b];
    }
    Batch() = default;
    Batch(const Batch &) = delete;                               // (src.plan and poses point into pl and grouped)
};
struct RefineJob {
    MeshSource mesh;                                             // one mesh, or a mixed batch in its plan's order (Batch::src; synchronous calls only: the batch lives on the entry point's stack)
    uint32_t W = 0, H = 0; pr_mat4 proj{}; float K[9] = { 0 };
    int scene_kind = 0; pr_scene_proj_crop sp{}; pr_scene_nn sn{}; pr_scene_grid sg{}; pr_criteria crit{}; pr_roi roi{ 0, 0, 0, 0 };
    pr_result *results_dev = nullptr;
    pr_robust robust[PR_PYRAMID_MAX_LEVELS] = {};                // robust weight per pyramid level ([0]: a call without levels); all PR_ROBUST_NONE unless a _robust entry point set them (synchronous calls only)
    const void *scene() const { return scene_kind == PR_SCENE_NN ? static_cast<const void *>(&sn) : scene_kind == PR_SCENE_GRID ? static_cast<const void *>(&sg) : &sp; }   // as make_scene takes it (a crop starts with the plain view)
};
// ... from the C arguments, with every check that needs no device.  No HIP call in here: tools/job_sanitize.cpp runs it under ASan / UBSan.
inline int make_job(const char *fn, const pr_triangle *tris_dev, size_t n_tris, uint32_t W, uint32_t H, const pr_mat4 *proj, const float K[9], int scene_kind,
                    const void *scene, pr_criteria crit, pr_roi roi, pr_result *results_dev, RefineJob &job,
                    const pr_robust *robust = nullptr, uint32_t n_robust = 0, uint32_t n_levels = 1)      // robust: null (plain), or a table for n_levels levels
{
    if (n_levels == 0 || n_levels > PR_PYRAMID_MAX_LEVELS) { set_error("%s: bad arguments", fn); return PR_ERR_INVALID; }
    if (robust || n_robust) PR_TRY(robust_table_ok(fn, robust, n_robust, n_levels));
    if ((!tris_dev && n_tris > 0) || !proj || !K || !scene || W == 0 || H == 0) { set_error("%s: bad arguments", fn); return PR_ERR_INVALID; }   // (an empty model has no array)
    if (scene_kind != PR_SCENE_NN && scene_kind != PR_SCENE_PROJ && scene_kind != PR_SCENE_PROJ_CROP && scene_kind != PR_SCENE_GRID) { set_error("unknown scene kind %d", scene_kind); return PR_ERR_INVALID; }
    if (scene_kind == PR_SCENE_GRID) PR_TRY(grid_desc_ok(fn, static_cast<const pr_scene_grid *>(scene), /*built=*/true));
    if (!frame_size_ok(W, H) || !roi_ok(roi, W, H)) return PR_ERR_INVALID;
    if (crit.max_iteration < 0) { set_error("max_iteration must be >= 0"); return PR_ERR_INVALID; }
    job = RefineJob();
    job.mesh = MeshSource{ tris_dev, n_tris, nullptr }; job.W = W; job.H = H; job.proj = *proj; std::memcpy(job.K, K, sizeof job.K);
    job.scene_kind = scene_kind; job.crit = crit; job.roi = roi; job.results_dev = results_dev;
    if (scene_kind == PR_SCENE_NN) job.sn = *static_cast<const pr_scene_nn *>(scene);
    else if (scene_kind == PR_SCENE_GRID) job.sg = *static_cast<const pr_scene_grid *>(scene);
    else if (scene_kind == PR_SCENE_PROJ_CROP) job.sp = *static_cast<const pr_scene_proj_crop *>(scene);
    else job.sp.view = *static_cast<const pr_scene_proj *>(scene);     // (a plain projective scene: a crop at 0, 0)
    if (robust) for (uint32_t l = 0; l < n_levels; ++l) job.robust[l] = robust[n_robust == 1 ? 0 : l];
    return PR_OK;
}
// ---- the description of one scoring call (pr_score_poses, pr_score_overlap, pr_score_cover, pr_score_contours, pr_score_normals, pr_compose_detections and their _multi forms; pr_contour_information[_multi]) ----
// What the caller asked for, as the entry point got it; score_run (pr_refine.cpp) takes it from there.  Every member is set by the entry point.
enum ScoreKind { kScorePoses, kScoreOverlap, kScoreContours, kScoreNormals, kScoreCompose, kScoreCover, kScoreContourFit };
struct ScoreRequest {
    const char *fn; ScoreKind kind;                              // the entry point's name (for messages) and what it returns besides the scores
    MeshArg mesh;                                                // one mesh for every hypothesis, or a mesh table and every hypothesis' index into it
    const pr_mat4 *poses; uint32_t P, W, H; const pr_mat4 *proj; pr_roi roi;
    const void *scene; bool scene_i32; int32_t tau;
    pr_pose_score *scores;                                       // host, P records (kScoreContourFit: may be null)
    uint32_t *overlap;                                           // host, P x P (kScoreOverlap: required; kScoreContours, kScoreNormals: null = none)
    int32_t jump; const uint8_t *edge_dist; pr_pose_contour *contours;                          // kScoreContours: device distance image in, P host records out
    const float *K; uint32_t step; float cos_min; pr_pose_normal *normals;                      // kScoreNormals (with jump): intrinsics and the estimator's step in, P host records out
    const uint32_t *nearest; const prk::FitMeta *fit_meta; pr_contour_fit *fit; pr_pose_info *fit_info;      // kScoreContourFit (with jump and K): device nearest-edge map and P host centres (in the order of poses) in, P + P host records out
    uint16_t *labels_dev; int32_t *depth_dev; pr_pose_visible *visible; pr_frame_explained *frame;     // kScoreCompose: two optional device images, host records
    const uint32_t *cov_order; prk::CoverRule cov_rule; pr_pose_cover *cover; pr_cover_frame *cover_frame; uint32_t *selected, *n_selected;      // kScoreCover: the walk in (cov_rule.n_order indices), P + 1 host records and the selected list out
    const Batch *batch;                                          // score_run's, null from the entry point: the batch score_core runs on (poses: in its order)
};
// pr_score_overlap's own condition
inline int overlap_args_ok(const char *fn, uint32_t P, const uint32_t *overlap_host)
{
    if (P > PR_OVERLAP_MAX_POSES) {
        set_error("%s: %u hypotheses, but the overlap matrix is limited to PR_OVERLAP_MAX_POSES = %u (a 64 MB matrix)", fn, P, (uint32_t)PR_OVERLAP_MAX_POSES);
        return PR_ERR_INVALID;
    }
    if (P && !overlap_host) { set_error("%s: bad arguments (overlap_host is null)", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
// pr_score_cover's own conditions
inline int cover_args_ok(const ScoreRequest &r)
{
    PR_TRY(prh::cover_rule_ok(r.fn, r.cov_order, r.P ? r.cov_rule.n_order : 0, r.P, r.cov_rule.new_num, r.cov_rule.new_den));      // (no hypotheses: no walk)
    if (r.P && (!r.cover || !r.cover_frame || !r.selected || !r.n_selected)) {
        set_error("%s: bad arguments (cover_host, frame_host, selected_out or n_selected is null)", r.fn); return PR_ERR_INVALID;
    }
    return PR_OK;
}
// pr_compose_detections' own condition (its entry points ask before any device use as well)
inline int compose_args_ok(const char *fn, uint32_t P)
{
    if (P > PR_COMPOSE_MAX_POSES) {
        set_error("%s: %u hypotheses, but a label is a uint16: at most PR_COMPOSE_MAX_POSES = %u", fn, P, (uint32_t)PR_COMPOSE_MAX_POSES);
        return PR_ERR_INVALID;
    }
    return PR_OK;
}
// pr_score_normals' own conditions (its entry points ask for the first before any device use as well)
inline int normal_params_ok(const char *fn, uint32_t step, int32_t jump, float cos_min)
{
    if (step == 0 || step > PR_NORMAL_MAX_STEP) { set_error("%s: step must be 1 .. PR_NORMAL_MAX_STEP = %d (got %u)", fn, PR_NORMAL_MAX_STEP, step); return PR_ERR_INVALID; }
    if (jump < 0) { set_error("%s: jump_mm must be >= 0 (got %d)", fn, (int)jump); return PR_ERR_INVALID; }
    if (!(cos_min >= 0.0f && cos_min <= 1.0f)) { set_error("%s: cos_min must lie in [0, 1] (got %g)", fn, (double)cos_min); return PR_ERR_INVALID; }      // (a NaN fails both)
    return PR_OK;
}
// pr_contour_information's own condition on K (its entry points ask before any device use as well)
inline int fit_intrinsics_ok(const char *fn, const float *K)
{
    if (!K) { set_error("%s: bad arguments (K is null)", fn); return PR_ERR_INVALID; }
    for (int i = 0; i < 9; ++i) if (!std::isfinite(K[i])) { set_error("%s: K[%d] is not finite", fn, i); return PR_ERR_INVALID; }
    if (K[0] == 0.0f || K[4] == 0.0f) { set_error("%s: K[0] and K[4] must not be 0", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
// Every check of a request that needs no device, in one order for all fourteen entry points (the mesh table of a mixed batch: Batch::make).  No HIP
// call in here: tools/job_sanitize.cpp runs it under ASan / UBSan.  A request without hypotheses needs no arrays.
inline int score_request_ok(const ScoreRequest &r)
{
    const char *fn = r.fn;
    if (r.kind == kScoreOverlap || ((r.kind == kScoreContours || r.kind == kScoreNormals) && r.overlap)) PR_TRY(overlap_args_ok(fn, r.P, r.overlap));
    if (r.kind == kScoreCompose) PR_TRY(compose_args_ok(fn, r.P));
    if (r.kind == kScoreCover) PR_TRY(cover_args_ok(r));
    if (r.tau < 0) { set_error("%s: tau_mm must be >= 0 (got %d)", fn, (int)r.tau); return PR_ERR_INVALID; }
    if (!r.proj || r.W == 0 || r.H == 0 || (r.P && (!r.poses || !r.scene || (!r.scores && r.kind != kScoreContourFit) || (!r.mesh.multi && !r.mesh.tris && r.mesh.n_tris > 0)))) {
        set_error("%s: bad arguments", fn); return PR_ERR_INVALID;
    }
    if (!frame_size_ok(r.W, r.H)) return PR_ERR_INVALID;
    if (!roi_ok(r.roi, r.W, r.H)) { set_error("%s: roi out of image", fn); return PR_ERR_INVALID; }      // renderer.cu:202-203 asserts
    if (r.kind == kScoreContours && r.jump < 0) { set_error("%s: jump_mm must be >= 0 (got %d)", fn, (int)r.jump); return PR_ERR_INVALID; }
    if (r.kind == kScoreContours && r.P && (!r.edge_dist || !r.contours)) { set_error("%s: bad arguments (edge_dist_dev or contours_host is null)", fn); return PR_ERR_INVALID; }
    if (r.kind == kScoreContourFit && r.jump < 0) { set_error("%s: jump_mm must be >= 0 (got %d)", fn, (int)r.jump); return PR_ERR_INVALID; }
    if (r.kind == kScoreContourFit && r.P && (!r.nearest || !r.fit || !r.fit_info || !r.fit_meta)) { set_error("%s: bad arguments (nearest_dev, fit_host or info_host is null)", fn); return PR_ERR_INVALID; }
    if (r.kind == kScoreContourFit) PR_TRY(fit_intrinsics_ok(fn, r.K));
    if (r.kind == kScoreNormals) PR_TRY(normal_params_ok(fn, r.step, r.jump, r.cos_min));
    if (r.kind == kScoreNormals && r.P && (!r.K || !r.normals)) { set_error("%s: bad arguments (K or normals_host is null)", fn); return PR_ERR_INVALID; }
    if (r.kind == kScoreCompose && r.P && (!r.visible || !r.frame)) { set_error("%s: bad arguments (visible_host or frame_host is null)", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
// pr_pose_distance's checks, all of them: no device is touched before they pass (no HIP call in here).  *n_pairs_out = 0: nothing to do.
inline bool finite16(const pr_mat4 &m) { for (float v : m.m) if (!std::isfinite(v)) return false; return true; }
inline int pose_dist_args_ok(const pr_vec3 *points_dev, uint32_t n_points, const pr_mat4 *a, uint32_t n_a, const pr_mat4 *b, uint32_t n_b, int all_pairs,
                             const pr_mat4 *syms, uint32_t n_syms, const float *K, const pr_pose_dist *out, uint64_t *n_pairs_out)
{
    const char *fn = "pr_pose_distance";
    *n_pairs_out = 0;
    if (n_a > PR_POSE_DIST_MAX_POSES || n_b > PR_POSE_DIST_MAX_POSES) {
        set_error("%s: %u x %u poses, but a side is limited to PR_POSE_DIST_MAX_POSES = %u", fn, n_a, n_b, (uint32_t)PR_POSE_DIST_MAX_POSES); return PR_ERR_INVALID;
    }
    if (n_syms > PR_POSE_DIST_MAX_SYMS) { set_error("%s: %u symmetry transforms, at most PR_POSE_DIST_MAX_SYMS = %u", fn, n_syms, (uint32_t)PR_POSE_DIST_MAX_SYMS); return PR_ERR_INVALID; }
    if (!all_pairs && n_a != n_b) { set_error("%s: %u poses against %u without all_pairs", fn, n_a, n_b); return PR_ERR_INVALID; }
    const uint64_t n_pairs = all_pairs ? (uint64_t)n_a * n_b : n_a;
    if (n_pairs == 0) return PR_OK;
    if (n_points == 0 || n_points > PR_POSE_DIST_MAX_POINTS) { set_error("%s: n_points must be 1 .. PR_POSE_DIST_MAX_POINTS = %u (got %u)", fn, (uint32_t)PR_POSE_DIST_MAX_POINTS, n_points); return PR_ERR_INVALID; }
    if (!points_dev || !a || !b || !out || (n_syms && !syms)) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    for (uint32_t i = 0; i < n_a; ++i) if (!finite16(a[i])) { set_error("%s: a_host[%u] has a non-finite entry", fn, i); return PR_ERR_INVALID; }
    for (uint32_t i = 0; i < n_b; ++i) if (!finite16(b[i])) { set_error("%s: b_host[%u] has a non-finite entry", fn, i); return PR_ERR_INVALID; }
    for (uint32_t i = 0; i < n_syms; ++i) if (!finite16(syms[i])) { set_error("%s: syms_host[%u] has a non-finite entry", fn, i); return PR_ERR_INVALID; }
    if (K) {
        for (int i = 0; i < 9; ++i) if (!std::isfinite(K[i])) { set_error("%s: K[%d] is not finite", fn, i); return PR_ERR_INVALID; }
        if (K[0] == 0.0f || K[4] == 0.0f) { set_error("%s: K[0] and K[4] must not be 0", fn); return PR_ERR_INVALID; }
    }
    *n_pairs_out = n_pairs;
    return PR_OK;
}
// pr_pose_vsd / pr_pose_vsd_multi's checks, all but a mixed batch's mesh table (plan_meshes, which needs no device either): no device is touched
// before they pass (no HIP call in here; tools/job_sanitize.cpp runs it under ASan / UBSan).  multi: a mesh table instead of tris_dev, pairs only.
inline int vsd_args_ok(const char *fn, bool multi, const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *est, uint32_t n_est, const pr_mat4 *gt, uint32_t n_gt,
                       uint32_t W, uint32_t H, const pr_mat4 *proj, const void *scene, const float *K, float delta, const float *taus, uint32_t n_taus,
                       const pr_vsd_counts *out)
{
    if (n_gt != n_est && (multi || n_gt != 1)) { set_error("%s: %u estimates against %u truths (as many of each%s)", fn, n_est, n_gt, multi ? "" : ", or one truth"); return PR_ERR_INVALID; }
    if (n_est > 0x7fffffffu) { set_error("%s: more than 2^31 - 1 pairs", fn); return PR_ERR_INVALID; }
    if (n_taus > PR_VSD_MAX_TAUS) { set_error("%s: %u taus, at most PR_VSD_MAX_TAUS = %d", fn, n_taus, PR_VSD_MAX_TAUS); return PR_ERR_INVALID; }
    if (!(delta >= 0.0f) || !std::isfinite(delta)) { set_error("%s: delta_mm must be finite and >= 0", fn); return PR_ERR_INVALID; }
    for (uint32_t k = 0; taus && k < n_taus; ++k) {
        if (!(taus[k] >= 0.0f) || !std::isfinite(taus[k])) { set_error("%s: taus_mm[%u] must be finite and >= 0", fn, k); return PR_ERR_INVALID; }
        if (k && taus[k] < taus[k - 1]) { set_error("%s: taus_mm must not decrease (entry %u)", fn, k); return PR_ERR_INVALID; }
    }
    if (K) {
        for (int i = 0; i < 9; ++i) if (!std::isfinite(K[i])) { set_error("%s: K[%d] is not finite", fn, i); return PR_ERR_INVALID; }
        if (K[0] == 0.0f || K[4] == 0.0f) { set_error("%s: K[0] and K[4] must not be 0", fn); return PR_ERR_INVALID; }
    }
    if (W == 0 || H == 0) { set_error("%s: bad arguments (an empty frame)", fn); return PR_ERR_INVALID; }
    if (!frame_size_ok(W, H)) return PR_ERR_INVALID;
    if (n_est == 0) return PR_OK;
    if (!proj || !est || !gt || !scene || !out || (n_taus && !taus) || (!multi && !tris_dev && n_tris > 0)) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    for (uint32_t i = 0; i < n_est; ++i) if (!finite16(est[i])) { set_error("%s: est_host[%u] has a non-finite entry", fn, i); return PR_ERR_INVALID; }
    for (uint32_t i = 0; i < n_gt; ++i) if (!finite16(gt[i])) { set_error("%s: gt_host[%u] has a non-finite entry", fn, i); return PR_ERR_INVALID; }
    return PR_OK;
}
// pr_pose_penetration / pr_pose_penetration_multi's checks, all but a mixed batch's mesh table (plan_meshes): no device is touched before they pass (no
// HIP call in here).  The near and far boxes of all P hypotheses are resident together: 2 P renders within the bound depth_chunk (pr_refine.cpp) keeps.
uint32_t depth_chunk(size_t img, uint32_t P);
inline int penetration_args_ok(const char *fn, bool multi, const pr_triangle *tris_dev, size_t n_tris, const pr_mat4 *poses, uint32_t P, uint32_t W, uint32_t H,
                               const pr_mat4 *proj, int32_t slack, const pr_pair_solid *out)
{
    if (slack < 0) { set_error("%s: slack_mm = %d must not be negative", fn, slack); return PR_ERR_INVALID; }
    if (P > PR_PENETRATION_MAX_POSES) { set_error("%s: %u hypotheses, at most PR_PENETRATION_MAX_POSES = %d", fn, P, PR_PENETRATION_MAX_POSES); return PR_ERR_INVALID; }
    if (W == 0 || H == 0) { set_error("%s: bad arguments (an empty frame)", fn); return PR_ERR_INVALID; }
    if (!frame_size_ok(W, H)) return PR_ERR_INVALID;
    if (P == 0) return PR_OK;
    const uint32_t fit = depth_chunk((size_t)W * H, 2 * P);
    if (fit < 2 * P) {
        set_error("%s: %u hypotheses are %u near and far renders of %ux%u resident together, the depth workspace holds at most %u", fn, P, 2 * P, W, H, fit);
        return PR_ERR_INVALID;
    }
    if (!proj || !poses || !out || (!multi && !tris_dev && n_tris > 0)) { set_error("%s: bad arguments (a null pointer)", fn); return PR_ERR_INVALID; }
    return PR_OK;
}
// A slot's pinned blocks, in bytes.  h_in, staged to the device by one kernel: poses | pixel boxes | offsets of the packed boxes.
// h_out, stored by the batch's last kernels: cloud sizes | result records | the word the device-side model-box check writes (1 = the
// assumed box or a scene cache was stale), each on a 64-byte line of its own.
struct SlotIn {
    size_t box, off, bytes;
    explicit SlotIn(size_t P) : box(sizeof(pr_mat4) * P), off(box + sizeof(int4) * P), bytes(off + sizeof(uint32_t) * P) {}
};
struct SlotOut {
    size_t res, flag, bytes;
    explicit SlotOut(size_t P) : res((P * sizeof(uint32_t) + 63) & ~(size_t)63), flag((res + sizeof(pr_result) * P + 63) & ~(size_t)63), bytes(flag + 64) {}
};
// The kd-tree workspace of a batch, in 32-bit words behind one base: winners | slack of the keep-the-winner test | queue 1 | queue 2 (8 B per
// entry) -- one entry each per cloud point, `span` = the largest start + count of the batch -- | kQCountStride queue counters for each of the P
// hypotheses; `bytes` carries 64 B of slack.  No HIP call in here: tools/job_sanitize.cpp runs it under ASan / UBSan.
struct NNLayout { size_t winners, slack, queue, queue2, qcount, bytes; };
inline NNLayout nn_layout(size_t span, size_t P)
{
    static_assert(prk::kNNWordsPerPoint == 1 + 1 + 2 + 2, "winner | slack | queue 1 entry | queue 2 entry");
    NNLayout l{};
    l.slack = l.winners + span; l.queue = l.slack + span; l.queue2 = l.queue + 2 * span; l.qcount = l.queue2 + 2 * span;
    l.bytes = sizeof(uint32_t) * (l.qcount + prk::kQCountStride * P) + 64;
    return l;
}
// the nn_* fields of a batch whose workspace starts at `base`
inline void nn_carve(prk::IcpBatch &b, uint32_t *base, const NNLayout &l)
{
    b.nn_prev = base + l.winners; b.nn_slack = reinterpret_cast<float *>(base + l.slack);
    b.nn_queue = reinterpret_cast<uint2 *>(base + l.queue); b.nn_queue2 = reinterpret_cast<uint2 *>(base + l.queue2); b.nn_qcount = base + l.qcount;
}
// ---- the sizes of one asynchronous batch, from the host's pixel boxes alone -------------------------------------------------------------
// What refine_submit_async needs before anything of the batch has run: the capacity of a cloud, the grid of the passes, the sub-batch split and
// where every box sits in its sub-batch's depth workspace.  No HIP call in here: tools/job_sanitize.cpp runs it under ASan / UBSan.
struct AsyncPlan {
    size_t max_area, cstride;        // pixels of the largest box (at least 1), which bounds every cloud; the host's capacity bound per hypothesis, in points (the clouds themselves are packed: PoseMeta::start)
    uint32_t steps, nblk, grid_x;    // 1024-point steps per workgroup; blocks a hypothesis may have (capacity of the partial sums); workgroups per hypothesis
    uint32_t sub, n_sub;             // hypotheses per sub-batch, sub-batches
};
// the depth workspace's bound per hypothesis, in ints: a full-frame box and its rounding (banded boxes: the height rounded up to whole bands, pose_box.h "Capacity")
inline size_t depth_ints_per_pose(uint32_t W, uint32_t H, bool bands) { return (size_t)W * (bands ? (((size_t)H + 3) & ~(size_t)3) : (size_t)H) + prk::kBoxPack; }
// boxes: the P host-computed pixel boxes; box_off (P words out): box i at box_off[i] ints of its sub-batch's depth workspace, its own width as
// pitch (fill_box_kernel), or -- bands -- in the banded layout of pose_box.h (band_box) -- the offsets restart at every sub-batch
inline AsyncPlan plan_async(uint32_t P, uint32_t W, uint32_t H, const int4 *boxes, int opt_steps, int opt_sub_batch, uint32_t cloud_hint, uint32_t *box_off,
                            bool bands = false)
{
    AsyncPlan pl{};
    const size_t img = depth_ints_per_pose(W, H, bands) - prk::kBoxPack;
    pl.max_area = 1;
    for (uint32_t i = 0; i < P; ++i) pl.max_area = std::max<size_t>(pl.max_area, prk::box_area(boxes[i]));   // an off-screen pose has an empty box
    // capacity per hypothesis (a multiple of the packing's alignment, so that no sum of rounded sizes exceeds P x cstride)
    pl.cstride = prk::cloud_slot((uint32_t)pl.max_area);
    pl.steps = (uint32_t)std::max(1, opt_steps);
    const uint32_t ppb = pl.steps * prk::kPointsPerStep;
    pl.nblk = (uint32_t)((pl.max_area + ppb - 1) / ppb);       // bound from the pixel boxes: capacity of the partial sums
    // grid: one workgroup per block of the largest cloud of the previous batch (workgroups loop if this batch's clouds are
    // larger, surplus workgroups exit at once); the box bound itself would launch ~60 % empty workgroups (-2.5 % poses/s)
    pl.grid_x = cloud_hint ? std::min(pl.nblk, (cloud_hint + ppb - 1) / ppb) : pl.nblk;

    // Large batches run as consecutive sub-batches that reuse the same depth / cloud / partial-sum memory: the clouds of
    // <= 512 hypotheses (~140 MB touched) stay in the 256 MiB Infinity Cache over their 21 passes (1024 poses as one batch:
    // 199 k poses/s, as 2 x 512: see DESIGN.md)
    // ... and, for large frames, small enough that the depth workspace of a sub-batch stays within ~4 GiB (as the synchronous path
    // bounds its chunks) and the clouds within 2^30 points (offsets are 32-bit): 64 hypotheses per sub-batch at 4096 x 4096, all 512 up to 2 M pixels
    uint32_t sub_cap = (uint32_t)std::max(32, opt_sub_batch);
    sub_cap = (uint32_t)std::max<size_t>(1, std::min<size_t>({ (size_t)sub_cap, ((size_t)4 << 30) / (img * sizeof(int32_t)), ((size_t)1 << 30) / pl.cstride }));     // (2^30 cloud points per sub-batch: 12 GiB of clouds, 24 GiB of kd-tree search state at most)
    pl.n_sub = (P + sub_cap - 1) / sub_cap;
    pl.sub = pl.n_sub ? (P + pl.n_sub - 1) / pl.n_sub : 0;
    size_t acc = 0;
    for (uint32_t i = 0; i < P; ++i) {
        if (i % pl.sub == 0) acc = 0;
        box_off[i] = (uint32_t)acc;
        acc += prk::box_slot_of(boxes[i], H, bands);
    }
    return pl;
}
// When may the OTHER slot start rendering?  The pass of a (sub-)batch's loop behind which its render is released: a timed batch's last, else the
// options (start_overlap for a batch that starts a pipeline, overlap_pass), else the rule below.  No HIP call in here.
// Both phases are bound by the same units, so a batch that renders while the other slot is in the middle of its ICP loop
// slows that loop by more than it gains; its render is therefore held back until the other slot has issued this pass
// of its (last sub-batch's) loop -- late enough to disturb little, early enough that the GPU never idles.
inline uint32_t release_pass_for(size_t n_tris, uint32_t nq, uint32_t cloud_hint, pr_criteria crit, int scene_kind, bool timed, bool pipeline_start,
                                 int start_overlap, int overlap_pass)
{
    const uint32_t last_pass = (uint32_t)crit.max_iteration;
    if (timed) return last_pass;
    if (pipeline_start && start_overlap >= 0) return std::min(last_pass, (uint32_t)start_overlap);
    if (overlap_pass >= 0) return std::min(last_pass, (uint32_t)overlap_pass);
    // Measured optimum (21 passes of obj_06, overlap_pass swept per batch size):
    // pass 4 or earlier at 128 hypotheses, 9-10 at 256, 14-16 at 384, 16 at 512 -- i.e. when about 2800 hypothesis-passes of
    // this loop are left (never fewer than 5 passes): that much loop work is what a render hides behind without stretching the
    // passes it runs beside.  The render's own weight scales that figure: triangles per hypothesis against cloud points per
    // hypothesis (31 468 and 27 400 there; cloud_hint = the largest cloud of the previous batch).
    const double weight = ((double)std::max<size_t>(n_tris, 1) / 31468.0) * (27400.0 / (double)std::max(cloud_hint, 1000u));
    double left = std::max(5.0, 2800.0 * weight / (double)std::max(nq, 1u));   // passes of this sub-batch's loop still to run
    // Since the clouds are packed (end of round 4) a render disturbs the loop beside it less, as long as the clouds of BOTH slots stay in
    // the 256 MiB Infinity Cache: then the render is released with 13 passes to go (256 hypotheses: passes 5-9 give 272 k poses/s, the rule
    // above -- pass 10 -- 268 k; 384: pass 8 277 k against 272 k at 14; 512, whose two slots' clouds do not fit: 275 k at pass 16, 263 k at 10).
    if (2.0 * (double)nq * (double)std::max(cloud_hint, 1000u) * sizeof(pr_vec3) <= 240.0e6) left = std::max(left, 13.0);
    const double passes = (double)crit.max_iteration + 1.0;
    uint32_t auto_overlap = left >= passes ? 0u : (uint32_t)(passes - left + 0.5);
    // kd-tree scenes: the loop is seven times a render and its first passes are the heavy ones -- the other slot's render (and with it
    // that slot's own first passes) should start at once: 37.3 / 37.5 k against 36.0 k poses/s for the rule above (pass 1 / 2 / 3 / 6: 37.2 /
    // 37.2 / 37.1 / 37.0 k; 10: 35.7 k; 16: 34.0 k)
    if (scene_kind == PR_SCENE_NN) auto_overlap = 0u;
    return std::min(last_pass, auto_overlap);
}
// ---- kd-tree scenes: the two policies of make_scene (pr_scene.cpp).  No HIP call in here: tools/job_sanitize.cpp runs them under ASan / UBSan. ----
// Which of the sets of derived records a scene takes.  The caller states per set: valid; hit = it holds this scene and nothing says it is stale;
// same_arrays = it was derived from this scene's pcd and nodes arrays; in_flight = a batch in flight reads it; used = the clock of its latest use.
// In this order: the first hit; else a victim -- the first valid set of the same arrays (this scene, rewritten), the first invalid one, the least
// recently used one that no batch in flight reads, the least recently used of all (its readers then drain first).
struct NNSetFacts { bool valid, hit, same_arrays, in_flight; uint64_t used; };
struct NNSetPick { int set; bool hit; };
inline NNSetPick pick_nn_set(const NNSetFacts *f, int n)
{
    for (int i = 0; i < n; ++i) if (f[i].hit) return { i, true };
    for (int i = 0; i < n; ++i) if (f[i].valid && f[i].same_arrays) return { i, false };
    for (int i = 0; i < n; ++i) if (!f[i].valid) return { i, false };
    int pick = -1;
    for (int i = 0; i < n; ++i) if (!f[i].in_flight && (pick < 0 || f[i].used < f[pick].used)) pick = i;
    if (pick < 0) { pick = 0; for (int i = 1; i < n; ++i) if (f[i].used < f[pick].used) pick = i; }
    return { pick, false };
}
// How a set's records are searched, from its control words and the options nn_lds_nodes, nn_lds_records, nn_stack, nn_compact, nn_wide.
// Pending far children on the stack never exceed the tree depth; deeper trees use the stackless walk.  The caller has refused an inconsistent tree (depth >= 0x7fffffff).
// topo_nodes: what a stackless walk of this set stages whatever the route says -- a robust pass without compact records walks stackless beside any stack_depth.
struct NNRoute { uint32_t lds_nodes, stack_depth; bool compact, wide; uint32_t topo_nodes; };   // compact: the 32-byte records (SceneNNDev::rec32); wide: the wide records as well
inline NNRoute nn_route(const prk::NNInfo &info, uint32_t n_nodes, int nn_lds_nodes, int nn_lds_records, int nn_stack, int nn_compact, int nn_wide)
{
    NNRoute r{};
    r.lds_nodes = r.topo_nodes = std::min<uint32_t>(std::min((uint32_t)std::max(0, nn_lds_nodes), n_nodes), prk::kNNLdsNodesMax);      // <= 128 KiB of LDS (beyond 64 KiB: launch_icp_pass_nn opts in)
    if (nn_stack) r.stack_depth = (info.depth <= 16) ? 16u : ((info.depth <= 24) ? 24u : 0u);
    // stacks + records + the pass kernel's static LDS <= 64 KiB: 504 records beside 16 entries, 248 beside 24 (no opt-in on this route)
    if (r.stack_depth) r.lds_nodes = std::min<uint32_t>({ (uint32_t)std::max(0, nn_lds_records), n_nodes, (65536u - prk::kPassStaticLds - r.stack_depth * 2048u) / 64u });
    r.compact = r.stack_depth && nn_compact && info.rec32_valid == 1u;
    r.wide = r.compact && nn_wide && info.wide_state == prk::kWideValid && info.n_wide > 0u;
    return r;
}
// ---- profiling spans: pooled HIP events around launches, turned into the context's accounts -------------------------------------------
// One recorder for the context's own stream (SpanGuard) and one per asynchronous slot (a TIMED batch, option profile = 3).  A span is a start /
// stop pair in enqueue order; a kd-tree pass may carry three marks between its four kernels.  drain() -- once the stream has been waited for --
// adds every span to the calling thread's context (render_ms, cloud_ms, icp_ms, icp_launches, icp_points, icp_bytes, the launch list, the
// kd-tree parts) and hands the events back to the pool.
// Failure policy, the same for both owners: a failed event call costs the SPAN it belongs to (failed marks: the span's kd-tree parts), dropped
// and counted once (pr_stats) -- never the launches between the events: the batch itself always runs.  (HIP_TRY would clear the sticky error
// and return: the span is dropped HERE instead.)
enum { kSpanIcp = 0, kSpanRender = 1, kSpanCloud = 2 };
constexpr size_t kNoEvent = (size_t)-1;
// algorithmic bytes per point of a correspondence pass: 12 read + 24 gathered, + 12 written back once a transform is pending; an EDGE
// pass -- the first, or a score-only last one, which needs the scene point but not its normal (12 + 12 + 12) -- moves 36
inline uint64_t icp_span_bytes(uint64_t points, bool edge) { return points * (edge ? 36u : 48u); }
struct Spans {
    struct Span { size_t e0, e1; int kind; uint32_t q0, nq; bool edge, marks; size_t m[3]; };   // q0, nq: the hypotheses of an ICP span (drain's points_of)
    std::vector<hipEvent_t> pool;    // reused from batch to batch
    size_t used = 0;
    std::vector<Span> spans;
    size_t take();                                               // an event of the pool, or kNoEvent
    size_t begin(hipStream_t st);                                // ... recorded on st, or kNoEvent (counted)
    void end(size_t e0, int kind, uint32_t q0, uint32_t nq, bool edge, hipStream_t st, const size_t *marks = nullptr);
    bool reserve_marks(size_t idx[3], hipEvent_t ev[3]);         // the three mark events of a kd-tree pass (launch_nn_search records them); false: none (counted)
    template <class PointsOf> void drain(PointsOf &&points_of);  // points_of(i): cloud size of hypothesis i
    void reset() { spans.clear(); used = 0; }
    void destroy() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); pool.clear(); reset(); }
};
// A slot's helper thread (PR_SOLVE_HOST): the reference solves on the host (icp.cu:207), which makes a batch a chain of
// launch -> wait -> solve -> launch that only a host thread can drive; the reference's answer is "many host threads, each refining its own
// hypothesis" (README.md:15).  A caller that pipelines batches through pr_refine_submit / pr_refine_wait from ONE thread gets the same
// overlap from the library: each slot owns a thread with a private context (its own streams, workspaces and caches, as pr_thread_context
// gives a caller's thread) that runs the synchronous host-solve path for the batch while the caller goes on to submit the next one.
struct SlotWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool has_job = false, done = false, quit = false, alive = false, started = false;
    int device = 0;
    // the job: every input by value (the caller's arrays of poses may go away after pr_refine_submit returns)
    RefineJob in;
    std::vector<pr_mat4> poses;
    pr_result *results_host = nullptr;
    uint32_t *sizes_host = nullptr;
    int rc = PR_OK;
    std::string err;
};
struct Slot {
    std::unique_ptr<SlotWorker> worker;
    bool worker_job = false;         // the batch in flight runs on the helper thread
    DevBuf poses_bbox, depth, row_count, row_off, counts, cloud, meta, partial, dstate, dresults, arrive, aabb_keys, nn_prev;
    PackedCache packed;
    PinBuf h_in, h_out;
    RefineJob again;                 // the batch in flight, as refine_wait runs it again when the model box it assumed turns out stale
    hipStream_t stream = nullptr, side[3] = { nullptr, nullptr, nullptr };
    hipEvent_t fork = nullptr, join[3] = { nullptr, nullptr, nullptr }, done = nullptr, scene_ready = nullptr, progress = nullptr;
    bool progress_valid = false;
    bool pending = false, delivered = false;
    int nn_set = -1;                 // the set of derived kd-tree records the batch in flight reads (Ctx::nn_sets), -1: none
    uint32_t P = 0;
    pr_result *user_results_host = nullptr;
    uint32_t *user_sizes = nullptr;
    // a TIMED asynchronous batch (option profile = 3): HIP events on the slot's stream around its render, its cloud emit and every
    // correspondence pass, drained by pr_refine_wait
    bool timed = false;
    Spans spans;
};

// ---- hipGraph cache for the device-solve iteration loop ------------------------------------------
struct GraphKey {                    // every value a captured launch depends on, byte for byte (grows as needed)
    std::vector<unsigned char> bytes;
    template <class T> void add(const T &v) { const unsigned char *p = reinterpret_cast<const unsigned char *>(&v); bytes.insert(bytes.end(), p, p + sizeof(T)); }
    bool operator==(const GraphKey &o) const { return bytes == o.bytes; }
};
struct CachedGraph {
    GraphKey key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    uint64_t stamp = 0;
    bool nn_pass = false; uint32_t nn_lds_nodes = 0, nn_stack_depth = 0;     // an in-pass kd-tree launch was captured: what it ran with (a replay reports it again)
};
inline void destroy_graph(CachedGraph &c)
{
    if (c.exec) (void)hipGraphExecDestroy(c.exec);
    if (c.graph) (void)hipGraphDestroy(c.graph);
    c = CachedGraph();
}

constexpr int kNNSets = 2;
struct NNDerived {
    DevBuf topo, bmin, bmax, pts, nnrec, nnrec32, nndesc, nnwide, nnwq, nndepth, nn_cells, nn_grid;
    const void *pcd = nullptr, *normal = nullptr, *nodes = nullptr; uint32_t n_points = 0, n_nodes = 0; uint64_t gen = 0; bool valid = false;
    prk::NNInfo info{};                                          // the host's copy of the control words in nndepth
    float frame_margin = 0.0f;                                   // the acceptance radius (x 1.01) the wide records' frame was built for: a larger radius rebuilds
    bool grid_valid = false, grid_usable = false; uint32_t gw = 0, gh = 0; float gk[4] = { 0, 0, 0, 0 };
    uint64_t used = 0;                                           // Ctx::nn_clock of the latest call that chose this set
    void release() { for (DevBuf *b : { &topo, &bmin, &bmax, &pts, &nnrec, &nnrec32, &nndesc, &nnwide, &nnwq, &nndepth, &nn_cells, &nn_grid }) b->release(); valid = false; grid_valid = false; }
};
struct Ctx {
    std::mutex mu;                   // one call at a time per context; contexts of different devices / threads run side by side
    std::atomic<int> pins{ 0 };      // pr_free holds a private context alive through this while it drains it WITHOUT g_private_mu (private_unregister_and_wait)
    bool ready = false;
    bool is_private = false;         // pr_thread_context(1): owned by one host thread
    int device = -1;
    hipStream_t stream = nullptr;
    hipStream_t side[3] = { nullptr, nullptr, nullptr };   // extra lanes of the device-solve loop (pose groups overlap one group's solve tail with another group's pass)
    hipEvent_t ev_fork = nullptr, ev_join[3] = { nullptr, nullptr, nullptr };
    int n_cus = 256;
    // host copy of the model box the asynchronous path derives its pixel boxes from: keyed by (pointer, size) and VERIFIED on
    // the device by every batch that uses it (refine_submit / refine_wait), so a rewritten triangle buffer cannot go unnoticed
    float aabb_host[6] = { 0, 0, 0, 0, 0, 0 }; bool aabb_host_valid = false;
    const void *mesh_key = nullptr; size_t mesh_n = 0;   // triangle buffer aabb_host belongs to
    // ... and the same buffer's triangles in spatial order (prh::mesh_order), with the multiset fingerprint of the content they were copied from
    // (BatchCheck::mesh_hash): same key, same life cycle, verified by the same batches
    DevBuf mesh_sorted; bool mesh_sorted_valid = false; unsigned long long mesh_hash = 0;
    // ... and its distinct vertices as {x, y, z, 0} (prh::mesh_vertices; option tight_box), made from the same host copy in the same place: valid when
    // mesh_sorted_valid is, and so under the same per-batch fingerprint of the caller's buffer -- a stale list would clip pixels
    DevBuf mesh_verts; uint32_t mesh_verts_n = 0;
    void drop_mesh() { mesh_key = nullptr; aabb_host_valid = false; mesh_sorted_valid = false; mesh_verts_n = 0; }
    uint32_t cloud_hint = 0;          // largest cloud of the latest finished asynchronous batch: sizes the next batch's grid
    // workspaces
    DevBuf aabb, aabb_keys, bbox, poses, depth, row_count, row_off, counts, cloud, meta, partial, sums, nn_prev, dstate, dresults, arrive, conv16, conv8, kd_scratch, kd_tmp, nn_full;
    DevBuf scores;                   // pr_score_poses: the records of a chunk
    DevBuf ov_bits, ov_box, ov_mat;  // pr_score_overlap: the support bit planes and pixel boxes of ALL hypotheses of a call (they outlive its depth chunks), the P x P matrix
    PinBuf h_ov;                     // the matrix on its way to the caller
    DevBuf cov_state, cov_claimed;   // pr_score_cover (the planes and boxes are ov_bits and ov_box): control words, records, order tables and selected list (prk::CoverState); the claimed plane
    PinBuf h_cov;                    // the order tables on their way in, then the whole state on its way to the caller
    DevBuf contours;                 // pr_score_contours: the contour records of a chunk
    DevBuf normals;                  // pr_score_normals: the normal records of a chunk
    PinBuf h_normals;                // ... on their way to the caller
    DevBuf edge_bits, edge_rows;     // pr_scene_edge_distance_dev: the scene's edge bit plane and its row distances (scratch of one call)
    PinBuf h_contours;
    DevBuf cmp_keys, cmp_box, cmp_rec;   // pr_compose_detections: the key frame (8 bytes per frame pixel), the pixel boxes of ALL hypotheses of a call followed by their caller's indices, the records
    PinBuf h_cmp;                    // the records on their way to the caller, then the index table on its way to the device
    DevBuf pd_mats, pd_part, pd_rec; // pr_pose_distance: rows 0..2 of every A S_k (double) followed by those of every B (float); the partials of a launch; its records
    PinBuf h_pd_mats, h_pd_rec;      // the matrices on their way in, the records on their way out
    DevBuf ppf_tmp, ppf_out;         // pr_ppf_*: bucket counts / cursors of a model build or the row counts and offsets of a scene sample; the peaks and references of a vote (pr_ppf_vote_multi: behind the table's model records)
    PinBuf h_ppf;                    // ... and a build's or sample's total, a vote's peaks and references, on their way to the caller (pr_ppf_vote_multi: behind the model records on their way to the device)
    DevBuf plane_tmp;                // pr_scene_planes_dev: the rounds' records, the row counts and offsets of the sample, the samples, the support table (unless the caller's)
    PinBuf h_plane;                  // ... the sample's size, then the rounds' records on their way to the caller
    DevBuf seg_tmp;                  // pr_scene_segments_dev: control words, records, the rank table, the qualifying roots, chunk counts and offsets, the forest and the per-root counts; pr_segment_depth_dev: the keep bits
    PinBuf h_seg;                    // ... the control words and roots on their way to the host, the rank table on its way to the device, the records on their way to the caller
    DevBuf cloud_tmp;                // pr_cloud_normals_dev / pr_scene_nn_from_cloud_dev: the tally of the points per status
    DevBuf dfilt_tmp;                // pr_depth_filter_dev: the control words (the pixels per flag code)
    PinBuf h_dfilt;                  // ... on their way to the caller
    DevBuf reproj_tmp;               // pr_depth_reproject_dev: the key plane of the target and, behind it, the control words
    PinBuf h_reproj;                 // ... which the last resolve tile leaves here
    DevBuf vsd_rec;                  // pr_pose_vsd: the records of a chunk's pairs
    PinBuf h_vsd;                    // ... on their way to the caller
    DevBuf solid_far, solid_rec;     // pr_render_span / pr_pose_penetration: the far plane of the boxes in g->depth (same offsets); the P x P pair records
    PinBuf h_solid;                  // the records on their way to the caller
    DevBuf info_meta, info_part;     // pr_icp_information / pr_pose_information: the hypotheses' records (cloud, centre, radius) and the workgroups' partial sums
    PinBuf h_info_meta, h_info_out;  // the records on their way in; pr_pose_info and pr_pose_eig on their way to the caller (stored by the eigen kernel)
    DevBuf lvl_rows, lvl_counts, lvl_carry;   // pr_refine_pyramid: per-row sample counts and offsets of every level of a chunk, the level clouds' sizes, the per-level carry records
    PinBuf h_lvl_carry;
    DevBuf multi;                    // mixed batches (pr_*_multi): mesh table, box index / image of each hypothesis, raster groups
    PinBuf h_sums, h_meta, h_counts, h_results, h_dstate, h_poses, h_flags, h_scores, h_multi;
    PackedCache packed;              // synchronous paths (the asynchronous slots keep their own)
    // kd-tree scenes: what the library derives from a scene (traversal records, wide records, pixel grid) -- kNNSets sets, so that with a NEW scene per
    // frame the batch of one asynchronous slot keeps the set it runs on while the next frame's records are derived into the other (round 5: one set
    // meant draining both slots before every new scene)
    NNDerived nn_sets[kNNSets];
    uint64_t nn_clock = 0;
    DevBuf nn_counters;
    // profiling
    Spans spans;                     // of the context's own stream (SpanGuard)
    double icp_ms = 0, render_ms = 0, cloud_ms = 0; uint64_t icp_launches = 0, icp_points = 0, icp_bytes = 0, sample_clock = 0;
    std::vector<float> icp_launch_us;                            // the timed launches one by one (pr_profile_launches), bounded
    uint64_t stat_repeated = 0, stat_timing_dropped = 0;         // pr_stats: batches run twice by the stale-cache safety net; timed spans lost to a failed event call
    double nn_part_ms[4] = { 0, 0, 0, 0 }; uint64_t nn_part_n = 0;   // kd-tree pass by kernel: search, bound, task walk, winners pass (pr_profile_nn)
    Slot slots[kSlots];
    std::vector<CachedGraph> graphs;
    uint64_t graph_clock = 0;
    // RCCL communicator this context is a rank of (pr_comm_init_rank / pr_comm_init_all), or null
    ncclComm_t comm = nullptr; int comm_rank = 0, comm_world = 1;
    DevBuf gather_tmp;
    // HIP events around the gathers issued while option "profile" is on (pr_gather_profile)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> gather_ev; size_t gather_ev_used = 0; double gather_ms = 0; uint64_t gather_n = 0;
};

// ---- context registry --------------------------------------------------------------------------------
// One shared context per device (created by pr_init / pr_set_device / first use) plus optional private contexts of single
// host threads (pr_thread_context).  `g` is the context the calling thread is bound to; every entry point binds a thread
// that never chose one to the process default (the device of the first pr_init, else device 0).
extern std::mutex g_reg_mu;
extern std::vector<Ctx *> g_shared;         // index = device ordinal
extern int g_default_device;
extern thread_local Ctx *g;
struct PrivateCtx { Ctx *c = nullptr; ~PrivateCtx(); };   // destructor below, once the teardown helpers exist
extern thread_local PrivateCtx tl_private;
// every private context alive, so that pr_free can drain the device's contexts one by one.  g_private_mu guards the LIST only and is never
// held while a context's mu is taken or waited for (a slot's helper thread registers / unregisters its private context while its
// caller holds the caller's context mutex and waits for it; pr_free on a third thread used to hold g_private_mu while it locked every context
// of the device -- a three-way wait).  pr_free pins the contexts it found (under g_private_mu), drops g_private_mu, then locks them one by
// one; a context that is being released is unregistered first (no new pins), torn down, and deleted once its pins are gone.
extern std::mutex g_private_mu;
extern std::vector<Ctx *> g_private;
inline void private_register(Ctx *c) { std::lock_guard<std::mutex> lk(g_private_mu); g_private.push_back(c); }
inline void private_unregister(Ctx *c) { std::lock_guard<std::mutex> lk(g_private_mu); for (size_t i = 0; i < g_private.size(); ++i) if (g_private[i] == c) { g_private.erase(g_private.begin() + (long)i); break; } }
inline void private_wait_unpinned(Ctx *c) { while (c->pins.load(std::memory_order_acquire) != 0) std::this_thread::yield(); }   // call with NO lock held, after private_unregister

inline void drop_graphs() { for (auto &c : g->graphs) destroy_graph(c); g->graphs.clear(); }
void comm_teardown(Ctx *c);

inline int device_count_checked(int *n_out)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no usable HIP device (hipGetDeviceCount: %s, count %d) -- this library has no CPU fallback",
                  hipGetErrorString(e), n);
        return PR_ERR_NO_DEVICE;
    }
    *n_out = n;
    return PR_OK;
}

// bind the calling thread to the shared context of `device` (-1: the process default), creating it if needed
inline int bind_shared(int device)
{
    std::lock_guard<std::mutex> lk(g_reg_mu);
    if (device < 0) device = g_default_device >= 0 ? g_default_device : 0;
    int n = 0;
    PR_TRY(device_count_checked(&n));
    if (device >= n) { set_error("device %d out of range (%d visible)", device, n); return PR_ERR_NO_DEVICE; }
    if ((int)g_shared.size() < n) g_shared.resize((size_t)n, nullptr);
    if (!g_shared[(size_t)device]) { g_shared[(size_t)device] = new Ctx(); g_shared[(size_t)device]->device = device; }
    if (g_default_device < 0) g_default_device = device;
    g = g_shared[(size_t)device];
    return PR_OK;
}
inline int bind_default() { return g ? PR_OK : bind_shared(-1); }

// with g->mu held: make the context's device current for this thread and create its stream on first use
inline int require_ctx()
{
    HIP_TRY(hipSetDevice(g->device));                            // the current device is per host thread
    if (g->ready) return PR_OK;
    HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&g->ev_fork, hipEventDisableTiming));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, g->device) == hipSuccess && prop.multiProcessorCount > 0) g->n_cus = prop.multiProcessorCount;
    g->ready = true;
    return PR_OK;
}
// every device entry point: bind, lock, make current
#define PR_ENTER()                                   \
    PR_TRY(bind_default());                          \
    std::lock_guard<std::mutex> lk(g->mu);           \
    PR_TRY(require_ctx())

// ---- profiling spans: the recorder's bodies (they count into the calling thread's context) and the guard of the context's own stream ---------
inline size_t Spans::take()
{
    hipEvent_t e = nullptr;
    if (used == pool.size()) { if (hipEventCreate(&e) != hipSuccess || !e) { (void)hipGetLastError(); return kNoEvent; } pool.push_back(e); }
    return used++;
}
inline size_t Spans::begin(hipStream_t st)
{
    const size_t e = take();
    if (e != kNoEvent && hipEventRecord(pool[e], st) == hipSuccess) return e;
    (void)hipGetLastError(); g->stat_timing_dropped++; return kNoEvent;
}
inline void Spans::end(size_t e0, int kind, uint32_t q0, uint32_t nq, bool edge, hipStream_t st, const size_t *marks)
{
    const size_t e1 = e0 == kNoEvent ? kNoEvent : begin(st);     // (a span without its start was dropped and counted by begin)
    if (e1 == kNoEvent) return;
    spans.push_back({ e0, e1, kind, q0, nq, edge, marks != nullptr, { marks ? marks[0] : 0, marks ? marks[1] : 0, marks ? marks[2] : 0 } });
}
inline bool Spans::reserve_marks(size_t idx[3], hipEvent_t ev[3])
{
    for (int k = 0; k < 3; ++k) { if ((idx[k] = take()) == kNoEvent) { g->stat_timing_dropped++; return false; } ev[k] = pool[idx[k]]; }
    return true;
}
constexpr size_t kLaunchSamples = 8192;
template <class PointsOf> inline void Spans::drain(PointsOf &&points_of)      // call after the stream has been synchronised
{
    for (const Span &s : spans) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, pool[s.e0], pool[s.e1]) != hipSuccess) continue;
        if (s.kind == kSpanRender) { g->render_ms += ms; continue; }
        if (s.kind == kSpanCloud) { g->cloud_ms += ms; continue; }
        uint64_t pts = 0;
        for (uint32_t i = s.q0; i < s.q0 + s.nq; ++i) pts += points_of(i);
        g->icp_ms += ms; g->icp_launches++; g->icp_points += pts; g->icp_bytes += icp_span_bytes(pts, s.edge);
        if (g->icp_launch_us.size() < kLaunchSamples) g->icp_launch_us.push_back(ms * 1e3f);
        if (!s.marks) continue;                                 // kd-tree pass: search | bound | task walk | winners pass
        const hipEvent_t ev[5] = { pool[s.e0], pool[s.m[0]], pool[s.m[1]], pool[s.m[2]], pool[s.e1] };
        float part[4]; bool ok = true;
        for (int k = 0; k < 4; ++k) ok = ok && hipEventElapsedTime(&part[k], ev[k], ev[k + 1]) == hipSuccess;
        if (ok) { for (int k = 0; k < 4; ++k) g->nn_part_ms[k] += part[k]; g->nn_part_n++; }
    }
    reset();
}
// a span of the context's own stream, for the guard's lifetime (option profile).  The synchronous drivers know their cloud sizes when they enqueue:
// they add the points and bytes of an ICP span themselves (icp_span_bytes), and the span carries no hypotheses.
struct SpanGuard {
    bool on; size_t e0 = kNoEvent; int kind;
    explicit SpanGuard(int k) : on(opt.profile != 0), kind(k) { if (on) e0 = g->spans.begin(g->stream); }
    ~SpanGuard() { if (on) g->spans.end(e0, kind, 0, 0, false, g->stream); }
};
inline void drain_spans() { g->spans.drain([](uint32_t) { return 0u; }); }      // call after the stream has been synchronised

// A few words from device memory to the host WITHOUT a copy command: a kernel stores them into the context's pinned flag array, the stream is
// waited for, the host copies them out.  Round 6: copy commands to pageable host memory go through the runtime's bounce buffers and its copy-engine
// path -- tens of microseconds each, and the place where one-off multi-millisecond stalls came from (profiles/r06/README.md).  n_words <= 64.
inline int read_back_words(const void *dev_src, void *host_dst, uint32_t n_words, hipStream_t st)
{
    if (n_words == 0 || n_words > 64) { set_error("read_back_words: 1..64 words"); return PR_ERR_INVALID; }
    PR_TRY(g->h_flags.ensure(256));
    HIP_TRY(prk::launch_copy_words32(dev_src, g->h_flags.dev, n_words, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(host_dst, g->h_flags.p, sizeof(uint32_t) * n_words);
    return PR_OK;
}

inline void identity16(float *T) { for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.0f : 0.0f; }

// ---- scene variants -----------------------------------------------------------------------------
struct SceneSel {
    int kind = PR_SCENE_PROJ;
    bool packed = false;
    prk::SceneProjAoS aos{};
    prk::SceneProjPacked pk{};
    prk::SceneNNDev nn{};
    prk::SceneGridDev grid{};        // closest-point grid (kind PR_SCENE_GRID): the caller's arrays as they are, nothing derived, nothing cached
    uint32_t nn_split = 0;           // kd-tree scene: search kernel + winners pass instead of the fused search pass
    uint32_t nn_max_points = 0;      // largest cloud of the batch (grid of the search kernel)
    int nn_set = -1;                 // kd-tree scene: which of Ctx::nn_sets the records are in
};
// the route of a kd-tree batch: search kernels + winners pass (compact records and option nn_split), else the fused search pass
inline uint32_t nn_split_for(const SceneSel &sc) { return (sc.kind == PR_SCENE_NN && sc.nn.rec32 && opt.nn_split) ? 1u : 0u; }
constexpr uint32_t kCounterPasses = 64;
// camera of the hypotheses (fused paths): lets a kd-tree scene be indexed by pixel as well
struct Camera { uint32_t w = 0, h = 0; float fx = 0, fy = 0, cx = 0, cy = 0; };

// ---- functions of the other translation units (pr_scene / pr_icp / pr_refine / pr_comm / pr_context) ---------------------------------
int make_scene(int kind, const void *scene, bool want_packed, SceneSel &out, PackedCache *pc_in = nullptr, hipStream_t st = nullptr, const Camera *cam = nullptr,
               bool verify_now = true);
int kd_build_dev(pr_vec3 *pcd, pr_vec3 *nrm, uint32_t n, int max_leaf, pr_kdnode *nodes, size_t cap, uint32_t *n_nodes);
hipError_t launch_pass(const prk::IcpBatch &b, const SceneSel &sc, uint32_t P, hipStream_t st = nullptr, hipEvent_t *nn_marks = nullptr);
int ensure_stream(hipStream_t &st, hipEvent_t *ev = nullptr);

// ---- pose groups: a batch split over up to four streams ------------------------------------------------------------
// The lanes of one loop: the context's own (icp_drive) or a slot's (refine_submit_async).  Side streams and their join events are created
// on first use (ensure_stream has the reason), so the arrays are the owner's.
struct Lanes { hipStream_t main; hipStream_t *side; hipEvent_t fork; hipEvent_t *join; };
inline hipStream_t lane(const Lanes &l, uint32_t grp) { return grp ? l.side[grp - 1] : l.main; }
// groups of a batch of n hypotheses.  Launches of different groups overlap: a timed batch is one group, so that the measured kernel has the chip to itself
inline uint32_t pose_group_count(int scene_kind, uint32_t n, bool timed) { return timed ? 1u : std::max(1u, std::min({ pose_groups_for(scene_kind), 4u, n / 32u })); }
inline uint32_t group_begin(uint32_t n, uint32_t n_groups, uint32_t grp) { return (uint32_t)(((uint64_t)n * grp) / n_groups); }
// the side lanes start behind everything the main lane holds so far ...
inline int lanes_fork(const Lanes &l, uint32_t n_groups)
{
    if (n_groups <= 1) return PR_OK;
    for (uint32_t k = 1; k < n_groups; ++k) PR_TRY(ensure_stream(l.side[k - 1], &l.join[k - 1]));
    HIP_TRY(hipEventRecord(l.fork, l.main));
    for (uint32_t k = 1; k < n_groups; ++k) HIP_TRY(hipStreamWaitEvent(l.side[k - 1], l.fork, 0));
    return PR_OK;
}
// ... and the main lane goes on behind all of them
inline int lanes_join(const Lanes &l, uint32_t n_groups)
{
    for (uint32_t k = 1; k < n_groups; ++k) { HIP_TRY(hipEventRecord(l.join[k - 1], l.side[k - 1])); HIP_TRY(hipStreamWaitEvent(l.main, l.join[k - 1], 0)); }
    return PR_OK;
}
// the part of a batch that belongs to the group starting at hypothesis p0 (the clouds themselves are addressed through PoseMeta::start)
inline prk::IcpBatch group_slice(const prk::IcpBatch &b, uint32_t p0)
{
    prk::IcpBatch bb = b;
    bb.meta += p0; bb.partial += (size_t)p0 * b.nblk * prk::kAccStride; if (bb.nn_qcount) bb.nn_qcount += prk::kQCountStride * (size_t)p0;
    return bb;
}
// The device-solve iteration loop of n hypotheses (meta, dstate, arrive, b.partial and b's kd-tree queue counters at hypothesis 0): fork, (max_iteration + 1) x
// [pass (+ finalize / solve launch unless the pass' tail does it: fused)] per group, join.  Both the synchronous driver and the asynchronous slots
// run THIS loop -- the slots' safety net re-runs a batch through the synchronous one and expects the same bytes.  It makes no synchronising call
// of its own (drive_device records it into a hipGraph); what differs between the callers comes in as
//   pass(bb, p0, np, stream) -> rc: launch_pass for one group, with whatever timing the caller keeps around it;
//   after(it, stop) -> rc:          behind the launches of iteration `it` (an early-exit read-back, a progress event); stop = true ends the loop.
template <class Pass, class After>
int device_solve_loop(const Lanes &lanes, uint32_t n_groups, prk::IcpBatch b, uint32_t n, pr_criteria crit, bool fused, prk::PoseMeta *meta,
                      prk::DevIcpState *dstate, uint32_t *arrive, Pass &&pass, After &&after)
{
    b.meta = meta;
    PR_TRY(lanes_fork(lanes, n_groups));
    bool stop = false;
    for (uint32_t it = 0; it <= (uint32_t)crit.max_iteration && !stop; ++it) {
        for (uint32_t grp = 0; grp < n_groups; ++grp) {
            const uint32_t p0 = group_begin(n, n_groups, grp), np = group_begin(n, n_groups, grp + 1) - p0;
            prk::IcpBatch bb = group_slice(b, p0);
            bb.iter = it;
            if (fused) { bb.fused = 1; bb.crit = crit; bb.st = dstate + p0; bb.arrive = arrive + p0; }
            bb.score_only = (it == (uint32_t)crit.max_iteration) ? 1u : 0u;
            PR_TRY(pass(bb, p0, np, lane(lanes, grp)));
            if (!fused) HIP_TRY(prk::launch_icp_finalize_solve(bb.partial, meta + p0, b.nblk, b.steps, dstate + p0, crit, it, np, lane(lanes, grp)));
        }
        PR_TRY(after(it, stop));
    }
    return lanes_join(lanes, n_groups);
}
int icp_drive(pr_vec3 *cloud_base, const uint32_t *start_h, const uint32_t *count_h, uint32_t P, const SceneSel &sc_in,
              pr_criteria crit, pr_result *results_host, pr_result *results_dev, const pr_robust &robust = pr_robust{ PR_ROBUST_NONE, 0.0f, 0.0f, 0 });
// The information pass and the eigen kernel (pose_info.hip) on P clouds laid out as icp_drive takes them; centers: 3 floats per cloud, radii: one;
// info_host[P], eig_host[P] or null (pr_pose_info.cpp).  Returns with the stream drained.  The clouds are only read.
int info_drive(const pr_vec3 *cloud_base, const uint32_t *start_h, const uint32_t *count_h, uint32_t P, const SceneSel &sc, const pr_robust &robust,
               const float *centers, const float *radii, pr_pose_info *info_host, pr_pose_eig *eig_host);
// the information calls' own argument checks, before any device is touched, and the covariance of one record pair.  No HIP call in here:
// tools/job_sanitize.cpp runs them under ASan / UBSan.
inline int info_scene_ok(const char *fn, int scene_kind, const void *scene)
{
    if (scene_kind != PR_SCENE_NN && scene_kind != PR_SCENE_PROJ && scene_kind != PR_SCENE_PROJ_CROP && scene_kind != PR_SCENE_GRID) { set_error("%s: unknown scene kind %d", fn, scene_kind); return PR_ERR_INVALID; }
    if (!scene) { set_error("%s: bad arguments (scene is null)", fn); return PR_ERR_INVALID; }
    if (scene_kind == PR_SCENE_GRID) PR_TRY(grid_desc_ok(fn, static_cast<const pr_scene_grid *>(scene), /*built=*/true));
    return PR_OK;
}
// c_i = pose_i applied to its mesh's centre, in float64, millimetres to metres as the cloud extraction converts them, rounded to float32; rad_i = its
// mesh's radius.  mesh_of: every pose's index into centers_model / radii (null: one mesh).  pr_pose_information and pr_contour_information both
// call THIS: combine_information adds their matrices, so their centres must be the same bits.
inline void camera_centers(const pr_mat4 *poses, const uint32_t *mesh_of, uint32_t P, const float *centers_model, const float *radii, float *centers, float *rad)
{
    for (uint32_t j = 0; j < P; ++j) {
        const uint32_t m = mesh_of ? mesh_of[j] : 0u;
        const float *M = poses[j].m, *cm = centers_model + 3 * (size_t)m;
        for (int a = 0; a < 3; ++a) {
            const double v = (((double)M[4 * a] * (double)cm[0] + (double)M[4 * a + 1] * (double)cm[1]) + (double)M[4 * a + 2] * (double)cm[2]) + (double)M[4 * a + 3];
            centers[3 * (size_t)j + a] = (float)(v / 1000.0);
        }
        rad[j] = radii[m];
    }
}
inline int info_center_radius_ok(const char *fn, const float *centers, const float *radii, uint32_t n)
{
    if (n && (!centers || !radii)) { set_error("%s: bad arguments (centres or radii null)", fn); return PR_ERR_INVALID; }
    for (uint32_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) if (!std::isfinite(centers[3 * (size_t)i + a])) { set_error("%s: centre %u is not finite", fn, i); return PR_ERR_INVALID; }
        if (!std::isfinite(radii[i]) || !(radii[i] > 0.0f)) { set_error("%s: radius %u must be finite and positive (got %g)", fn, i, (double)radii[i]); return PR_ERR_INVALID; }
    }
    return PR_OK;
}
// pr_info_covariance, host only.  The eigenpairs counted: lambda[k] > 0 and lambda[k] > min_ratio * lambda[5]; cov = sigma2 * sum v_k v_k^T / lambda[k], k ascending.
inline int info_covariance(const pr_pose_info *info, const pr_pose_eig *eig, double sigma, double min_ratio, double *cov21_out, uint32_t *rank_out,
                           double *sigma2_out)
{
    const char *fn = "pr_info_covariance";
    if (!info || !eig) { set_error("%s: bad arguments (info or eig is null)", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(min_ratio) || min_ratio < 0.0) { set_error("%s: min_ratio must be finite and >= 0", fn); return PR_ERR_INVALID; }
    if (!std::isfinite(sigma)) { set_error("%s: sigma must be finite", fn); return PR_ERR_INVALID; }
    double sigma2;
    if (sigma > 0.0) sigma2 = sigma * sigma;
    else {
        if (info->n_valid <= 6 || info->sum_w == 0.0) { set_error("%s: no residual variance with n_valid = %u, sum_w = %g (give sigma > 0)", fn, info->n_valid, info->sum_w); return PR_ERR_INVALID; }
        sigma2 = (info->sum_wr2 / info->sum_w) * (double)info->n_valid / (double)(info->n_valid - 6u);
    }
    uint32_t rank = 0;
    double cov[21] = { 0.0 };
    for (int k = 0; k < 6; ++k) {
        const double l = eig->lambda[k];
        if (!(l > 0.0) || !(l > min_ratio * eig->lambda[5])) continue;
        ++rank;
        int idx = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) cov[idx++] += eig->V[6 * i + k] * eig->V[6 * j + k] / l;
    }
    if (cov21_out) for (int i = 0; i < 21; ++i) cov21_out[i] = sigma2 * cov[i];
    if (rank_out) *rank_out = rank;
    if (sigma2_out) *sigma2_out = sigma2;
    return PR_OK;
}
// ---- audit recorder of the host-solve loop's sums (pr_debug_trace_sums, pr_icp.cpp) ---------------------------------
// Per host thread, hence for the context that thread is bound to: `armed` waits for the thread's next synchronous ICP call, whose
// entry point opens a TraceScope -- the recorder becomes `active` for exactly that call and is gone when it returns, error or
// not.  icp_drive reads `active` only; a traced fused batch stays on the caller's thread (refine_submit).
struct SumsTrace { float *rows = nullptr; uint32_t n_hyp = 0, n_passes = 0; };
struct SumsTraceState { SumsTrace armed, active; };
extern thread_local SumsTraceState tl_sums_trace;
struct TraceScope {
    TraceScope() { tl_sums_trace.active = tl_sums_trace.armed; tl_sums_trace.armed = SumsTrace(); }
    ~TraceScope() { tl_sums_trace.active = SumsTrace(); }
    TraceScope(const TraceScope &) = delete;
    TraceScope &operator=(const TraceScope &) = delete;
};
// with a recorder active: does it fit a batch of P hypotheses under crit?  (PR_ERR_INVALID with a message if not; PR_OK without a recorder)
int sums_trace_admits(const char *fn, uint32_t P, const pr_criteria &crit);
void drain_all_slots();
// a write through the library into caller-owned device memory: logged for the caches (WriteLog) and ordered BEHIND every batch of this context that is still
// in flight and reads the range as part of its scene, mesh or result block (a scene object re-initialised per frame keeps its arrays, so the
// next frame's preparation would otherwise overwrite them under the previous frame's batch).  Call with g->mu held.
void drain_slots_reading(const void *p, size_t bytes);
inline void note_write(const void *p, size_t bytes) { g_writes.note(p, bytes); drain_slots_reading(p, bytes); }
void slot_release(Slot &sl);
void slot_drain(Slot &sl);
void comm_teardown(Ctx *c);
void ctx_teardown(Ctx *c);
int rccl_load();

}  // namespace prr
