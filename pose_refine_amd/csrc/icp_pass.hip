// icp_pass.hip -- THE hot kernel: thrust::transform_reduce(thrust__pcd2Ab<Scene>) (icp.cu:170-172) fused with transform_pcd_cuda of the previous iteration (icp.cu:142-153), and the second reduction stage / device solve (icp.cu:178-212)
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
#include "pr_launch.h"
#include "icp_accumulate.h"
#include "icp_solve_device.h"

namespace prk {

// ================================================================================================
//  THE hot kernel: pending transform + correspondence + 29-term transform-reduce, all hypotheses
//  of a batch in one launch.  grid = (workgroups per hypothesis, hypotheses), 256 lanes.
// ================================================================================================
template <class Scene, bool kNN, int kStack = 0, bool kRobust = false>
__global__ __launch_bounds__(256, PR_PASS_WAVES) void icp_pass_kernel(IcpBatch b, Scene scene)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ float wsum[4][kAccStride];

    const uint32_t pose = blockIdx.y;
    const PoseMeta &pm = b.meta[pose];                           // uniform address: one 64-byte scalar load
    const int32_t st = pm.state;
    if (st == kSkip) return;
    const uint32_t n = pm.count;
    const uint32_t ppb = b.steps * kPointsPerStep;
    if ((uint64_t)blockIdx.x * ppb >= n) return;

    const int4 *lds_topo = nullptr;
    int *stk_node = nullptr; float *stk_lb = nullptr;
    if constexpr (kNN && kStack == 0) {
        int4 *dst = reinterpret_cast<int4 *>(lds_raw);
        for (uint32_t i = threadIdx.x; i < scene.lds_nodes; i += kBlockThreads) dst[i] = scene.topo[i];
        __syncthreads();
        lds_topo = dst;
    }
    if constexpr (kNN && kStack > 0) {                           // per-lane stacks: [entry][lane], then the staged records
        stk_node = reinterpret_cast<int *>(lds_raw) + threadIdx.x;
        stk_lb = reinterpret_cast<float *>(lds_raw) + (size_t)(kStack & 0xff) * kBlockThreads + threadIdx.x;
        float4 *recs = reinterpret_cast<float4 *>(lds_raw + (size_t)(kStack & 0xff) * kBlockThreads * 8);
        if constexpr ((kStack & 0x100) == 0) for (uint32_t i = threadIdx.x; i < scene.lds_nodes * 4; i += kBlockThreads) recs[i] = scene.rec[i];
        __syncthreads();
        lds_topo = reinterpret_cast<const int4 *>(recs);
    }
    if constexpr (kNN && kStack == -1) scene.winner += pm.start;  // winners are indexed like the cloud

    float *cl = reinterpret_cast<float *>(b.cloud + pm.start);
    // a pending update that nn_search_kernel has already applied to the cloud must not be applied again
    const bool xf = (st == kRunWithTransform) && !b.pre_transformed;   // also: not the first pass of this cloud (a seed exists)
    uint32_t *nn_prev = (kNN && kStack >= 0 && b.nn_prev) ? b.nn_prev + pm.start : nullptr;
    float M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = xf ? pm.xform[i] : 0.0f;

    // One virtual workgroup of the canonical tree per trip.  The grid normally holds one workgroup per 2048-point block; the
    // asynchronous fused path sizes its grid from the previous batch's cloud sizes (the current ones are still on the device),
    // so a workgroup may have to take more than one block -- partial sums are per virtual block either way.
    const uint32_t used = (n + ppb - 1) / ppb;
    for (uint32_t vb = blockIdx.x; vb < used; vb += gridDim.x) {
        if (vb != blockIdx.x) __syncthreads();                   // wsum of the previous trip has been read
        float acc[29];
#pragma unroll
        for (int i = 0; i < 29; ++i) acc[i] = 0.0f;
        float t;
        if (b.score_only) {                                      // uniform: the final pass needs sums 27 and 28 only
            vb_accumulate<Scene, kNN, kStack, true>(acc, cl, n, vb * ppb, b.steps, xf, M, scene, lds_topo, stk_node, stk_lb, nn_prev, xf);
            t = vb_reduce<true>(acc, wsum);
        } else {
            if constexpr (kRobust)                               // the weight of b (uniform); the score-only pass above needs none
                vb_accumulate<Scene, kNN, kStack, false, true>(acc, cl, n, vb * ppb, b.steps, xf, M, scene, lds_topo, stk_node, stk_lb, nn_prev, xf, RobustW{ b.robust_kind, b.robust_c, b.robust_inv_c });
            else
                vb_accumulate<Scene, kNN, kStack>(acc, cl, n, vb * ppb, b.steps, xf, M, scene, lds_topo, stk_node, stk_lb, nn_prev, xf);
            t = vb_reduce(acc, wsum);
        }
        if (pass_deliver(b, pose, vb, used, n, t)) return;
    }
}

// second stage: workgroup sums added sequentially in workgroup order, starting from 0
__device__ __forceinline__ float sum_partials(const float *partial, uint32_t pose, uint32_t nblk, uint32_t used, uint32_t comp)
{
    // the loads of a chunk are independent and issued together; only the additions are ordered
    float total = 0.0f;
    const float *p = partial + (size_t)pose * nblk * kAccStride + comp;
    for (uint32_t g0 = 0; g0 < used; g0 += 16) {
        float v[16];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) v[k] = (g0 + k < used) ? p[(size_t)(g0 + k) * kAccStride] : 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) if (g0 + k < used) total += v[k];
    }
    return total;
}

// ================================================================================================
//  The whole loop of a hypothesis in ONE workgroup (option "resident_loop", asynchronous fused path, packed projective scene, device solve):
//  grid = hypotheses, all passes in one launch, in one of two workgroup sizes (option "loop_waves"): 1024 lanes = 16 wavefronts, one workgroup
//  per compute unit (icp_loop_cu_kernel), or 512 lanes = 8 wavefronts, two workgroups per compute unit (icp_loop_cu8_kernel).  The library takes
//  the 8-wave form for a sub-batch with at least one hypothesis per compute unit and the 16-wave form for a smaller one, which cannot fill the
//  chip and keeps the lower latency.  Between the two barriers of a pass one wavefront adds the rows and solves while the others of its workgroup
//  wait -- 4.5 us of a pass, measured -- and the wavefronts of a second, independent hypothesis on the same compute unit use that time; so do the
//  idle rounds of a cloud whose items do not divide by the wavefronts.  HIP promises nothing about where a workgroup lands, and nothing here
//  depends on it: no workgroup waits for another one.  What the multi-launch loop pays per pass --
//  a launch, a ragged last round of workgroups, partial sums and an arrival ticket through memory, a PoseMeta round trip -- becomes two
//  LDS barriers.  No workgroup waits for another one: a batch larger than the chip runs in rounds.
//  Unit of work: item 4 * vb + w = wavefront w of virtual block vb of the canonical tree (vb_accumulate_at with tib = 64 w + lane), always
//  taken by wavefront (4 * vb + w) mod kWaves (16 or 8).  The mapping never changes, so a lane only reads cloud points that it wrote itself (or that
//  were there before the launch): the cloud stays in memory, moved and written back per pass exactly as icp_pass_kernel does, no fence.
//  Per pass: every wavefront leaves the 29 sums of its items in LDS row [vb][w] (wave_reduce) | barrier | wavefront 0 forms
//  ((w0+w1)+w2)+w3 per block, adds the blocks in block order from 0.0f (sum_partials' sequence), runs pose_iteration_wave and leaves the
//  update and the finished flag in LDS | barrier | everyone reads them.  Trip count and early exit are read from LDS behind the second
//  barrier, so every wavefront -- also one without items -- meets both barriers of every pass.
//  DevIcpState stays in the LDS header over the loop (only wavefront 0 touches it; registers are left to the point work) and is stored once;
//  PoseMeta is left as the multi-launch loop leaves it (kSkip, the last update).  Same source per point, same tree: the same bytes.
//  LDS (dynamic): b.nblk * 4 rows of kAccStride floats, then kLoopHeader words: [0..11] update, [12] finished, [16..35] DevIcpState, then
//  (kTables, option "loop_lds_tables") the scene's colf and rowf tables, width + height floats, then the LDS image of the cloud's head (option
//  "loop_lds_blocks") -- within 160 KiB for the 16-wave form and 80 KiB for the 8-wave one (icp_loop_cu_layout).
//  The tables in LDS: filled once at the start of the kernel by the whole workgroup, one more barrier ahead of pass 0 (behind the early return,
//  which is the whole workgroup's); from then on two of the three gathers per point and pass (gather_issue(SceneProjPackedLds), proj_query.h)
//  are ds_read_b32 instead of trips through the texture addresser, whose rate is what a pass waits for.  The record gather stays in memory.
//  With and without tables are two instantiations, not a branch per gather.
//  The head of the cloud in LDS: the workgroup has its compute unit to itself (sixteen wavefronts of 124+ VGPRs are the whole register file),
//  so the LDS beyond rows and header is free.  Points [0, b.lds_blocks * ppb) -- whole blocks, items 0 .. 4 * b.lds_blocks - 1 -- are loaded from
//  memory in pass 0 (pending transform applied exactly where the other items apply it), stored to LDS whether moved or not, and from pass 1 on
//  read from LDS, moved and written to LDS: their 12 + 12 bytes per point and pass never reach the fabric, and the first of a step's two
//  dependent trips (point, then scene gather) is an LDS access.  The other items run as before.  The item -> wavefront -> lane mapping is
//  fixed, so a lane reads only LDS words that it stored itself in its own pass 0 or later -- no barrier beyond the two of a pass, and a
//  workgroup that follows another one on the compute unit never sees what that one left.  The one exception is the clamp: a lane past the end
//  of the cloud reads the cloud's LAST point and never uses it.  Blocks are resident whole, so for a lane of a resident block that index, below the
//  lane's own, is inside the image, and its owner stored it ahead of pass 0's first barrier (pass 0 itself reads memory); a later pass may
//  read it while the owner rewrites it -- the value is discarded, as in memory.
//  Layout: 12-byte records, point j at byte 12 j, the cloud's own layout -- the lane's byte offset serves both address spaces.  Banks: the
//  accesses are ds_read2_b32 + ds_read_b32 (and their writes), banked (a / 4) mod 32 per 32-lane half; adjacent lanes hold adjacent points,
//  word 3 t + k for lane t, and 3 is odd, so the 32 lanes of a half fall on 32 different banks: conflict-free, six LDS cycles per point
//  and wavefront, the same as three planes of floats would cost, without three base registers.
//  The cloud in MEMORY is left stale for the resident points (nothing is flushed): a slot's cloud buffer is private scratch that only the emit
//  writes and only the loop of the same sub-batch reads, and the next sub-batch's emit overwrites it (AsyncBatch::sub_batch, pr_refine.cpp).
// ================================================================================================
constexpr uint32_t kLoopLanes = 1024, kLoopWaves = kLoopLanes / 64, kLoopHeader = 64;
// (Measured and not kept: the two barriers with a fence on LDS alone, so that a wavefront does not wait for its cloud stores before it meets the
// others -- 330.2-332.9 k against 329.7-332.5 k poses/s for __syncthreads, five alternating runs on one box.)
static_assert(sizeof(DevIcpState) == 20 * sizeof(uint32_t), "the LDS header holds DevIcpState as 20 words");
size_t icp_loop_cu_lds_bytes(uint32_t nblk) { return ((size_t)nblk * 4 * kAccStride + kLoopHeader) * sizeof(float); }
// blocks of a cloud's head that the kernel keeps in LDS behind rows and header: as many whole blocks of steps * 1024 points as the compute unit's
// LDS holds, at most the plan's nblk and at most `cap` (option "loop_lds_blocks": negative = no cap)
uint32_t icp_loop_cu_lds_blocks(uint32_t nblk, uint32_t steps, int cap)
{
    const size_t fixed = icp_loop_cu_lds_bytes(nblk), block = (size_t)steps * kPointsPerStep * sizeof(pr_vec3);
    if (fixed > kLoopCuLdsBudget || block == 0) return 0;
    const size_t fit = (kLoopCuLdsTotal - fixed) / block;
    uint32_t r = (uint32_t)(fit < nblk ? fit : nblk);
    if (cap >= 0 && (uint32_t)cap < r) r = (uint32_t)cap;
    return r;
}
// words of the two tables in LDS (option "loop_lds_tables"): width + height floats, rounded up to four so that the cloud image behind them keeps
// its 16-byte alignment
__host__ __device__ constexpr uint32_t loop_table_words(uint32_t width, uint32_t height) { return (width + height + 3u) & ~3u; }
// The whole layout for a workgroup of `waves` wavefronts (16: the compute unit's 160 KiB; 8: half of it, so that two workgroups fit): rows and
// header, then the tables of a width x height scene (0 x 0: none asked for), then whole blocks -- returned -- in what is left, at most nblk, at
// most `cap`.  *fixed_bytes: rows, header and the tables that were granted.  Tables first, whole blocks after: the tables are granted whenever
// they fit beside rows and header.  Rows and header over the 64 KiB budget: nothing (the launch is refused).
uint32_t icp_loop_cu_layout(uint32_t nblk, uint32_t steps, int cap, uint32_t width, uint32_t height, uint32_t waves, uint32_t *fixed_bytes)
{
    const size_t limit = waves >= kLoopWaves ? kLoopCuLdsTotal : kLoopCuLdsTotal / 2;
    const size_t rows = icp_loop_cu_lds_bytes(nblk), block = (size_t)steps * kPointsPerStep * sizeof(pr_vec3);
    size_t tables = (size_t)loop_table_words(width, height) * sizeof(float);
    if (fixed_bytes) *fixed_bytes = (uint32_t)rows;
    if (rows > kLoopCuLdsBudget || rows > limit || block == 0) return 0;
    auto blocks_behind = [&](size_t fixed) {
        const size_t fit = (limit - fixed) / block;
        uint32_t r = (uint32_t)(fit < nblk ? fit : nblk);
        if (cap >= 0 && (uint32_t)cap < r) r = (uint32_t)cap;
        return r;
    };
    if (rows + tables > limit) tables = 0;
    if (fixed_bytes) *fixed_bytes = (uint32_t)(rows + tables);
    return blocks_behind(rows + tables);
}

// the scene as the point work of the loop sees it: the kernel's argument, or (kTables) the same scene with its two tables read from `tab` in LDS
template <bool kTables> struct LoopScene;
template <> struct LoopScene<false> {
    using type = SceneProjPacked;
    static __device__ __forceinline__ const type &make(const SceneProjPacked &sc, const float *) { return sc; }
};
template <> struct LoopScene<true> {
    using type = SceneProjPackedLds;
    static __device__ __forceinline__ type make(const SceneProjPacked &sc, const float *tab) { return type{ sc, tab, tab + sc.width }; }
};

template <uint32_t kWaves, bool kTables>
__device__ __forceinline__ void icp_loop_cu_body(const IcpBatch &b, const SceneProjPacked &scene_arg)
{
    using Scene = typename LoopScene<kTables>::type;
    extern __shared__ __attribute__((aligned(16))) float loop_lds[];
    const uint32_t pose = blockIdx.x;
    const PoseMeta &pm = b.meta[pose];                           // uniform address: one 64-byte scalar load
    const int32_t st0 = pm.state;
    const uint32_t n = pm.count;
    if (st0 == kSkip || n == 0) return;                          // (whole workgroup, ahead of every barrier)
    const uint32_t ppb = b.steps * kPointsPerStep;
    const uint32_t items = ((n + ppb - 1) / ppb) * 4u;           // <= 4 * b.nblk: the cloud fits its pixel box
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *hdr = loop_lds + (size_t)b.nblk * 4 * kAccStride;
    uint32_t *hdw = reinterpret_cast<uint32_t *>(hdr);
    float *cl = reinterpret_cast<float *>(b.cloud + pm.start);
    float *tab = hdr + kLoopHeader;                              // kTables: colf[0 .. width), rowf[0 .. height), rounded up to four words
    float *lcl = tab + (kTables ? loop_table_words(scene_arg.width, scene_arg.height) : 0u);   // the LDS image of points [0, b.lds_blocks * ppb) of the cloud
    const uint32_t lds_items = b.lds_blocks * 4u;
    bool xf = (st0 == kRunWithTransform) && !b.pre_transformed;
    float M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = xf ? pm.xform[i] : 0.0f;
    if (wave == 0 && lane < 20) hdw[16 + lane] = reinterpret_cast<const uint32_t *>(b.st + pose)[lane];
    if constexpr (kTables) {                                     // once per hypothesis and loop: every gather of every pass reads the copy
        const uint32_t w = scene_arg.width, wh = w + scene_arg.height;
        for (uint32_t i = threadIdx.x; i < wh; i += kWaves * 64u) tab[i] = i < w ? scene_arg.colf[i] : scene_arg.rowf[i - w];
        __syncthreads();
    }
    const Scene scene = LoopScene<kTables>::make(scene_arg, tab);
#if PR_LOOP_CU_PROBE
    uint64_t probe_serial = 0, probe_total = 0;
#endif

    const uint32_t last_it = (uint32_t)b.crit.max_iteration;
    uint32_t it = 0;
    for (;; ++it) {
        const bool score_only = it == last_it;                   // uniform: the final pass needs sums 27 and 28 only
#if PR_LOOP_CU_PROBE
        const uint64_t probe_t0 = wall_clock64();
        uint64_t probe_t1 = 0;
#endif
        for (uint32_t item = wave; item < items; item += kWaves) {
            const uint32_t vb = item >> 2, tib = ((item & 3u) << 6) | lane;
            float acc[29];
            float *row = loop_lds + (size_t)item * kAccStride;
            // where the item's points live (uniform): memory, or the LDS image -- filled from memory in pass 0, moved in place from then on.
            // Three call sites per pass kind, each with one address space for its loads and one for its stores.
            const bool in_lds = item < lds_items;
            if (score_only) {
                if (!in_lds) vb_accumulate_at<Scene, false, 0, true>(tib, acc, cl, cl, n, vb * ppb, b.steps, xf, M, scene, nullptr, nullptr, nullptr, nullptr, xf);
                else if (it == 0) vb_accumulate_at<Scene, false, 0, true, false, true>(tib, acc, cl, lcl, n, vb * ppb, b.steps, xf, M, scene, nullptr, nullptr, nullptr, nullptr, xf);
                else vb_accumulate_at<Scene, false, 0, true>(tib, acc, lcl, lcl, n, vb * ppb, b.steps, xf, M, scene, nullptr, nullptr, nullptr, nullptr, xf);
                wave_reduce<true>(acc, lane, row);
            } else {
                if (!in_lds) vb_accumulate_at<Scene, false, 0>(tib, acc, cl, cl, n, vb * ppb, b.steps, xf, M, scene, nullptr, nullptr, nullptr, nullptr, xf);
                else if (it == 0) vb_accumulate_at<Scene, false, 0, false, false, true>(tib, acc, cl, lcl, n, vb * ppb, b.steps, xf, M, scene, nullptr, nullptr, nullptr, nullptr, xf);
                else vb_accumulate_at<Scene, false, 0>(tib, acc, lcl, lcl, n, vb * ppb, b.steps, xf, M, scene, nullptr, nullptr, nullptr, nullptr, xf);
                wave_reduce(acc, lane, row);
            }
        }
        __syncthreads();                                         // every item's row is in LDS
#if PR_LOOP_CU_PROBE
        probe_t1 = wall_clock64();
#endif
        if (wave == 0) {
            float total = 0.0f;
            if (lane < 29) {
                const float *r = loop_lds + lane;
                for (uint32_t i = 0; i < items; i += 4u, r += 4 * kAccStride)
                    total += ((r[0] + r[kAccStride]) + r[2 * kAccStride]) + r[3 * kAccStride];
            }
            DevIcpState s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s.T[i] = hdr[16 + i];
            s.fitness = hdr[32]; s.rmse = hdr[33]; s.done = (int32_t)hdw[34]; s.passes = (int32_t)hdw[35];
            float E[16];
            const bool finished = pose_iteration_wave(total, n, s, b.crit, it, E);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) hdr[16 + i] = s.T[i];
                hdr[32] = s.fitness; hdr[33] = s.rmse; hdw[35] = (uint32_t)s.passes;
                if (!finished) {
#pragma unroll
                    for (int i = 0; i < 12; ++i) hdr[i] = E[i];
                }
                hdw[12] = (finished || it >= last_it) ? 1u : 0u;
            }
        }
#if PR_LOOP_CU_PROBE
        probe_serial += wall_clock64() - probe_t1;               // wavefront 0: the stretch between the two barriers
#endif
        __syncthreads();                                         // update and flag are in LDS; the rows have been read
#if PR_LOOP_CU_PROBE
        probe_total += wall_clock64() - probe_t0;
#endif
        if (__builtin_amdgcn_readfirstlane(hdw[12]) != 0u) break;
#pragma unroll
        for (int i = 0; i < 12; ++i) M[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(hdr[i])));
        xf = true;
    }
    if (threadIdx.x == 0) {                                      // what the multi-launch loop leaves in memory
        DevIcpState s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s.T[i] = hdr[16 + i];
        s.fitness = hdr[32]; s.rmse = hdr[33]; s.done = 1; s.passes = (int32_t)hdw[35];
        b.st[pose] = s;
        PoseMeta *wm = const_cast<PoseMeta *>(b.meta) + pose;
        if (it > 0) {                                            // the update of the last pass that did not finish
#pragma unroll
            for (int i = 0; i < 12; ++i) wm->xform[i] = hdr[i];
        }
        wm->state = kSkip;
#if PR_LOOP_CU_PROBE
        // four floats per hypothesis in the slot's partial buffer (unused on this route): ticks of the 100 MHz wall clock between the barriers and
        // over whole passes, the passes, the items
        float *pr = b.partial + (size_t)pose * 4;
        pr[0] = (float)probe_serial; pr[1] = (float)probe_total; pr[2] = (float)(it + 1u); pr[3] = (float)items;
#endif
    }
}
// 16 wavefronts: the compute unit is the workgroup's own.  8 wavefronts: two workgroups share one -- the cap on the registers (four waves per SIMD,
// at most 128 VGPRs) is what lets the second one in; without it the compiler may take up to 256 and one workgroup would fill the compute unit again.
template <bool kTables>
__global__ __launch_bounds__(kLoopLanes) PR_LOOP_CU_ATTR void icp_loop_cu_kernel(IcpBatch b, SceneProjPacked scene) { icp_loop_cu_body<kLoopWaves, kTables>(b, scene); }
template <bool kTables>
__global__ __launch_bounds__(kLoopLanes / 2) __attribute__((amdgpu_waves_per_eu(4, 4))) void icp_loop_cu8_kernel(IcpBatch b, SceneProjPacked scene) { icp_loop_cu_body<kLoopWaves / 2, kTables>(b, scene); }
hipError_t launch_icp_loop_cu_proj_packed(const IcpBatch &b, const SceneProjPacked &sc, uint32_t n_poses, hipStream_t s, LoopCuForm form, LoopCuUsed *used)
{
    if (used) *used = LoopCuUsed{ 0, 0, 0 };
    if (n_poses == 0 || b.nblk == 0) return hipSuccess;
    const size_t rows = icp_loop_cu_lds_bytes(b.nblk);
    if (rows > kLoopCuLdsBudget || b.robust_kind != PR_ROBUST_NONE) return hipErrorInvalidValue;   // (the caller keeps such batches on the multi-launch loop)
    const uint32_t waves = form.waves == kLoopWaves / 2 ? kLoopWaves / 2 : kLoopWaves;
    // b.lds_blocks is the caller's wish; what is launched never exceeds what icp_loop_cu_layout allows, and falls to none -- and the tables to
    // memory where they do not fit the 64 KiB either -- when the device refuses dynamic LDS beyond 64 KiB
    // the tables by the library's choice (form.tables < 0): in LDS for the 8-wave form, in memory for the 16-wave one (pr_tuning.h has the runs)
    const bool want_tables = form.tables < 0 ? waves != kLoopWaves : form.tables != 0;
    IcpBatch bb = b;
    uint32_t fixed = 0;
    bb.lds_blocks = icp_loop_cu_layout(b.nblk, b.steps, (int)(b.lds_blocks < b.nblk ? b.lds_blocks : b.nblk), want_tables ? sc.width : 0u, want_tables ? sc.height : 0u, waves, &fixed);
    const size_t block = (size_t)b.steps * kPointsPerStep * sizeof(pr_vec3);
    bool tables = fixed > rows;
    const void *fn = waves == kLoopWaves ? (tables ? reinterpret_cast<const void *>(icp_loop_cu_kernel<true>) : reinterpret_cast<const void *>(icp_loop_cu_kernel<false>))
                                         : (tables ? reinterpret_cast<const void *>(icp_loop_cu8_kernel<true>) : reinterpret_cast<const void *>(icp_loop_cu8_kernel<false>));
    const int slot = waves == kLoopWaves ? (tables ? 3 : 0) : (tables ? 5 : 4);
    const size_t limit = waves == kLoopWaves ? kLoopCuLdsTotal : kLoopCuLdsTotal / 2;
    if (fixed + bb.lds_blocks * block > kLoopCuLdsBudget && !lds_opt_in(fn, slot, (uint32_t)limit)) {
        bb.lds_blocks = 0;
        if (fixed > kLoopCuLdsBudget) {                          // (the form without tables is another kernel, and fits without asking)
            tables = false; fixed = (uint32_t)rows;
            fn = waves == kLoopWaves ? reinterpret_cast<const void *>(icp_loop_cu_kernel<false>) : reinterpret_cast<const void *>(icp_loop_cu8_kernel<false>);
        }
    }
    const size_t lds = fixed + bb.lds_blocks * block;
    if (used) *used = LoopCuUsed{ bb.lds_blocks, waves, tables ? fixed - (uint32_t)rows : 0u };
    void *args[] = { &bb, const_cast<SceneProjPacked *>(&sc) };
    return hipLaunchKernel(fn, dim3(n_poses), dim3(waves * 64u), args, lds, s);
}

__global__ __launch_bounds__(64) void icp_finalize_kernel(const float *__restrict__ partial, const PoseMeta *__restrict__ meta,
                                                          uint32_t nblk, uint32_t ppb, float *__restrict__ sums)
{
    const uint32_t pose = blockIdx.x;
    if (meta[pose].state == kSkip) return;
    const uint32_t n = meta[pose].count;
    const uint32_t used = (n + ppb - 1) / ppb;
    if (threadIdx.x < kAccStride)
        sums[(size_t)pose * kAccStride + threadIdx.x] = (threadIdx.x < 29) ? sum_partials(partial, pose, nblk, used, threadIdx.x) : 0.0f;
}

// PR_SOLVE_DEVICE: the per-iteration host logic of icp.cu:178-212 for one hypothesis per wavefront
__global__ __launch_bounds__(64) void icp_finalize_solve_kernel(const float *__restrict__ partial, PoseMeta *__restrict__ meta,
                                                                uint32_t nblk, uint32_t ppb, DevIcpState *__restrict__ st,
                                                                pr_criteria crit, uint32_t iter)
{
    const uint32_t pose = blockIdx.x;
    if (meta[pose].state == kSkip) return;
    const uint32_t n = meta[pose].count;
    const uint32_t used = (n + ppb - 1) / ppb;
    DevIcpState s = st[pose];
    float total = 0.0f;
    if (threadIdx.x < 29) total = sum_partials(partial, pose, nblk, used, threadIdx.x);
    float E[16];
    const bool finished = pose_iteration_wave(total, n, s, crit, iter, E);
    if (threadIdx.x != 0) return;
    if (finished) { s.done = 1; meta[pose].state = kSkip; }
    else {
#pragma unroll
        for (int i = 0; i < 12; ++i) meta[pose].xform[i] = E[i];
        meta[pose].state = kRunWithTransform;
    }
    st[pose] = s;
}

__global__ void pack_results_kernel(const DevIcpState *__restrict__ st, pr_result *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pr_result r;
    for (int k = 0; k < 16; ++k) r.T[k] = st[i].T[k];
    r.inlier_rmse = st[i].rmse; r.fitness = st[i].fitness;
    out[i] = r;
}
// results to the device buffer and, in the same launch, results / cloud sizes to pinned host staging (stores over the host link)
__global__ void pack_export_kernel(const DevIcpState *__restrict__ st, pr_result *__restrict__ out, const uint32_t *__restrict__ counts,
                                   uint32_t *__restrict__ host_counts, pr_result *__restrict__ host_results, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pr_result r;
    for (int k = 0; k < 16; ++k) r.T[k] = st[i].T[k];
    r.inlier_rmse = st[i].rmse; r.fitness = st[i].fitness;
    out[i] = r;
    host_counts[i] = counts[i];
    if (host_results) host_results[i] = r;
}
// small host-staged inputs (poses, pixel boxes) pulled into device memory by a kernel: an SDMA copy of 20 KB costs ~20 us of latency
__global__ void stage_words_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint32_t n16)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}

// the same in 8-byte words, for records whose total is no multiple of 16 (72-byte results): never a byte beyond the destination
__global__ void stage_words64_kernel(const uint2 *__restrict__ src, uint2 *__restrict__ dst, uint32_t n8)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n8) dst[i] = src[i];
}

template <class Scene, bool kNN, int kStack = 0, bool kRobust = false>
static hipError_t launch_pass(const IcpBatch &b, const Scene &sc, uint32_t n_poses, size_t lds_bytes, hipStream_t s)
{
    if (n_poses == 0 || b.nblk == 0) return hipSuccess;
    for (uint32_t p0 = 0; p0 < n_poses; p0 += 32768) {
        const uint32_t np = (n_poses - p0 < 32768) ? (n_poses - p0) : 32768;
        IcpBatch bb = b;
        bb.meta += p0;
        bb.partial += (size_t)p0 * b.nblk * kAccStride;
        if (bb.st) bb.st += p0;                                  // everything indexed by the hypothesis moves with the piece
        if (bb.arrive) bb.arrive += p0;
        if (bb.sums_out) bb.sums_out += (size_t)p0 * kAccStride;
        if (bb.nn_qcount) bb.nn_qcount += kQCountStride * (size_t)p0;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(icp_pass_kernel<Scene, kNN, kStack, kRobust>), dim3(b.grid_x ? b.grid_x : b.nblk, np), dim3(kBlockThreads), lds_bytes, s, bb, sc);
    }
    return hipGetLastError();
}
hipError_t launch_icp_pass_proj_aos(const IcpBatch &b, const SceneProjAoS &sc, uint32_t n_poses, hipStream_t s)
{ return b.robust_kind != PR_ROBUST_NONE ? launch_pass<SceneProjAoS, false, 0, true>(b, sc, n_poses, 0, s) : launch_pass<SceneProjAoS, false>(b, sc, n_poses, 0, s); }
// (Round 5 measured the two tables colf / rowf of the packed scene staged in LDS per workgroup -- two of a point's three gathers off the texture
// addresser: 0.84 against 0.82 ms per 21 launches, 272 / 263 k against 277 / 276 k poses/s on one box.  Not kept.)
hipError_t launch_icp_pass_proj_packed(const IcpBatch &b, const SceneProjPacked &sc, uint32_t n_poses, hipStream_t s)
{ return b.robust_kind != PR_ROBUST_NONE ? launch_pass<SceneProjPacked, false, 0, true>(b, sc, n_poses, 0, s) : launch_pass<SceneProjPacked, false>(b, sc, n_poses, 0, s); }
// the stackless walk (plain or robust instantiation, opt-in slots 1 and 2): the staged count never exceeds the tree or kNNLdsNodesMax whatever the
// caller's record says, and falls to kNNLdsNodesPlain when the device refuses dynamic LDS beyond 64 KiB
template <bool kRobust>
static hipError_t launch_pass_nn_stackless(const IcpBatch &b, const SceneNNDev &sc, uint32_t n_poses, hipStream_t s, NNPassRan *ran)
{
    SceneNNDev ss = sc;
    ss.lds_nodes = sc.topo_nodes;                                // (sc.lds_nodes counts 64-byte records when sc.stack_depth selects a stack walk: the robust pass of such a scene)
    if (ss.lds_nodes > ss.n_nodes) ss.lds_nodes = ss.n_nodes;
    if (ss.lds_nodes > kNNLdsNodesMax) ss.lds_nodes = kNNLdsNodesMax;
    const auto fn = icp_pass_kernel<SceneNNDev, true, 0, kRobust>;
    if (ss.lds_nodes > kNNLdsNodesPlain && !lds_opt_in(reinterpret_cast<const void *>(fn), kRobust ? 2 : 1, kNNLdsNodesMax * (uint32_t)sizeof(int4))) ss.lds_nodes = kNNLdsNodesPlain;
    if (ran) *ran = NNPassRan{ ss.lds_nodes, 0u };
    return launch_pass<SceneNNDev, true, 0, kRobust>(b, ss, n_poses, (size_t)ss.lds_nodes * sizeof(int4), s);
}
// the per-lane-stack walk on exact 64-byte records: stacks + staged records + the kernel's static LDS stay within 64 KiB (nn_route's cap, held here too)
template <int kDepth>
static hipError_t launch_pass_nn_stack_exact(const IcpBatch &b, const SceneNNDev &sc, uint32_t n_poses, hipStream_t s, NNPassRan *ran)
{
    constexpr uint32_t stacks = (uint32_t)kDepth * kBlockThreads * 8u, most = ((64u << 10) - kPassStaticLds - stacks) / 64u;
    SceneNNDev ss = sc;
    if (ss.lds_nodes > ss.n_nodes) ss.lds_nodes = ss.n_nodes;
    if (ss.lds_nodes > most) ss.lds_nodes = most;
    if (ran) *ran = NNPassRan{ ss.lds_nodes, (uint32_t)kDepth };
    return launch_pass<SceneNNDev, true, kDepth>(b, ss, n_poses, (size_t)stacks + (size_t)ss.lds_nodes * 64, s);
}
hipError_t launch_icp_pass_nn(const IcpBatch &b, const SceneNNDev &sc, uint32_t n_poses, hipStream_t s, NNPassRan *ran)
{
    // a robust pass that searches in the pass (a scene without compact records: with them the driver takes the split route) walks stackless,
    // the one in-pass walk instantiated with the weight; every walk returns the same winners
    if (b.robust_kind != PR_ROBUST_NONE) return launch_pass_nn_stackless<true>(b, sc, n_poses, s, ran);
    if ((sc.stack_depth == 16 || sc.stack_depth == 24) && sc.rec32) {                         // compact records: the stacks alone
        if (ran) *ran = NNPassRan{ 0u, sc.stack_depth };
        if (sc.stack_depth == 16) return launch_pass<SceneNNDev, true, 16 + 0x100>(b, sc, n_poses, (size_t)16 * kBlockThreads * 8, s);
        return launch_pass<SceneNNDev, true, 24 + 0x100>(b, sc, n_poses, (size_t)24 * kBlockThreads * 8, s);
    }
    if (sc.stack_depth == 16) return launch_pass_nn_stack_exact<16>(b, sc, n_poses, s, ran);
    if (sc.stack_depth == 24) return launch_pass_nn_stack_exact<24>(b, sc, n_poses, s, ran);
    return launch_pass_nn_stackless<false>(b, sc, n_poses, s, ran);
}

hipError_t launch_icp_pass_nn_winners(const IcpBatch &b, const SceneNNWinners &sc, uint32_t n_poses, hipStream_t s)
{ return b.robust_kind != PR_ROBUST_NONE ? launch_pass<SceneNNWinners, true, -1, true>(b, sc, n_poses, 0, s) : launch_pass<SceneNNWinners, true, -1>(b, sc, n_poses, 0, s); }

hipError_t launch_icp_finalize(const float *partial, const PoseMeta *meta, uint32_t nblk,
                               uint32_t steps, float *sums, uint32_t n_poses, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    hipLaunchKernelGGL(icp_finalize_kernel, dim3(n_poses), dim3(64), 0, s, partial, meta, nblk, steps * kPointsPerStep, sums);
    return hipGetLastError();
}
hipError_t launch_icp_finalize_solve(const float *partial, PoseMeta *meta, uint32_t nblk,
                                     uint32_t steps, DevIcpState *st, pr_criteria crit, uint32_t iter,
                                     uint32_t n_poses, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    hipLaunchKernelGGL(icp_finalize_solve_kernel, dim3(n_poses), dim3(64), 0, s, partial, meta, nblk,
                       steps * kPointsPerStep, st, crit, iter);
    return hipGetLastError();
}
hipError_t launch_pack_export(const DevIcpState *st, pr_result *out, const uint32_t *counts, uint32_t *host_counts, pr_result *host_results,
                              uint32_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_export_kernel, dim3((n + 255) / 256), dim3(256), 0, s, st, out, counts, host_counts, host_results, n);
    return hipGetLastError();
}
hipError_t launch_stage_words(const void *src_host_mapped, void *dst, size_t bytes, hipStream_t s)
{
    const uint32_t n16 = (uint32_t)((bytes + 15) / 16);
    if (n16 == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_words_kernel, dim3((n16 + 255) / 256), dim3(256), 0, s, static_cast<const uint4 *>(src_host_mapped), static_cast<uint4 *>(dst), n16);
    return hipGetLastError();
}
// 4-byte words, either direction (device -> pinned host too: small read-backs without a copy command)
__global__ void copy_words32_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
hipError_t launch_copy_words32(const void *src, void *dst, uint32_t n_words, hipStream_t s)
{
    if (n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(copy_words32_kernel, dim3((n_words + 255) / 256), dim3(256), 0, s, static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst), n_words);
    return hipGetLastError();
}
hipError_t launch_stage_words64(const void *src_host_mapped, void *dst, size_t bytes, hipStream_t s)
{
    if (bytes % 8) return hipErrorInvalidValue;
    const uint32_t n8 = (uint32_t)(bytes / 8);
    if (n8 == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_words64_kernel, dim3((n8 + 255) / 256), dim3(256), 0, s, static_cast<const uint2 *>(src_host_mapped), static_cast<uint2 *>(dst), n8);
    return hipGetLastError();
}
hipError_t launch_pack_results(const DevIcpState *st, pr_result *out, uint32_t n_poses, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    hipLaunchKernelGGL(pack_results_kernel, dim3((n_poses + 255) / 256), dim3(256), 0, s, st, out, n_poses);
    return hipGetLastError();
}

}  // namespace prk
