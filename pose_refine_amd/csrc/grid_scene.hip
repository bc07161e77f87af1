// grid_scene.hip -- the closest-point grid scene (pr_scene_grid, include/pose_refine.h; no counterpart in the reference): its build from a kd-tree
// scene, its correspondence pass and its per-point audit entry
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-element value is bit-identical to the CPU restatement.
//
// All hypotheses of a frame query the SAME scene, 10^8 times per frame; every kd-tree query is a fresh descent.  The grid spends the exact search
// once per cell and frame (grid_build_kernel) and turns every later query into arithmetic, one 4-byte gather (the cell's scene point) and one
// 32-byte record gather (that point and its normal): the projective pass' shape with nearest-neighbour semantics.
#include "pr_launch.h"
#include "icp_accumulate.h"
#include "icp_solve_device.h"

namespace prk {

// ---- the definition, in one place each (include/pose_refine.h states it; tests/grid_ref.py restates it in numpy) ---------------------------
// cell of a point: per axis f = (p - origin) * inv_cell, inside iff 0 <= f < dim (a NaN or an infinity fails one of the two), i = (int)f
__device__ __forceinline__ bool grid_cell_of(const SceneGridDev &s, float x, float y, float z, uint32_t &idx)
{
    const float fx = (x - s.origin[0]) * s.inv_cell, fy = (y - s.origin[1]) * s.inv_cell, fz = (z - s.origin[2]) * s.inv_cell;
    const bool inside = fx >= 0.0f && fx < (float)s.dim[0] && fy >= 0.0f && fy < (float)s.dim[1] && fz >= 0.0f && fz < (float)s.dim[2];
    // (the conversions of an outside value saturate harmlessly: idx is only used when the test passed)
    idx = inside ? (uint32_t)(int)fx + s.dim[0] * ((uint32_t)(int)fy + s.dim[1] * (uint32_t)(int)fz) : 0u;
    return inside;
}
// acceptance of a gathered record: ((ex*ex + ey*ey) + ez*ez) < max_dist_diff^2 with e = d - p (accumulate() forms the same e and the same sum)
__device__ __forceinline__ bool grid_accept(const SceneGridDev &s, float sx, float sy, float sz, const float4 d)
{
    const float ex = d.x - sx, ey = d.y - sy, ez = d.z - sz;
    return (ex * ex + ey * ey + ez * ez) < s.max_dist_diff * s.max_dist_diff;
}

// ================================================================================================
//  build: one lane per cell, the exact search of the scene's kd-tree from the cell's centre
// ================================================================================================
// The ordered stackless walk of Scene_nn::query (nn_walk_stackless, nn_query.h), started from the bound reach^2: it visits a leaf point only while
// a strictly nearer one is possible, compares with '<', and so returns the first point -- in the tree's own visiting order -- that attains the
// minimum squared distance (pcd_scene.h:87-90) among the points nearer than `reach`, or nothing: the definition's winner (any point of a tie is
// allowed) and its PR_GRID_NONE rule (minimum < reach * reach, the product in float32) at once.  The walk depends on nothing but the tree and
// the centre, so two builds give the same bytes.  Cells far from the surface end at the root's box; cells near it cost one descent.
__global__ __launch_bounds__(256) void grid_build_kernel(SceneNNDev tree, SceneGridDev grid, uint32_t *__restrict__ cell_point)
{
    const uint32_t nx = grid.dim[0], ny = grid.dim[1], nz = grid.dim[2];
    const size_t cells = (size_t)nx * ny * nz;                   // <= PR_GRID_MAX_CELLS
    const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (c >= cells) return;
    const uint32_t ix = (uint32_t)(c % nx), iy = (uint32_t)((c / nx) % ny), iz = (uint32_t)(c / ((size_t)nx * ny));
    const float cx = grid.origin[0] + ((float)ix + 0.5f) * grid.cell;
    const float cy = grid.origin[1] + ((float)iy + 0.5f) * grid.cell;
    const float cz = grid.origin[2] + ((float)iz + 0.5f) * grid.cell;
    // tree.max_dist_diff carries `reach` here (launch_grid_build): the walk's own acceptance test is the definition's
    cell_point[c] = query_nn_bounded(tree, cx, cy, cz, tree.max_dist_diff * tree.max_dist_diff);
}
static_assert(kNoPrev == PR_GRID_NONE, "the walk's \"no point\" is the grid's empty cell");

// rec[k] = {px, py, pz, 0, nx, ny, nz, 0}: one 32-byte record per scene point, two aligned 16-byte loads per correspondence
__global__ __launch_bounds__(256) void grid_records_kernel(const pr_vec3 *__restrict__ pcd, const pr_vec3 *__restrict__ normal, uint32_t n, float4 *__restrict__ rec)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const pr_vec3 p = pcd[i], q = normal[i];
    rec[2 * (size_t)i] = make_float4(p.x, p.y, p.z, 0.0f);
    rec[2 * (size_t)i + 1] = make_float4(q.x, q.y, q.z, 0.0f);
}

hipError_t launch_grid_build(const SceneNNDev &tree, float reach, const SceneGridDev &grid, uint32_t *cell_point, hipStream_t s)
{
    const size_t cells = (size_t)grid.dim[0] * grid.dim[1] * grid.dim[2];
    if (cells == 0) return hipSuccess;
    SceneNNDev t = tree;
    t.max_dist_diff = reach;
    hipLaunchKernelGGL(grid_build_kernel, dim3((uint32_t)((cells + 255) / 256)), dim3(256), 0, s, t, grid, cell_point);
    return hipGetLastError();
}
hipError_t launch_grid_records(const pr_vec3 *pcd, const pr_vec3 *normal, uint32_t n, float4 *rec, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(grid_records_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pcd, normal, n, rec);
    return hipGetLastError();
}

// ================================================================================================
//  the correspondence pass: pending transform + grid lookup + 29-term transform-reduce
// ================================================================================================
// One virtual workgroup of the canonical tree, as vb_accumulate (icp_accumulate.h) walks it: lane t takes points first + s*1024 + i*256 + t,
// i = 0..3, of every 1024-point step.  Per step: the four points in (contiguous 12-byte loads), the pending update applied, ALL FOUR cell-index
// loads issued, then ALL FOUR record loads (two float4 each; record 0 stands in for a lane without a winner), and only then the tests and the
// accumulation: two dependent memory round trips per step, not eight.
template <bool kScoreOnly, bool kRobust = false>
__device__ __forceinline__ void grid_vb_accumulate(float (&acc_out)[29], float *cl, uint32_t n, uint32_t first, uint32_t steps, bool xf,
                                                   const float (&M)[12], const SceneGridDev &scene, const RobustW &rb = RobustW{})
{
    (void)rb;
    Acc29 acc;
    acc_clear(acc);
    const uint32_t last = n - 1u;                                // n >= 1 here: the workgroup has points
    for (uint32_t s = 0; s < steps; ++s) {
        const uint32_t j0 = first + s * kPointsPerStep + threadIdx.x;
        if (j0 >= n) break;
        const uint32_t left = (n - j0 + kBlockThreads - 1u) / kBlockThreads;
        const uint32_t cnt = left < kPointsPerLane ? left : kPointsPerLane;
        float p[12];
        // unconditional loads (a lane past the end re-reads the cloud's last point and never uses it: `i < cnt` gates every use)
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t j = j0 + i * kBlockThreads;
            const pr_vec3 v = ld_off<pr_vec3>(cl, (j < last ? j : last) * 12u);
            p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z;
        }
        if (xf) {                                                // icp.cu:142-153 transform_pcd_cuda, fused: the packed arithmetic of vb_accumulate, ((m0*x + m1*y) + m2*z) + m3
            const float2v Mx{ M[0], M[4] }, My{ M[1], M[5] }, Mz{ M[2], M[6] }, Mt{ M[3], M[7] };
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
                float2v t = Mx * float2v{ x, x };
                t = t + My * float2v{ y, y };
                t = t + Mz * float2v{ z, z };
                t = t + Mt;
                p[3 * i]     = t.x;
                p[3 * i + 1] = t.y;
                p[3 * i + 2] = M[8] * x + M[9] * y + M[10] * z + M[11];
            }
        }
        auto store_back = [&]() {
            if (!xf) return;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i)
                if (i < cnt) st_off<pr_vec3>(cl, (j0 + i * kBlockThreads) * 12u, pr_vec3{ p[3 * i], p[3 * i + 1], p[3 * i + 2] });
        };
#if !PR_PASS_LATE_STORE
        store_back();
#endif
        // round trip 1: the four cells' scene points (cell 0 for a point that is outside or past the end)
        bool in_grid[4];
        uint32_t w[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            uint32_t idx;
            in_grid[i] = grid_cell_of(scene, p[3 * i], p[3 * i + 1], p[3 * i + 2], idx) && i < cnt;
            w[i] = ld_off<uint32_t>(scene.cell_point, (in_grid[i] ? idx : 0u) * 4u);
        }
        // round trip 2: their records
        float4 d[4], nr[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            if (!in_grid[i]) w[i] = PR_GRID_NONE;
            const uint32_t at = (w[i] != PR_GRID_NONE) ? w[i] : 0u;
            d[i] = ld_off<float4>(scene.rec, at * 32u);            // (n_points < 2^27, make_scene: the byte offset fits 32 bits)
            nr[i] = ld_off<float4>(scene.rec, at * 32u + 16u);
        }
#if PR_PASS_LATE_STORE
        store_back();                                            // (behind the step's gathers, as the projective pass issues it: pr_tuning.h has the measurement)
#endif
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            if (w[i] != PR_GRID_NONE && grid_accept(scene, p[3 * i], p[3 * i + 1], p[3 * i + 2], d[i])) {
                Corr c; c.dx = d[i].x; c.dy = d[i].y; c.dz = d[i].z; c.nx = nr[i].x; c.ny = nr[i].y; c.nz = nr[i].z;
                accumulate_point<kScoreOnly, kRobust>(acc, p[3 * i], p[3 * i + 1], p[3 * i + 2], c, rb);
            }
        }
    }
    acc_export(acc, acc_out);
}

// grid = (workgroups per hypothesis, hypotheses), 256 lanes: icp_pass_kernel's frame (icp_pass.hip) around the grid's own point loop
template <bool kRobust = false>
__global__ __launch_bounds__(256, PR_GRID_PASS_WAVES) void icp_pass_grid_kernel(IcpBatch b, SceneGridDev scene)
{
    __shared__ float wsum[4][kAccStride];

    const uint32_t pose = blockIdx.y;
    const PoseMeta &pm = b.meta[pose];                           // uniform address: one 64-byte scalar load
    const int32_t st = pm.state;
    if (st == kSkip) return;
    const uint32_t n = pm.count;
    const uint32_t ppb = b.steps * kPointsPerStep;
    if ((uint64_t)blockIdx.x * ppb >= n) return;

    float *cl = reinterpret_cast<float *>(b.cloud + pm.start);
    const bool xf = (st == kRunWithTransform) && !b.pre_transformed;
    float M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = xf ? pm.xform[i] : 0.0f;

    const uint32_t used = (n + ppb - 1) / ppb;
    for (uint32_t vb = blockIdx.x; vb < used; vb += gridDim.x) {
        if (vb != blockIdx.x) __syncthreads();                   // wsum of the previous trip has been read
        float acc[29];
#pragma unroll
        for (int i = 0; i < 29; ++i) acc[i] = 0.0f;
        float t;
        if (b.score_only) {                                      // uniform: the final pass needs sums 27 and 28 only
            grid_vb_accumulate<true>(acc, cl, n, vb * ppb, b.steps, xf, M, scene);
            t = vb_reduce<true>(acc, wsum);
        } else {
            if constexpr (kRobust) grid_vb_accumulate<false, true>(acc, cl, n, vb * ppb, b.steps, xf, M, scene, RobustW{ b.robust_kind, b.robust_c, b.robust_inv_c });
            else grid_vb_accumulate<false>(acc, cl, n, vb * ppb, b.steps, xf, M, scene);
            t = vb_reduce(acc, wsum);
        }
        if (pass_deliver(b, pose, vb, used, n, t)) return;
    }
}

hipError_t launch_icp_pass_grid(const IcpBatch &b, const SceneGridDev &sc, uint32_t n_poses, hipStream_t s)
{
    if (n_poses == 0 || b.nblk == 0) return hipSuccess;
    for (uint32_t p0 = 0; p0 < n_poses; p0 += 32768) {           // (the pieces of launch_pass, icp_pass.hip: everything indexed by the hypothesis moves with the piece)
        const uint32_t np = (n_poses - p0 < 32768) ? (n_poses - p0) : 32768;
        IcpBatch bb = b;
        bb.meta += p0;
        bb.partial += (size_t)p0 * b.nblk * kAccStride;
        if (bb.st) bb.st += p0;
        if (bb.arrive) bb.arrive += p0;
        if (bb.sums_out) bb.sums_out += (size_t)p0 * kAccStride;
        if (b.robust_kind != PR_ROBUST_NONE) hipLaunchKernelGGL(icp_pass_grid_kernel<true>, dim3(b.grid_x ? b.grid_x : b.nblk, np), dim3(kBlockThreads), 0, s, bb, sc);
        else hipLaunchKernelGGL(icp_pass_grid_kernel<false>, dim3(b.grid_x ? b.grid_x : b.nblk, np), dim3(kBlockThreads), 0, s, bb, sc);
    }
    return hipGetLastError();
}

// ================================================================================================
//  audit entry: the 29 terms of every point of one cloud (pr_debug_contrib29), one lane per point
// ================================================================================================
struct GridUpdate12 { float m[12]; };
template <bool kRobust = false, class... Robust>                  // Robust: nothing, or (kRobust) one RobustArgs
__global__ __launch_bounds__(256) void contrib29_grid_kernel(pr_vec3 *__restrict__ cloud, uint32_t n, int apply, GridUpdate12 u, SceneGridDev scene, float *__restrict__ out, Robust... ra)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    pr_vec3 p = cloud[i];
    if (apply) { p = transform_point(u.m, p); cloud[i] = p; }    // the fused pass' operand order
    Acc29 acc;
    acc_clear(acc);
    Corr found{}; float wt = 0.0f; bool valid = false;            // (kRobust: what pr_debug_robust_terms reports beside the terms)
    (void)found; (void)wt; (void)valid;
    uint32_t idx;
    if (grid_cell_of(scene, p.x, p.y, p.z, idx)) {
        const uint32_t w = scene.cell_point[idx];
        if (w != PR_GRID_NONE) {
            const float4 d = scene.rec[2 * (size_t)w], nr = scene.rec[2 * (size_t)w + 1];
            if (grid_accept(scene, p.x, p.y, p.z, d)) {
                Corr c; c.dx = d.x; c.dy = d.y; c.dz = d.z; c.nx = nr.x; c.ny = nr.y; c.nz = nr.z;
                if constexpr (kRobust) { const RobustArgs &a = (ra, ...); wt = accumulate_weighted(acc, p.x, p.y, p.z, c, RobustW{ a.kind, a.c, a.inv_c }); found = c; valid = true; }
                else accumulate(acc, p.x, p.y, p.z, c);
            }
        }
    }
    if constexpr (kRobust) { const RobustArgs &a = (ra, ...); if (a.corr) robust_store_corr(a.corr + (size_t)i * 8, valid, found, wt); }
    float t[29];
    acc_export(acc, t);
#pragma unroll
    for (int k = 0; k < 29; ++k) out[(size_t)i * 29 + k] = t[k];
}
hipError_t launch_contrib29_grid(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneGridDev &sc, float *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    GridUpdate12 u{};
    if (update12) for (int k = 0; k < 12; ++k) u.m[k] = update12[k];
    hipLaunchKernelGGL(contrib29_grid_kernel<>, dim3((n + 255) / 256), dim3(256), 0, s, cloud, n, update12 ? 1 : 0, u, sc, out);
    return hipGetLastError();
}
hipError_t launch_robust_terms_grid(pr_vec3 *cloud, uint32_t n, const float *update12, const SceneGridDev &sc, const RobustArgs &ra, float *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    GridUpdate12 u{};
    if (update12) for (int k = 0; k < 12; ++k) u.m[k] = update12[k];
    hipLaunchKernelGGL(HIP_KERNEL_NAME(contrib29_grid_kernel<true, RobustArgs>), dim3((n + 255) / 256), dim3(256), 0, s, cloud, n, update12 ? 1 : 0, u, sc, out, ra);
    return hipGetLastError();
}

}  // namespace prk
