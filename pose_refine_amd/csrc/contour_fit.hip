// contour_fit.hip -- contour alignment (pr_contour_information, include/pose_refine.h; no counterpart in the reference): the silhouette's normal
// equations of every rendered box of a batch (launch_render_boxes) in pr_pose_info's coordinates -- the edge pixels of the render against the
// scene's nearest-edge map (contour.hip) -- and the kernel that adds the workgroups' partial sums in block order into the records.
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-pixel value is the one tests/contour_fit_ref.py forms with the same operations.
#include "score_walk.h"
#include "contour_fit.h"

namespace prk {

// One row of a used pixel.  The operations, in this order and each rounded on its own, ARE the definition (include/pose_refine.h):
//   a = (qy*nz - qz*ny, qz*nx - qx*nz, qx*ny - qy*nx) / rho;  J = (a, n);  H[i][j] += J[i] * J[j] (i <= j);  g[i] += J[i] * res;  sum_r2 += res * res
// Every index is a compile-time constant after unrolling: the 28 sums stay in registers.
__device__ __forceinline__ void fit_row(double (&acc)[kFitSums], double qx, double qy, double qz, double nx, double ny, double nz, double res, double rho)
{
    double J[6];
    J[0] = (qy * nz - qz * ny) / rho;
    J[1] = (qz * nx - qx * nz) / rho;
    J[2] = (qx * ny - qy * nx) / rho;
    J[3] = nx; J[4] = ny; J[5] = nz;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) { acc[k] += J[i] * J[j]; ++k; }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i] * res;
    acc[27] += res * res;
}

// contour_box_kernel's walk (contour.hip): one workgroup = 16 image rows of one hypothesis' box, 4 wavefronts x 4 rows, lanes along a row, the left and
// right neighbours from the neighbouring lanes.  A contour pixel (a few per cent of a box) reads the scene and the nearest-edge word, and a used
// one adds its two rows to the lane's 28 float64 sums.  The counters go the contour check's way (block_totals, one integer atomic per counter and
// workgroup: exact); the float64 sums through a fixed tree -- lanes pairwise by shuffles (offsets 32 .. 1), the four wavefronts as
// ((w0 + w1) + w2) + w3 -- into partial[hypothesis][blockIdx.x][kFitSums], which fit_reduce_kernel adds in block order.  No floating-point atomics.
// A workgroup covers image rows 16 b .. 16 b + 15 whatever the batch is, and a lane's pixels depend on the hypothesis' own box alone: a record does
// not depend on how the batch is chunked or on what else is in it.
// sum_d2: a workgroup covers kBoxRowsPerBlock rows x <= kFitMaxFrameSide columns of d^2 <= 2 * 32^2, so its sum fits 32 bits.
static_assert(kFitRowsPerBlock == kBoxRowsPerBlock, "contour_fit.h states the box walk's rows per workgroup");
constexpr uint64_t kFitMaxFrameSide = 8192;                       // frame_size_ok (pr_runtime.h) refuses wider or taller frames
static_assert(kBoxRowsPerBlock * kFitMaxFrameSide * 2 * PR_CONTOUR_MAX_RADIUS * PR_CONTOUR_MAX_RADIUS < (1ull << 32), "contour_fit_kernel: a workgroup's sum_d2 must fit 32 bits");
template <typename SceneT>
__global__ __launch_bounds__(256) void contour_fit_kernel(const int32_t *__restrict__ depth, const int4 *__restrict__ bbox, uint32_t width, uint32_t height,
                                                          const uint32_t *__restrict__ box_off, const int4 win, const SceneT *__restrict__ scene,
                                                          const uint32_t *__restrict__ nearest, const FitMeta *__restrict__ meta, const FitParams pm,
                                                          uint32_t *__restrict__ records, double *__restrict__ partial)
{
    __shared__ double wsum[4][kFitSums];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    BoxBlock blk;
    if (!box_block(bbox, height, blk)) return;
    const auto [bb, r_lo, r_hi, row0] = blk;
    const int64_t t = pm.tau, jump = pm.jump;
    const FitMeta mt = meta[blockIdx.y];
    const double ccx = (double)mt.c[0], ccy = (double)mt.c[1], ccz = (double)mt.c[2], rho = (double)mt.rho;
    const int32_t *line[6];
    int32_t off_box[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int row = row0 - 1 + k;
        const bool in_box = row >= r_lo && row <= r_hi;
        line[k] = in_box ? box_line(const_cast<int32_t *>(depth), box_off, bb, blockIdx.y, (uint32_t)row, width, height) : depth;
        off_box[k] = in_box ? 1 : ((row >= win.y && row <= win.w) ? 0 : kNoNeighbour);
    }
    auto value = [](int32_t d) { return rendered(d) ? d : 0; };
    uint32_t con = 0, use = 0, occ = 0, mis = 0, d2sum = 0;
    double acc[kFitSums];
#pragma unroll
    for (int i = 0; i < (int)kFitSums; ++i) acc[i] = 0.0;
    for (int x0 = bb.x; x0 <= bb.z; x0 += 64) {
        const int x = x0 + (int)lane;
        const bool in_x = x <= bb.z;
        const int xe = lane == 0 ? x0 - 1 : x0 + 64;
        const bool ends = lane == 0 || lane == 63;
        const int32_t side_out = (xe >= win.x && xe <= win.z) ? 0 : kNoNeighbour;
        const bool side_in = ends && xe >= bb.x && xe <= bb.z;
        int32_t v[6], e[4];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = (off_box[k] == 1) ? (in_x ? value(line[k][x]) : ((x <= win.z) ? 0 : kNoNeighbour)) : off_box[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = (off_box[k + 1] == 1 && side_in) ? value(line[k + 1][xe]) : side_out;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int32_t c = v[k + 1];
            const int32_t up = __shfl_up(c, 1), dn = __shfl_down(c, 1);
            const int32_t l = lane == 0 ? e[k] : up, r = lane == 63 ? e[k] : dn;
            if (!(off_box[k + 1] == 1 && in_x && c > 0)) continue;
            if (!(edge_trigger(c, l, jump) || edge_trigger(c, r, jump) || edge_trigger(c, v[k], jump) || edge_trigger(c, v[k + 2], jump))) continue;
            const int y = row0 + k;
            const size_t px = (size_t)y * width + (size_t)x;
            const int32_t s = (int32_t)scene[px];
            const uint32_t N = nearest[px];
            ++con;
            if (depth_class(c, s, t) == 1) { ++occ; continue; }
            if (N == PR_EDGE_NONE) { ++mis; continue; }
            const int ex = (int)(N & 0xffffu), ey = (int)(N >> 16);
            const int ddx = ex - x, ddy = ey - y;
            ++use;
            d2sum += (uint32_t)(ddx * ddx + ddy * ddy);
            const double Z = (double)c / 1000.0;
            const double ux = (double)x - pm.cx, uy = (double)y - pm.cy;
            const double qx = ux * Z / pm.fx - ccx, qy = uy * Z / pm.fy - ccy, qz = Z - ccz;
            fit_row(acc, qx, qy, qz, 1.0, 0.0, -(ux / pm.fx), (double)ddx * Z / pm.fx, rho);
            fit_row(acc, qx, qy, qz, 0.0, 1.0, -(uy / pm.fy), (double)ddy * Z / pm.fy, rho);
        }
    }
    const uint32_t cnt[5] = { con, use, occ, mis, d2sum };
    const uint32_t sum = block_totals(cnt), k = threadIdx.x;
    uint32_t *rec = records + (size_t)blockIdx.y * 8;
    if (sum && k < 4) atomicAdd(rec + k, sum);
    else if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(rec + 6), (unsigned long long)sum);      // (k == 4: the others' totals are 0)
#pragma unroll
    for (int i = 0; i < (int)kFitSums; ++i) {
        double a = acc[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) wsum[wave][i] = a;
    }
    __syncthreads();
    if (k < kFitSums) partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kFitSums + k] = ((wsum[0][k] + wsum[1][k]) + wsum[2][k]) + wsum[3][k];
}

// 32 lanes per hypothesis, lane i < 28 adds sum i over the workgroups that wrote one (those whose 16 rows meet the box: box_block's test), in block order;
// lane 28 writes the counts, the centre and sum_w = 2 * used.  The record goes where `info` points (the pinned block: no copy command).
__global__ __launch_bounds__(256) void fit_reduce_kernel(const double *__restrict__ partial, const int4 *__restrict__ bbox, const FitMeta *__restrict__ meta,
                                                         const uint32_t *__restrict__ records, uint32_t nblk, uint32_t height, uint32_t n_poses,
                                                         pr_pose_info *__restrict__ info)
{
    const uint32_t pose = blockIdx.x * 8u + (threadIdx.x >> 5), i = threadIdx.x & 31u;
    if (pose >= n_poses) return;
    pr_pose_info *o = info + pose;
    if (i < kFitSums) {
        const int4 bb = bbox[pose];
        const int r_lo = (int)height - 1 - bb.w, r_hi = (int)height - 1 - bb.y;
        double sum = 0.0;
        if (!(bb.x > bb.z || r_lo > r_hi || r_hi < 0)) {
            const uint32_t b_lo = (uint32_t)(r_lo > 0 ? r_lo : 0) / kBoxRowsPerBlock, b_hi = min((uint32_t)r_hi / kBoxRowsPerBlock, nblk - 1u);
            for (uint32_t b = b_lo; b <= b_hi; ++b) sum += partial[((size_t)pose * nblk + b) * kFitSums + i];
        }
        if (i < 21) o->H[i] = sum;
        else if (i < 27) o->g[i - 21] = sum;
        else { o->sum_wr2 = sum; o->sum_r2 = sum; }
    } else if (i == kFitSums) {
        const uint32_t *rec = records + (size_t)pose * 8;
        const FitMeta mt = meta[pose];
        o->n_points = rec[0]; o->n_valid = rec[1]; o->n_zero_weight = 0; o->reserved = 0;
        o->c[0] = mt.c[0]; o->c[1] = mt.c[1]; o->c[2] = mt.c[2]; o->rho = mt.rho;
        o->sum_w = 2.0 * (double)rec[1];
    }
}

hipError_t launch_contour_fit(const int32_t *depth, const int4 *bbox, const uint32_t *box_off, uint32_t n_poses, uint32_t width, uint32_t height, int4 window,
                              const void *scene, bool scene_i32, const uint32_t *nearest, const FitMeta *meta, const FitParams &pm, uint32_t *records,
                              double *partial, pr_pose_info *info, hipStream_t s)
{
    const uint32_t nblk = fit_blocks(height);
    const hipError_t e = for_box_launches(depth, box_off, n_poses, width, height, scene, scene_i32, [&](const BoxLaunch &b, auto *sc) {
        hipLaunchKernelGGL(contour_fit_kernel, b.grid, dim3(256), 0, s, b.depth, bbox + b.p0, width, height, b.box_off, window, sc, nearest, meta + b.p0, pm,
                           records + (size_t)b.p0 * 8, partial + (size_t)b.p0 * nblk * kFitSums);
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fit_reduce_kernel, dim3((n_poses + 7) / 8), dim3(256), 0, s, partial, bbox, meta, records, nblk, height, n_poses, info);
    return hipGetLastError();
}

}  // namespace prk
