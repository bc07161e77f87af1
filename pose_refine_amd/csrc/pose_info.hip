// pose_info.hip -- pose observability (pr_pose_info / pr_pose_eig, include/pose_refine.h; no counterpart in the reference): the information pass,
// which forms the weighted point-to-plane normal matrix of every hypothesis in float64 about a caller-given centre, and the eigen kernel, which adds
// the workgroups' partial sums in block order and diagonalises the 6 x 6 by cyclic Jacobi.
// gfx950 (CDNA4, wave64); compiled with -ffp-contract=off: every per-point value is the one tests/info_ref.py forms with the same operations.
//
// Association and acceptance are the correspondence pass' own: gather_issue / gather_finish for the projective kinds, the winners of the kd-tree
// search kernels (query_nn<false> per lane for a tree without compact records), and the closest-point grid's two rules, restated below word for word
// because grid_scene.hip keeps them to itself.  r and w are the pass' float32 values (robust_weight).  Nothing is written to the cloud.  No atomics:
// a workgroup's sums go to memory and are added in block order, so two calls on the same inputs return the same bytes.
#include "pr_launch.h"
#include "icp_accumulate.h"
#include "pose_info.h"

namespace prk {

// the closest-point grid's definition (include/pose_refine.h states it; grid_scene.hip: grid_cell_of, grid_accept -- the same expressions)
__device__ __forceinline__ bool info_grid_cell_of(const SceneGridDev &s, float x, float y, float z, uint32_t &idx)
{
    const float fx = (x - s.origin[0]) * s.inv_cell, fy = (y - s.origin[1]) * s.inv_cell, fz = (z - s.origin[2]) * s.inv_cell;
    const bool inside = fx >= 0.0f && fx < (float)s.dim[0] && fy >= 0.0f && fy < (float)s.dim[1] && fz >= 0.0f && fz < (float)s.dim[2];
    idx = inside ? (uint32_t)(int)fx + s.dim[0] * ((uint32_t)(int)fy + s.dim[1] * (uint32_t)(int)fz) : 0u;
    return inside;
}
__device__ __forceinline__ bool info_grid_accept(const SceneGridDev &s, float sx, float sy, float sz, const float4 d)
{
    const float ex = d.x - sx, ey = d.y - sy, ez = d.z - sz;
    return (ex * ex + ey * ey + ez * ez) < s.max_dist_diff * s.max_dist_diff;
}

// ================================================================================================
//  the information pass
// ================================================================================================
// The lane's running sums: 30 float64 (H[21], g[6], sum_w, sum_wr2, sum_r2 -- pr_pose_info's order) and two exact counters.  Every index below is a
// compile-time constant after unrolling, so the 60 registers stay registers (no scratch).
struct InfoAcc { double v[kInfoSums]; uint32_t n_valid, n_zero; };

// One valid correspondence.  The operations, in this order and each rounded on its own, ARE the definition (include/pose_refine.h; tests/info_ref.py):
//   float32:  e = d - s;  r = (ex*nx + ey*ny) + ez*nz;  w = robust_weight(r)
//   float64:  q = s - c;  a = (qy*nz - qz*ny, qz*nx - qx*nz, qx*ny - qy*nx) / rho;  J = (a, n);  wJ[i] = w * J[i];  wr = w * r
//             H[i][j] += wJ[i] * J[j] (i <= j);  g[i] += wJ[i] * r;  sum_w += w;  sum_wr2 += wr * r;  sum_r2 += r * r
__device__ __forceinline__ void info_accumulate(InfoAcc &acc, float sx, float sy, float sz, const Corr &c, const RobustW &rb, double cx, double cy, double cz, double rho)
{
    const float ex = c.dx - sx, ey = c.dy - sy, ez = c.dz - sz;
    const float rf = ex * c.nx + ey * c.ny + ez * c.nz;
    const float wf = robust_weight(rf, rb);
    const double qx = (double)sx - cx, qy = (double)sy - cy, qz = (double)sz - cz;
    const double nx = (double)c.nx, ny = (double)c.ny, nz = (double)c.nz;
    double J[6];
    J[0] = (qy * nz - qz * ny) / rho;
    J[1] = (qz * nx - qx * nz) / rho;
    J[2] = (qx * ny - qy * nx) / rho;
    J[3] = nx; J[4] = ny; J[5] = nz;
    const double w = (double)wf, r = (double)rf;
    double wJ[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) wJ[i] = w * J[i];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) { acc.v[k] += wJ[i] * J[j]; ++k; }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc.v[21 + i] += wJ[i] * r;
    const double wr = w * r;
    acc.v[27] += w;
    acc.v[28] += wr * r;
    acc.v[29] += r * r;
    acc.n_valid += 1u;
    acc.n_zero += (wf == 0.0f) ? 1u : 0u;
}

enum { kInfoProj = 0, kInfoNN = 1, kInfoGrid = 2, kInfoWinners = 3 };

// grid = (blocks per hypothesis, hypotheses), 256 lanes.  Block b of a hypothesis takes points [b * kInfoPointsPerBlock, ...) of its cloud in steps of
// 1024; within a step lane t takes points t, t + 256, t + 512, t + 768 -- adjacent lanes hold adjacent cloud points, as in vb_accumulate, so the
// scene gathers of a wavefront land on neighbouring pixels.  A block past its hypothesis' cloud writes nothing (the eigen kernel does not read it).
template <class Scene, int kKind>
__global__ __launch_bounds__(256) void pose_info_pass_kernel(const pr_vec3 *__restrict__ cloud, const InfoMeta *__restrict__ meta, Scene scene, RobustW rb,
                                                             uint32_t nblk, double *__restrict__ partial)
{
    __shared__ double wsum[4][kInfoStride];
    const uint32_t pose = blockIdx.y, blk = blockIdx.x;
    const InfoMeta m = meta[pose];
    const uint32_t n = m.count, first = blk * kInfoPointsPerBlock;
    if (first >= n) return;                                      // (uniform over the workgroup: nobody reaches the barrier)
    const float *cl = reinterpret_cast<const float *>(cloud + m.start);
    const double cx = (double)m.c[0], cy = (double)m.c[1], cz = (double)m.c[2], rho = (double)m.rho;
    InfoAcc acc;
#pragma unroll
    for (int i = 0; i < (int)kInfoSums; ++i) acc.v[i] = 0.0;
    acc.n_valid = 0u; acc.n_zero = 0u;
    const uint32_t last = n - 1u;
    for (uint32_t s = 0; s < kInfoSteps; ++s) {
        const uint32_t j0 = first + s * kPointsPerStep + threadIdx.x;
        if (first + s * kPointsPerStep >= n) break;              // (uniform)
        float p[12];
        bool live[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t j = j0 + i * kBlockThreads;
            live[i] = j < n;
            const pr_vec3 v = ld_off<pr_vec3>(cl, (j < last ? j : last) * 12u);      // (a lane past the end re-reads the last point and never uses it)
            p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z;
        }
        if constexpr (kKind == kInfoProj) {
            Gathered gth[4];
            bool in_img[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) in_img[i] = gather_issue(scene, p[3 * i], p[3 * i + 1], p[3 * i + 2], live[i], gth[i]);
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                Corr c;
                if (gather_finish(scene, in_img[i], p[3 * i + 2], gth[i], c)) info_accumulate(acc, p[3 * i], p[3 * i + 1], p[3 * i + 2], c, rb, cx, cy, cz, rho);
            }
        } else if constexpr (kKind == kInfoGrid) {
            uint32_t w[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                uint32_t idx;
                const bool in_grid = info_grid_cell_of(scene, p[3 * i], p[3 * i + 1], p[3 * i + 2], idx) && live[i];
                w[i] = scene.cell_point[in_grid ? idx : 0u];
                if (!in_grid) w[i] = PR_GRID_NONE;
            }
            float4 d[4], nr[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const size_t at = (w[i] != PR_GRID_NONE) ? w[i] : 0u;      // (record 0 stands in for a lane without a winner)
                d[i] = scene.rec[2 * at]; nr[i] = scene.rec[2 * at + 1];
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                if (w[i] != PR_GRID_NONE && info_grid_accept(scene, p[3 * i], p[3 * i + 1], p[3 * i + 2], d[i])) {
                    Corr c; c.dx = d[i].x; c.dy = d[i].y; c.dz = d[i].z; c.nx = nr[i].x; c.ny = nr[i].y; c.nz = nr[i].z;
                    info_accumulate(acc, p[3 * i], p[3 * i + 1], p[3 * i + 2], c, rb, cx, cy, cz, rho);
                }
            }
        } else if constexpr (kKind == kInfoWinners) {
            // kd-tree scenes after the product's search kernels have run (launch_nn_search): four winners, then the four (point, normal) pairs, all in
            // flight before the first use -- the gathers of vb_accumulate's winners branch
            const uint32_t *win = scene.winner + m.start;
            uint32_t w[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) w[i] = live[i] ? win[j0 + i * kBlockThreads] : kNoPrev;
            float4 d[4]; float nx[4], ny[4], nz[4];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t at = (w[i] != kNoPrev) ? w[i] : 0u;
                d[i] = scene.pts[at];
                const float *nr = reinterpret_cast<const float *>(scene.normal + at);
                nx[i] = nr[0]; ny[i] = nr[1]; nz[i] = nr[2];
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                if (w[i] != kNoPrev) {
                    Corr c; c.dx = d[i].x; c.dy = d[i].y; c.dz = d[i].z; c.nx = nx[i]; c.ny = ny[i]; c.nz = nz[i];
                    info_accumulate(acc, p[3 * i], p[3 * i + 1], p[3 * i + 2], c, rb, cx, cy, cz, rho);
                }
            }
        } else {
            // kd-tree scenes without compact records (no search kernels for them): the reference's own stackless ordered walk per lane, as the audit
            // kernel runs it (contrib29_kernel) -- exact, and several times the cost of the search kernels (profiles/information/README.md)
#pragma unroll 1
            for (uint32_t i = 0; i < 4; ++i) {
                Corr c;
                if (live[i] && query_nn<false>(scene, nullptr, p[3 * i], p[3 * i + 1], p[3 * i + 2], c)) info_accumulate(acc, p[3 * i], p[3 * i + 1], p[3 * i + 2], c, rb, cx, cy, cz, rho);
            }
        }
    }
    // wavefront: pairwise over lanes (offsets 32 .. 1), the sum in lane 0; workgroup: ((w0 + w1) + w2) + w3
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < (int)kInfoSums; ++i) {
        double v = acc.v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
        acc.v[i] = v;
    }
    const uint32_t nv = wave_sum_u32(acc.n_valid), nz = wave_sum_u32(acc.n_zero);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < (int)kInfoSums; ++i) wsum[wave][i] = acc.v[i];
        uint32_t *cnt = reinterpret_cast<uint32_t *>(&wsum[wave][kInfoSums]);
        cnt[0] = nv; cnt[1] = nz;
    }
    __syncthreads();
    double *out = partial + ((size_t)pose * nblk + blk) * kInfoStride;
    if (threadIdx.x < kInfoSums) out[threadIdx.x] = ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
    else if (threadIdx.x == kInfoSums) {
        uint32_t tv = 0, tz = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const uint32_t *cnt = reinterpret_cast<const uint32_t *>(&wsum[w][kInfoSums]); tv += cnt[0]; tz += cnt[1]; }
        uint32_t *o = reinterpret_cast<uint32_t *>(out + kInfoSums);
        o[0] = tv; o[1] = tz;
    }
}

// ================================================================================================
//  the eigen kernel: partials -> pr_pose_info, cyclic Jacobi -> pr_pose_eig.  One lane per hypothesis.
// ================================================================================================
// Jacobi on the symmetric 6 x 6 A (full storage) with V = I at the start; all indices are compile-time constants (macros over literal p, q).
//   sweep:     the 15 rotations (p, q), p < q, in row-major order (0,1) (0,2) ... (4,5)
//   rotation:  skipped when A[p][q] == 0 exactly; else theta = (A[q][q] - A[p][p]) / (2 A[p][q]), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)),
//              c = 1 / sqrt(t^2 + 1), s = t c;  A[p][p] -= t A[p][q], A[q][q] += t A[p][q], A[p][q] = A[q][p] = 0, and for every other k
//              (A[k][p], A[k][q]) <- (c A[k][p] - s A[k][q], s A[k][p] + c A[k][q]) with their mirror images; the same update on columns p, q of V
//   stopping:  BEFORE every sweep: stop when max_{p<q} |A[p][q]| <= 2^-56 * max_p |A[p][p]| (so a zero or diagonal matrix takes no sweep)
//   sweep cap: kInfoMaxSweeps = 16; `sweeps` is the number of sweeps run
struct Sym6 { double a[6][6]; double v[6][6]; };

template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(Sym6 &m)
{
    const double apq = m.a[P][Q];
    if (apq == 0.0) return;
    const double theta = (m.a[Q][Q] - m.a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    m.a[P][P] -= t * apq;
    m.a[Q][Q] += t * apq;
    m.a[P][Q] = 0.0; m.a[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (k != P && k != Q) {
            const double akp = m.a[k][P], akq = m.a[k][Q];
            const double np = c * akp - s * akq, nq = s * akp + c * akq;
            m.a[k][P] = np; m.a[P][k] = np;
            m.a[k][Q] = nq; m.a[Q][k] = nq;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double vkp = m.v[k][P], vkq = m.v[k][Q];
        m.v[k][P] = c * vkp - s * vkq;
        m.v[k][Q] = s * vkp + c * vkq;
    }
}
// compare-exchange of eigenpairs I < J: ascending, strict (equal eigenvalues keep their places)
template <int I, int J>
__device__ __forceinline__ void eig_order(double (&lam)[6], Sym6 &m)
{
    const bool swap = lam[I] > lam[J];
    const double li = lam[I], lj = lam[J];
    lam[I] = swap ? lj : li; lam[J] = swap ? li : lj;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double vi = m.v[k][I], vj = m.v[k][J];
        m.v[k][I] = swap ? vj : vi; m.v[k][J] = swap ? vi : vj;
    }
}

__global__ __launch_bounds__(64) void pose_info_eigen_kernel(const double *__restrict__ partial, const InfoMeta *__restrict__ meta, uint32_t nblk, uint32_t n_poses,
                                                             pr_pose_info *__restrict__ info, pr_pose_eig *__restrict__ eig)
{
    const uint32_t pose = blockIdx.x * 64u + threadIdx.x;
    if (pose >= n_poses) return;
    const InfoMeta mt = meta[pose];
    const uint32_t used = (mt.count + kInfoPointsPerBlock - 1u) / kInfoPointsPerBlock;      // blocks that wrote a partial, added in block order
    double sum[kInfoSums];
#pragma unroll
    for (int i = 0; i < (int)kInfoSums; ++i) sum[i] = 0.0;
    uint32_t n_valid = 0, n_zero = 0;
    for (uint32_t b = 0; b < used; ++b) {
        const double *src = partial + ((size_t)pose * nblk + b) * kInfoStride;
#pragma unroll
        for (int i = 0; i < (int)kInfoSums; ++i) sum[i] += src[i];
        const uint32_t *cnt = reinterpret_cast<const uint32_t *>(src + kInfoSums);
        n_valid += cnt[0]; n_zero += cnt[1];
    }
    pr_pose_info o;
    o.n_points = mt.count; o.n_valid = n_valid; o.n_zero_weight = n_zero; o.reserved = 0;
    o.c[0] = mt.c[0]; o.c[1] = mt.c[1]; o.c[2] = mt.c[2]; o.rho = mt.rho;
#pragma unroll
    for (int i = 0; i < 21; ++i) o.H[i] = sum[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) o.g[i] = sum[21 + i];
    o.sum_w = sum[27]; o.sum_wr2 = sum[28]; o.sum_r2 = sum[29];
    info[pose] = o;
    if (!eig) return;

    Sym6 m;
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) { m.a[i][j] = sum[k]; m.a[j][i] = sum[k]; ++k; }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = 0; j < 6; ++j) m.v[i][j] = (i == j) ? 1.0 : 0.0;
        }
    }
    uint32_t sweeps = 0;
    for (; sweeps < kInfoMaxSweeps; ++sweeps) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            diag = fmax(diag, fabs(m.a[i][i]));
#pragma unroll
            for (int j = i + 1; j < 6; ++j) off = fmax(off, fabs(m.a[i][j]));
        }
        if (off <= 0x1p-56 * diag) break;
        jacobi_rotate<0, 1>(m); jacobi_rotate<0, 2>(m); jacobi_rotate<0, 3>(m); jacobi_rotate<0, 4>(m); jacobi_rotate<0, 5>(m);
        jacobi_rotate<1, 2>(m); jacobi_rotate<1, 3>(m); jacobi_rotate<1, 4>(m); jacobi_rotate<1, 5>(m);
        jacobi_rotate<2, 3>(m); jacobi_rotate<2, 4>(m); jacobi_rotate<2, 5>(m);
        jacobi_rotate<3, 4>(m); jacobi_rotate<3, 5>(m);
        jacobi_rotate<4, 5>(m);
    }
    double lam[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) lam[i] = m.a[i][i];
    // ascending order by a fixed 12-comparator network on six keys
    eig_order<1, 2>(lam, m); eig_order<4, 5>(lam, m);
    eig_order<0, 2>(lam, m); eig_order<3, 5>(lam, m);
    eig_order<0, 1>(lam, m); eig_order<3, 4>(lam, m); eig_order<2, 5>(lam, m);
    eig_order<0, 3>(lam, m); eig_order<1, 4>(lam, m);
    eig_order<2, 4>(lam, m); eig_order<1, 3>(lam, m);
    eig_order<2, 3>(lam, m);
    pr_pose_eig e;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        // the sign rule: the component of largest magnitude (lowest index on a tie) is positive
        double big = m.v[0][k];
#pragma unroll
        for (int i = 1; i < 6; ++i) if (fabs(m.v[i][k]) > fabs(big)) big = m.v[i][k];
        const double sg = (big < 0.0) ? -1.0 : 1.0;
        e.lambda[k] = lam[k];
#pragma unroll
        for (int i = 0; i < 6; ++i) e.V[i * 6 + k] = sg * m.v[i][k];
    }
    e.sweeps = sweeps; e.reserved = 0;
    eig[pose] = e;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
template <class Scene, int kKind>
static hipError_t launch_info_pass_t(const pr_vec3 *cloud, const InfoMeta *meta, const Scene &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s)
{
    if (n_poses == 0 || nblk == 0) return hipSuccess;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(pose_info_pass_kernel<Scene, kKind>), dim3(nblk, n_poses), dim3(kBlockThreads), 0, s, cloud, meta, sc, RobustW{ rb.kind, rb.c, rb.inv_c }, nblk, partial);
    return hipGetLastError();
}
hipError_t launch_info_pass_proj_aos(const pr_vec3 *cloud, const InfoMeta *meta, const SceneProjAoS &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s)
{ return launch_info_pass_t<SceneProjAoS, kInfoProj>(cloud, meta, sc, rb, nblk, n_poses, partial, s); }
hipError_t launch_info_pass_proj_packed(const pr_vec3 *cloud, const InfoMeta *meta, const SceneProjPacked &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s)
{ return launch_info_pass_t<SceneProjPacked, kInfoProj>(cloud, meta, sc, rb, nblk, n_poses, partial, s); }
hipError_t launch_info_pass_nn(const pr_vec3 *cloud, const InfoMeta *meta, const SceneNNDev &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s)
{ return launch_info_pass_t<SceneNNDev, kInfoNN>(cloud, meta, sc, rb, nblk, n_poses, partial, s); }
hipError_t launch_info_pass_nn_winners(const pr_vec3 *cloud, const InfoMeta *meta, const SceneNNWinners &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s)
{ return launch_info_pass_t<SceneNNWinners, kInfoWinners>(cloud, meta, sc, rb, nblk, n_poses, partial, s); }
hipError_t launch_info_pass_grid(const pr_vec3 *cloud, const InfoMeta *meta, const SceneGridDev &sc, const pr_robust &rb, uint32_t nblk, uint32_t n_poses, double *partial, hipStream_t s)
{ return launch_info_pass_t<SceneGridDev, kInfoGrid>(cloud, meta, sc, rb, nblk, n_poses, partial, s); }

hipError_t launch_info_eigen(const double *partial, const InfoMeta *meta, uint32_t nblk, uint32_t n_poses, pr_pose_info *info, pr_pose_eig *eig, hipStream_t s)
{
    if (n_poses == 0) return hipSuccess;
    hipLaunchKernelGGL(pose_info_eigen_kernel, dim3((n_poses + 63) / 64), dim3(64), 0, s, partial, meta, nblk, n_poses, info, eig);
    return hipGetLastError();
}

}  // namespace prk
