// jacobi.h -- the host's cyclic Jacobi eigen-solve of a symmetric N x N in doubles: pose_info_eigen_kernel's decomposition (pose_info.hip),
// statement for statement -- include/pose_refine.h specifies it for pr_info_eig (N = 6) and pr_plane_from_moments (N = 3).  Every result is
// held bit for bit: no operation may be reordered.
#pragma once
#include <cmath>
#include <cstdint>

// (one source for the host and for kernels that run the same solve per lane: cloud.h)
#if defined(__HIP__)
#define JACOBI_FN __host__ __device__ inline
#else
#define JACOBI_FN inline
#endif

namespace prr {

// one rotation that zeroes A[p][q]; V takes it along (its columns become the eigenvectors)
template <int N>
JACOBI_FN void jacobi_rotate(double (&A)[N][N], double (&V)[N][N], int p, int q)
{
    const double apq = A[p][q];
    if (apq == 0.0) return;
    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
    const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
    A[p][p] -= t * apq;
    A[q][q] += t * apq;
    A[p][q] = 0.0; A[q][p] = 0.0;
    for (int k = 0; k < N; ++k) {
        if (k == p || k == q) continue;
        const double akp = A[k][p], akq = A[k][q];
        const double np = c * akp - s * akq, nq = s * akp + c * akq;
        A[k][p] = np; A[p][k] = np;
        A[k][q] = nq; A[q][k] = nq;
    }
    for (int k = 0; k < N; ++k) {
        const double vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

// sweeps over all pairs p < q in row-major order until the largest off-diagonal is at most 2^-56 of the largest diagonal (tested before each
// sweep) or max_sweeps are done; returns the number of sweeps done
template <int N>
JACOBI_FN uint32_t jacobi_eigen(double (&A)[N][N], double (&V)[N][N], uint32_t max_sweeps)
{
    uint32_t sweeps = 0;
    for (; sweeps < max_sweeps; ++sweeps) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < N; ++i) {
            diag = std::fmax(diag, std::fabs(A[i][i]));
            for (int j = i + 1; j < N; ++j) off = std::fmax(off, std::fabs(A[i][j]));
        }
        if (off <= 0x1p-56 * diag) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) jacobi_rotate(A, V, p, q);
    }
    return sweeps;
}

}  // namespace prr
