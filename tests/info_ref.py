"""Plain float64 reference of the information pass (pr_pose_info / pr_pose_eig, include/pose_refine.h): numpy in the header's order of operations,
no code shared with the library.

  terms(cloud, corr, robust, c, rho)    the 30 per-point terms (H[21], g[6], w, w r^2, r^2), one row per VALID correspondence, and the weights
  sums(terms)                           each column by math.fsum (the correctly rounded sum) and the sum of the absolute terms beside it
  record(cloud, corr, robust, c, rho)   everything a pr_pose_info holds: counts, fsums, abs sums
  sym6(h21) / eigh(h21)                 the symmetric 6 x 6 and numpy.linalg.eigh of it
  covariance(...)                       pr_info_covariance's definition
  analytic clouds                       plane / sphere / cylinder with exact normals and the null spaces they must show

A `corr` is (d, n, valid) as in robust_ref; r and w are robust_ref's float32 values (the pass' own), everything after them is float64 with every
operation rounded on its own -- numpy evaluates elementwise IEEE operations without contraction, so each term equals the kernel's bit for bit and
only the order of the additions differs.
"""
from __future__ import annotations

import math

import numpy as np

import robust_ref as R

F32, F64 = np.float32, np.float64
N_SUMS = 30
_UPPER = [(a, b) for a in range(6) for b in range(a, 6)]
PLAIN = R.describe(R.NONE, 0.0)


def terms(cloud, corr, robust, c, rho):
    """((n_valid, 30) float64 terms, float32 weights of the valid rows, float32 residuals of the valid rows)."""
    s32 = np.asarray(cloud, F32).reshape(-1, 3)
    d, n, valid = corr
    valid = np.asarray(valid, bool).reshape(-1)
    r32 = R.residuals(s32, corr)[valid]
    w32 = R.weight(r32, robust if robust is not None else PLAIN)
    s = s32[valid].astype(F64)
    nn = np.asarray(n, F32).reshape(-1, 3)[valid].astype(F64)
    cc = np.asarray(c, F32).astype(F64)
    rho = F64(F32(rho))
    q = s - cc
    J = np.empty((len(s), 6), F64)
    J[:, 0] = (q[:, 1] * nn[:, 2] - q[:, 2] * nn[:, 1]) / rho
    J[:, 1] = (q[:, 2] * nn[:, 0] - q[:, 0] * nn[:, 2]) / rho
    J[:, 2] = (q[:, 0] * nn[:, 1] - q[:, 1] * nn[:, 0]) / rho
    J[:, 3:] = nn
    w, r = w32.astype(F64), r32.astype(F64)
    wJ = w[:, None] * J
    out = np.empty((len(s), N_SUMS), F64)
    for k, (a, b) in enumerate(_UPPER):
        out[:, k] = wJ[:, a] * J[:, b]
    for a in range(6):
        out[:, 21 + a] = wJ[:, a] * r
    out[:, 27] = w
    out[:, 28] = (w * r) * r
    out[:, 29] = r * r
    return out, w32, r32


def sums(t):
    """(fsum of every column, fsum of its absolute values): two (30,) float64 arrays."""
    t = np.asarray(t, F64).reshape(-1, N_SUMS)
    return (np.array([math.fsum(t[:, k]) for k in range(N_SUMS)], F64), np.array([math.fsum(np.abs(t[:, k])) for k in range(N_SUMS)], F64))


def record(cloud, corr, robust, c, rho):
    t, w, _ = terms(cloud, corr, robust, c, rho)
    total, absum = sums(t)
    return dict(n_points=len(np.asarray(cloud).reshape(-1, 3)), n_valid=len(t), n_zero_weight=int((w == F32(0.0)).sum()), sums=total, abs=absum)


def flat_sums(info):
    """The 30 sums of one POSE_INFO record in the reference's column order."""
    return np.concatenate([np.asarray(info["H"], F64).reshape(21), np.asarray(info["g"], F64).reshape(6),
                           [F64(info["sum_w"]), F64(info["sum_wr2"]), F64(info["sum_r2"])]])


def sum_bound(n_valid, absum):
    """|device sum - fsum| <= (n_valid + 16) * 2^-52 * sum |term|: the terms are the reference's own, each of the at most n_valid + 16 additions of
    the device's tree (lane, wavefront, workgroup, blocks) rounds once by at most 2^-53 relative to a partial sum that the absolute sum bounds;
    doubled for margin."""
    return (n_valid + 16) * 2.0 ** -52 * np.asarray(absum, F64)


def sym6(h21):
    m = np.zeros((6, 6), F64)
    m[np.triu_indices(6)] = np.asarray(h21, F64).reshape(21)
    return m + np.triu(m, 1).T


def eigh(h21):
    return np.linalg.eigh(sym6(h21))


def rank_of(lam, min_ratio):
    lam = np.asarray(lam, F64)
    return int(((lam > 0.0) & (lam > min_ratio * lam[5])).sum())


def covariance(lam, V, sigma2, min_ratio):
    """sigma2 * sum over the counted k of v_k v_k^T / lambda[k] (6 x 6), and the rank."""
    lam, V = np.asarray(lam, F64), np.asarray(V, F64).reshape(6, 6)
    keep = (lam > 0.0) & (lam > min_ratio * lam[5])
    cov = np.zeros((6, 6), F64)
    for k in np.flatnonzero(keep):
        cov += np.outer(V[:, k], V[:, k]) / lam[k]
    return sigma2 * cov, int(keep.sum())


def residual_sigma2(sum_wr2, sum_w, n_valid):
    return (sum_wr2 / sum_w) * n_valid / (n_valid - 6)


def projector(V, cols):
    V = np.asarray(V, F64).reshape(6, 6)[:, list(cols)]
    return V @ V.T


# ---- analytic surfaces: points, exact unit normals, and the null space of their information matrix about `c` -----------------------------------
def _span_projector(vectors):
    q, _ = np.linalg.qr(np.asarray(vectors, F64).T)
    return q @ q.T


def plane_cloud(n, z=0.8, half=0.1, seed=1):
    """A frontal plane z = const: normal (0, 0, -1).  Null space about any centre ON the plane: rotation about z, translation along x and y."""
    g = np.random.default_rng(seed)
    p = np.column_stack([g.uniform(-half, half, n), g.uniform(-half, half, n), np.full(n, z)])
    nr = np.tile([0.0, 0.0, -1.0], (n, 1))
    return p, nr, _span_projector(np.eye(6)[[2, 3, 4]])


def sphere_cloud(n, center=(0.02, -0.01, 0.8), radius=0.05, seed=2):
    """The camera-facing half of a sphere.  About its centre with rho = its radius: the three rotations are null."""
    g = np.random.default_rng(seed)
    v = g.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v[:, 2] = -np.abs(v[:, 2])
    return np.asarray(center) + radius * v, v, _span_projector(np.eye(6)[[0, 1, 2]])


def cylinder_cloud(n, center=(0.0, 0.0, 0.8), radius=0.04, half=0.06, seed=3):
    """The side of a cylinder with its axis along y through `center`: rotation about the axis and translation along it are null."""
    g = np.random.default_rng(seed)
    th = g.uniform(np.pi, 2 * np.pi, n)                              # the half facing the camera (z below the axis)
    nr = np.column_stack([np.cos(th), np.zeros(n), np.sin(th)])
    p = np.asarray(center) + radius * nr + np.column_stack([np.zeros(n), g.uniform(-half, half, n), np.zeros(n)])
    return p, nr, _span_projector(np.eye(6)[[1, 4]])


def null_bound(max_abs_s, rho, sum_w):
    """Upper bound on the null eigenvalues once points, normals and centre are rounded to float32 -- (4 * 2^-24 * max|s| / rho)^2 * sum_w; derived in
    tests/test_information_host.py."""
    return (4.0 * 2.0 ** -24 * max_abs_s / rho) ** 2 * sum_w
