"""Plain reference of the robust ICP pass (pr_robust, include/pose_refine.h): numpy float32 in the header's order of operations, no code shared
with the library.

  weight(r, robust)                         the weight of a float32 residual, every operation rounded on its own
  weighted_terms29(cloud, corr, robust)     the 29 per-point terms with the header's factor table (WEIGHTED_FACTOR) applied to columns 0..26
  plain_terms29(cloud, corr)                grid_ref.terms29's arithmetic on given correspondences
  loop(cloud, associate, robust, crit, ppb) the host-solve loop on top of them (grid_ref.transform, grid_ref.canonical_sums, solve_ref.pose_iteration)

A `robust` is anything with .kind, .c and .inv_c (api.Robust, or describe() below, which restates pr_robust_describe); a `corr` is (d, n, valid):
the scene point and normal of every cloud point's correspondence and whether it is a valid one.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import grid_ref
import solve_ref

F32 = np.float32
NONE, HUBER, TUKEY, CAUCHY = 0, 1, 2, 3

# THE FACTOR TABLE of include/pose_refine.h, one entry per weighted sum: which of the product's two factors has been multiplied by w first.
#   sums 0..20   J[a] * J[b], a <= b, row-major: 0 = J[a] (the lower index), 1 = J[b]
#   sums 21..26  J[a] * r, a = 0..5:             0 = J[a],                   1 = r
WEIGHTED_FACTOR = (0,) * 21 + (0, 0, 0, 1, 1, 1)
assert len(WEIGHTED_FACTOR) == 27

_UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def describe(kind, c):
    """pr_robust_describe's record: inv_c = 1.0f / c, once, in float32 (0 for NONE)."""
    c = F32(c)
    if kind == NONE:
        return SimpleNamespace(kind=NONE, c=F32(0.0), inv_c=F32(0.0))
    return SimpleNamespace(kind=int(kind), c=c, inv_c=F32(F32(1.0) / c))


def weight(r, robust):
    """float32 weights of float32 residuals.  HUBER: a = |r|; a <= c ? 1 : c / a.  TUKEY: u = r * inv_c; q = u * u; q < 1 ? (1 - q) * (1 - q) : 0.
    CAUCHY: 1 / (1 + q).  NONE: 1."""
    r = np.asarray(r, F32)
    one = F32(1.0)
    kind, c, inv_c = int(robust.kind), F32(robust.c), F32(robust.inv_c)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        if kind == NONE:
            return np.ones(r.shape, F32)
        if kind == HUBER:
            a = np.abs(r)
            return np.where(a <= c, one, (c / a).astype(F32)).astype(F32)
        u = (r * inv_c).astype(F32)
        q = (u * u).astype(F32)
        if kind == TUKEY:
            t = (one - q).astype(F32)
            return np.where(q < one, (t * t).astype(F32), F32(0.0)).astype(F32)
        if kind == CAUCHY:
            return (one / (one + q).astype(F32)).astype(F32)
    raise ValueError(f"unknown kind {kind}")


def _geometry(cloud, corr):
    s = np.asarray(cloud, F32).reshape(-1, 3)
    d, n, valid = corr
    d, n, valid = np.asarray(d, F32).reshape(-1, 3), np.asarray(n, F32).reshape(-1, 3), np.asarray(valid, bool).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (d - s).astype(F32)
        r = ((e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]).astype(F32)
        J = np.stack([n[:, 2] * s[:, 1] - n[:, 1] * s[:, 2], n[:, 0] * s[:, 2] - n[:, 2] * s[:, 0], n[:, 1] * s[:, 0] - n[:, 0] * s[:, 1],
                      n[:, 0], n[:, 1], n[:, 2]], 1).astype(F32)
        e2 = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(F32)
    return J, r, e2, valid


def residuals(cloud, corr):
    """The float32 residual of every point, r = (ex*nx + ey*ny) + ez*nz (meaningful where the correspondence is valid)."""
    return _geometry(cloud, corr)[1]


def weighted_terms29(cloud, corr, robust):
    """(n, 29) float32: columns 0..26 weighted through WEIGHTED_FACTOR (seven weighted values per point: w*J[0..5] and w*r), 27 and 28 plain; zero
    rows where there is no valid correspondence.  Also returns the weights (0 where invalid)."""
    J, r, e2, valid = _geometry(cloud, corr)
    w = weight(r, robust)
    out = np.zeros((len(J), 29), F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        wJ = (w[:, None] * J).astype(F32)
        wr = (w * r).astype(F32)
        for k, (a, b) in enumerate(_UPPER):
            out[:, k] = wJ[:, a] * J[:, b] if WEIGHTED_FACTOR[k] == 0 else J[:, a] * wJ[:, b]
        for a in range(6):
            out[:, 21 + a] = wJ[:, a] * r if WEIGHTED_FACTOR[21 + a] == 0 else J[:, a] * wr
        out[:, 27] = e2
        out[:, 28] = F32(1.0)
        out = (out + F32(0.0)).astype(F32)                          # (the kernels add every term to a zero: -0 becomes +0)
    out[~valid] = F32(0.0)
    return out, np.where(valid, w, F32(0.0)).astype(F32)


def plain_terms29(cloud, corr):
    """grid_ref.terms29 on given correspondences (its arithmetic, through a record array made of them)."""
    d, n, valid = corr
    m = len(np.asarray(valid).reshape(-1))
    rec = np.zeros((max(m, 1), 8), F32)
    rec[:m, 0:3] = np.asarray(d, F32).reshape(-1, 3)
    rec[:m, 4:7] = np.asarray(n, F32).reshape(-1, 3)
    return grid_ref.terms29(cloud, np.arange(m, dtype=np.uint32), np.asarray(valid, bool).reshape(-1), rec)


def grid_associate(desc, cell_point, rec):
    """associate(cloud) for a closest-point grid: all numpy (grid_ref.associate)."""
    rec = np.asarray(rec, F32).reshape(-1, 8)

    def associate(cloud):
        winner, valid = grid_ref.associate(cloud, desc, cell_point, rec)
        at = np.where(valid, winner, 0).astype(np.int64)
        return rec[at, 0:3], rec[at, 4:7], valid
    return associate


def loop(cloud, associate, robust, crit, ppb):
    """The host-solve loop (icp.cu:156-217 as pr_icp.cpp runs it) with weighted sums: returns (T (16,), rmse, fitness, (passes, 29) sums).
    associate(cloud) -> (d, n, valid) for the cloud as it stands (already moved by every update so far)."""
    cl = np.ascontiguousarray(cloud, F32).reshape(-1, 3).copy()
    T = np.eye(4, dtype=F32).reshape(16)
    rmse = fitness = 0.0
    rows = []
    if len(cl) == 0:
        return T, rmse, fitness, np.zeros((0, 29), F32)
    for it in range(int(crit[2]) + 1):
        terms, _ = weighted_terms29(cl, associate(cl), robust)
        sums = grid_ref.canonical_sums(terms, ppb)
        rows.append(sums)
        T, rmse, fitness, E, _ = solve_ref.pose_iteration(sums, len(cl), T, rmse, fitness, crit, it)
        if E is None:
            break
        cl = grid_ref.transform(cl, E)
    return np.asarray(T, F32), rmse, fitness, np.array(rows, F32)
