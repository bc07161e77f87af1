"""Plain reference of the closest-point grid scene (pr_scene_grid, include/pose_refine.h): numpy float32 in the header's order of operations, no
code shared with the library.

  describe(lo, hi, cell, ...)    the geometry pr_scene_grid_describe must return
  cell_of / centres              a point's cell, the cells' centres
  expected_cells                 per cell, brute force from its centre (nn_ref.BruteForce): the tie set the build may pick from, and whether the
                                 minimum is inside `reach`
  associate                      a cloud's winners and their validity against a built grid
  terms29 / transform            the 29 per-point terms of a correspondence (icp.h:138-206) and the pending update, in the pass' operand order
  canonical_sums                 the canonical tree (oracle: sum29_canonical) over per-point terms
  icp_loop                       the host-solve loop on top of them (solve_ref.pose_iteration)
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import nn_ref
import solve_ref

F32 = np.float32
NONE = 0xFFFFFFFF
MAX_CELLS = 1 << 26


def describe(lo, hi, cell, max_dist_diff, reach):
    """origin = lo, inv_cell = 1.0f / cell, dim[a] = floor((hi[a] - lo[a]) * inv_cell) + 1 (float32): hi itself lies inside the grid."""
    lo, hi = np.asarray(lo, F32).reshape(3), np.asarray(hi, F32).reshape(3)
    cell = F32(cell)
    inv = F32(F32(1.0) / cell)
    f = ((hi - lo).astype(F32) * inv).astype(F32)
    dim = (np.floor(f).astype(np.int64) + 1)
    return SimpleNamespace(origin=lo.copy(), cell=cell, inv_cell=inv, dim=tuple(int(d) for d in dim), max_dist_diff=F32(max_dist_diff), reach=F32(reach))


def from_ctypes(d):
    """The same record from a _lib.SceneGridDesc."""
    return SimpleNamespace(origin=np.array(list(d.origin), F32), cell=F32(d.cell), inv_cell=F32(d.inv_cell), dim=tuple(int(v) for v in d.dim),
                           max_dist_diff=F32(d.max_dist_diff), reach=F32(d.reach))


def cell_of(points, desc):
    """(inside, index): per axis f = (p - origin) * inv_cell, inside iff f >= 0 and f < dim (NaN and the infinities fail), i = (int)f,
    index = i0 + dim0 * (i1 + dim1 * i2); index is 0 where the point is outside."""
    p = np.asarray(points, F32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        f = ((p - desc.origin[None, :]).astype(F32) * desc.inv_cell).astype(F32)
        dim = np.array(desc.dim, F32)
        inside = ((f >= F32(0.0)) & (f < dim[None, :])).all(axis=1)
    i = np.where(inside[:, None], f, F32(0.0)).astype(np.int64)
    idx = i[:, 0] + desc.dim[0] * (i[:, 1] + desc.dim[1] * i[:, 2])
    return inside, np.where(inside, idx, 0)


def centres(desc):
    """(cells, 3) float32, x fastest: origin[a] + ((float)i[a] + 0.5f) * cell."""
    ax = [(desc.origin[a] + (np.arange(desc.dim[a], dtype=F32) + F32(0.5)) * desc.cell).astype(F32) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(F32))


def expected_cells(desc, pts):
    """nn_ref.BruteForce from every cell's centre with `reach` as its radius: .ties[c] = the scene points a build may store in cell c,
    .inside[c] = the cell holds one of them (d2 < reach * reach, float32) rather than NONE."""
    return nn_ref.BruteForce(centres(desc), pts, desc.reach)


def check_cells(cell_point, bf):
    """Every cell of a build against expected_cells: returns the list of cells that are wrong (empty: the build meets the definition)."""
    cp = np.asarray(cell_point, np.uint32).reshape(-1)
    assert len(cp) == len(bf.d2)
    bad = []
    for c in range(len(cp)):
        if bf.inside[c]:
            if int(cp[c]) not in bf.ties[c]:
                bad.append(c)
        elif cp[c] != NONE:
            bad.append(c)
    return bad


def transform(cloud, update):
    """The pending update on a cloud, float32, ((m0*x + m1*y) + m2*z) + m3 per row (the fused pass' operand order)."""
    M = np.asarray(update, F32).reshape(-1)[:12].reshape(3, 4)
    p = np.asarray(cloud, F32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        out = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]
    return np.ascontiguousarray(np.stack(out, 1).astype(F32))


def associate(cloud, desc, cell_point, rec):
    """(winner, valid): winner = the scene point of the cloud point's cell (NONE outside the grid and in a NONE cell), valid = it exists and
    ((ex*ex + ey*ey) + ez*ez) < max_dist_diff * max_dist_diff with e = d - p, float32."""
    p = np.asarray(cloud, F32).reshape(-1, 3)
    cp = np.asarray(cell_point, np.uint32).reshape(-1)
    rec = np.asarray(rec, F32).reshape(-1, 8)
    inside, idx = cell_of(p, desc)
    winner = np.where(inside, cp[idx], np.uint32(NONE)).astype(np.uint32)
    has = winner != NONE
    d = rec[np.where(has, winner, 0).astype(np.int64), 0:3]
    with np.errstate(invalid="ignore", over="ignore"):
        e = (d - p).astype(F32)
        e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        valid = has & (e2 < desc.max_dist_diff * desc.max_dist_diff)
    return winner, valid


_UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def terms29(cloud, winner, valid, rec):
    """(n, 29) float32: what each point adds to the 29 sums (icp.h:138-206, the operand order of the kernels' accumulate()); zero rows where
    there is no valid correspondence."""
    s = np.asarray(cloud, F32).reshape(-1, 3)
    rec = np.asarray(rec, F32).reshape(-1, 8)
    at = np.where(valid, winner, 0).astype(np.int64)
    d, n = rec[at, 0:3], rec[at, 4:7]
    out = np.zeros((len(s), 29), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (d - s).astype(F32)
        r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
        J = np.stack([n[:, 2] * s[:, 1] - n[:, 1] * s[:, 2], n[:, 0] * s[:, 2] - n[:, 2] * s[:, 0], n[:, 1] * s[:, 0] - n[:, 0] * s[:, 1],
                      n[:, 0], n[:, 1], n[:, 2]], 1).astype(F32)
        for k, (a, b) in enumerate(_UPPER):
            out[:, k] = J[:, a] * J[:, b]
        out[:, 21:27] = J * r[:, None]
        out[:, 27] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        out[:, 28] = F32(1.0)
        out = (out + F32(0.0)).astype(F32)                          # (the kernels add every term to a zero: -0 becomes +0)
    out[~np.asarray(valid, bool)] = F32(0.0)
    return out


def canonical_sums(terms, ppb):
    """The 29 sums of (n, 29) per-point terms in the canonical tree: workgroup g owns points [g * ppb, (g + 1) * ppb); lane t of its 256 adds,
    from 0, points g * ppb + s * 1024 + 256 * i + t in the order s, i; each wavefront of 64 lanes is reduced by a balanced pairwise tree in lane
    order; ((w0 + w1) + w2) + w3; the workgroup sums are added in workgroup order from 0.  All float32."""
    t = np.asarray(terms, F32).reshape(-1, 29)
    n = len(t)
    ppb = max(1024, int(ppb))
    groups = (n + ppb - 1) // ppb
    total = np.zeros(29, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(groups):
            blk = np.zeros((ppb, 29), F32)
            part = t[g * ppb:(g + 1) * ppb]
            blk[:len(part)] = part
            lanes = np.zeros((256, 29), F32)
            for row in blk.reshape(ppb // 256, 256, 29):           # rows in the order (s, i): point s * 1024 + i * 256 + t
                lanes = (lanes + row).astype(F32)
            w = lanes.reshape(4, 64, 29)
            while w.shape[1] > 1:
                w = (w[:, 0::2] + w[:, 1::2]).astype(F32)
            w = w[:, 0]
            total = (total + (((w[0] + w[1]) + w[2]) + w[3])).astype(F32)
    return total


def pass_sums(cloud, desc, cell_point, rec, ppb):
    """The 29 canonical-tree sums of one correspondence pass over `cloud` (already moved by whatever update was pending)."""
    w, v = associate(cloud, desc, cell_point, rec)
    return canonical_sums(terms29(cloud, w, v, rec), ppb), int(v.sum())


def icp_loop(cloud, desc, cell_point, rec, crit, ppb, trace=False):
    """The host-solve loop (icp.cu:156-217 as pr_icp.cpp runs it) on the grid: returns (T (16,), rmse, fitness, passes[, (passes, 29) sums])."""
    cl = np.ascontiguousarray(cloud, F32).reshape(-1, 3).copy()
    T = np.eye(4, dtype=F32).reshape(16)
    rmse = fitness = 0.0
    rows = []
    if len(cl) == 0:
        return (T, rmse, fitness, 0, np.zeros((0, 29), F32)) if trace else (T, rmse, fitness, 0)
    for it in range(int(crit[2]) + 1):
        sums, _ = pass_sums(cl, desc, cell_point, rec, ppb)
        rows.append(sums)
        T, rmse, fitness, E, _ = solve_ref.pose_iteration(sums, len(cl), T, rmse, fitness, crit, it)
        if E is None:
            break
        cl = transform(cl, E)
    out = (np.asarray(T, F32), rmse, fitness, len(rows))
    return out + (np.array(rows, F32),) if trace else out
