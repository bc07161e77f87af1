"""Support planes, restated in numpy from the text of include/pose_refine.h alone (no code shared with the library): float32 operation by
operation in the stated order, int64 moments, Python integers for the scatter matrix, Python floats (IEEE double) for the Jacobi refit."""
import math

import numpy as np

F = np.float32
MAX_SAMPLES, MAX_CANDIDATES, MAX_SWEEPS, BEHIND, NO_DEPTH = 65536, 4096, 16, 254, 255


class Invalid(Exception):
    """what the library answers with PR_ERR_INVALID"""


def dot(ax, ay, az, bx, by, bz):
    return F(F(F(ax * bx) + F(ay * by)) + F(az * bz)) if np.ndim(ax) == 0 and np.ndim(bx) == 0 else ((ax * bx + ay * by) + az * bz).astype(F)


def has_normal(nrm):
    return (nrm[..., 0] != 0) | (nrm[..., 1] != 0) | (nrm[..., 2] != 0)


def sample(pcd, nrm, width, height, stride):
    """(points mm float32[n, 3], normals float32[n, 3], pixel index int64[n]) in row-major order"""
    pcd, nrm = pcd.reshape(height, width, 3), nrm.reshape(height, width, 3)
    ys, xs = np.meshgrid(np.arange(0, height, stride), np.arange(0, width, stride), indexing="ij")
    p, m = pcd[ys, xs], nrm[ys, xs]
    keep = has_normal(m) & (p[..., 2] > 0) & ((p[..., 2] * F(1000.0)).astype(F) <= F(65535.0))
    return (p[keep] * F(1000.0)).astype(F), m[keep].astype(F), (ys * width + xs)[keep].astype(np.int64)


def normal_test(cos_min, nx, ny, nz, m):
    if F(cos_min) == F(-2.0):
        return np.ones(len(m), bool)
    return dot(F(nx), F(ny), F(nz), m[:, 0], m[:, 1], m[:, 2]) >= F(cos_min)


def inliers(pts, nrm, alive, c, tau_mm, cos_min):
    """the alive samples that support the plane of sample c"""
    pc, nc = pts[c], nrm[c]
    d = (pts - pc).astype(F)
    r = dot(nc[0], nc[1], nc[2], d[:, 0], d[:, 1], d[:, 2])
    return alive & (np.abs(r) <= F(tau_mm)) & normal_test(cos_min, nc[0], nc[1], nc[2], nrm)


def moments_of(pts):
    q = np.rint(pts.astype(np.float64) * 16.0).astype(np.int64)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.array([len(q), x.sum(), y.sum(), z.sum(), (x * x).sum(), (x * y).sum(), (x * z).sum(), (y * y).sum(), (y * z).sum(), (z * z).sum()], np.int64)


def _rotate(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    A[p][p] -= t * apq
    A[q][q] += t * apq
    A[p][q] = A[q][p] = 0.0
    k = 3 - p - q
    akp, akq = A[k][p], A[k][q]
    A[k][p] = A[p][k] = c * akp - s * akq
    A[k][q] = A[q][k] = s * akp + c * akq
    for r in range(3):
        vp, vq = V[r][p], V[r][q]
        V[r][p] = c * vp - s * vq
        V[r][q] = s * vp + c * vq


def scatter(m):
    """the exact scatter matrix n S_ab - S_a S_b as Python integers"""
    m = [int(v) for v in m]
    n, S = m[0], m[1:4]
    SS = [[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]]
    return [[n * SS[i][j] - S[i] * S[j] for j in range(3)] for i in range(3)]


def from_moments(m):
    """(normal [3 floats], offset_mm, rms_mm, eig [plane's, the other two in index order]) in double, or Invalid"""
    m = [int(v) for v in m]
    if m[0] < 3:
        raise Invalid("fewer than 3 points")
    Ci = scatter(m)
    if not any(Ci[i][j] for i in range(3) for j in range(3)):
        raise Invalid("all-zero scatter matrix")
    A = [[float(Ci[i][j]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(MAX_SWEEPS):
        off = max(abs(A[0][1]), abs(A[0][2]), abs(A[1][2]))
        diag = max(abs(A[0][0]), abs(A[1][1]), abs(A[2][2]))
        if off <= 2.0 ** -56 * diag:
            break
        _rotate(A, V, 0, 1)
        _rotate(A, V, 0, 2)
        _rotate(A, V, 1, 2)
    lo = 0
    for i in (1, 2):
        if A[i][i] < A[lo][lo]:
            lo = i
    v = [V[0][lo], V[1][lo], V[2][lo]]
    ln = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    if not (ln > 0.0) or not math.isfinite(ln):
        raise Invalid("no length")
    nu = [v[0] / ln, v[1] / ln, v[2] / ln]
    offset = ((nu[0] * float(m[1]) + nu[1] * float(m[2])) + nu[2] * float(m[3])) / float(m[0]) / 16.0
    first = nu[0] if nu[0] != 0.0 else (nu[1] if nu[1] != 0.0 else nu[2])
    if offset > 0.0 or (offset == 0.0 and first > 0.0):
        nu, offset = [-nu[0], -nu[1], -nu[2]], -offset
    rms = math.sqrt(max(A[lo][lo], 0.0)) / float(m[0]) / 16.0
    others = [i for i in range(3) if i != lo]
    return nu, offset, rms, [A[lo][lo], A[others[0]][others[0]], A[others[1]][others[1]]]


def scene_planes(pcd, nrm, depth, width, height, stride=4, cand_stride=16, tau_mm=3.0, label_tau_mm=6.0, cos_min=0.9, min_support=500, n_planes=1,
                 drop_behind=True):
    """dict(planes=[dict(normal f32[3], offset_mm f32, candidate, support, labelled, behind, rms_mm f32)], labels uint8[h, w], depth like the input,
    moments int64[n_found, 10], supports uint32[n_planes, MAX_CANDIDATES], n_samples, n_candidates)"""
    pcd, nrm = np.ascontiguousarray(pcd, F).reshape(-1, 3), np.ascontiguousarray(nrm, F).reshape(-1, 3)
    pts, nm, pix = sample(pcd, nrm, width, height, stride)
    n = len(pts)
    if n > MAX_SAMPLES:
        raise Invalid("samples")
    n_cand = (n - 1) // cand_stride + 1 if n else 0
    if n_cand > MAX_CANDIDATES:
        raise Invalid("candidates")
    labels = np.where(pcd[:, 2] > 0, 0, NO_DEPTH).astype(np.uint8)
    supports = np.zeros((n_planes, MAX_CANDIDATES), np.uint32)
    planes, moments = [], []
    pmm = (pcd * F(1000.0)).astype(F)
    with_normal = has_normal(nrm)
    for k in range(1, n_planes + 1):
        if n == 0:
            break
        alive = labels[pix] == 0
        best, best_c = 0, -1
        for c in range(n_cand):
            if not alive[c * cand_stride]:
                continue
            s = int(inliers(pts, nm, alive, c * cand_stride, tau_mm, cos_min).sum())
            supports[k - 1, c] = s
            if s > best:
                best, best_c = s, c
        if best == 0 or best < min_support:
            break
        m = moments_of(pts[inliers(pts, nm, alive, best_c * cand_stride, tau_mm, cos_min)])
        try:
            nu, offset, rms, _ = from_moments(m)
        except Invalid:
            break
        nu32, off32 = np.array(nu, np.float64).astype(F), F(offset)
        h = (dot(nu32[0], nu32[1], nu32[2], pmm[:, 0], pmm[:, 1], pmm[:, 2]) - off32).astype(F)
        free = labels == 0
        on = free & (np.abs(h) <= F(label_tau_mm)) & (~with_normal | normal_test(cos_min, nu32[0], nu32[1], nu32[2], nrm))
        behind = free & ~on & (h < -F(label_tau_mm)) if (k == 1 and drop_behind) else np.zeros(len(labels), bool)
        labels[on] = k
        labels[behind] = BEHIND
        planes.append(dict(normal=nu32, offset_mm=off32, candidate=best_c, support=best, labelled=int(on.sum()), behind=int(behind.sum()), rms_mm=F(rms)))
        moments.append(m)
    depth = np.asarray(depth)
    cleared = np.where(labels.reshape(depth.shape) == 0, depth, 0).astype(depth.dtype)
    return dict(planes=planes, labels=labels.reshape(height, width), depth=cleared, moments=np.array(moments, np.int64).reshape(-1, 10), supports=supports,
                n_samples=n, n_candidates=n_cand)
