"""CPU reference of pr_pose_distance and pr_cluster_greedy: the definition of include/pose_refine.h restated in numpy -- the candidates' matrices
in float64 (pr_mat4_mul's summation order), rounded once, then every listed float32 operation one by one (no contraction: numpy has none) --
and a float64 evaluation of the same distances to hold the definition itself against."""
import numpy as np

from pose_refine_amd import _lib

F = np.float32
SAT = 1 << 40


def _poses(p):
    return np.ascontiguousarray(p, np.float32).reshape(-1, 4, 4)


def as_rows64(A, S):
    """Rows 0..2 of A * S in float64, every entry summed as mat4_mul_impl does: 0 + a3 s3, + a2 s2, + a1 s1, + a0 s0."""
    A, S = A.astype(np.float64), S.astype(np.float64)
    out = np.zeros((3, 4), np.float64)
    for i in range(3):
        for j in range(4):
            acc = np.float64(0.0)
            for k in (3, 2, 1, 0):
                acc = acc + A[i, k] * S[k, j]
            out[i, j] = acc
    return out


def _apply(M, x, y, z):
    """((m0*x + m1*y) + m2*z) + m3 for the three rows of a float32 3x4, float32 throughout."""
    return [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)]


def candidate(points, A, B, S, K=None):
    """(sum_k, maxd_k, maxp_k) of one pair and one symmetry transform."""
    v = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    as64 = as_rows64(A, S)
    As = as64.astype(F)
    D = (as64 - B[:3].astype(np.float64)).astype(F)
    Bf = B[:3].astype(F)
    with np.errstate(all="ignore"):
        d = _apply(D, x, y, z)
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        q = np.rint(np.sqrt(d2) * F(65536.0))
        assert q.dtype == F and d2.dtype == F
        terms = np.where(q < F(SAT), q, F(0)).astype(np.uint64)
        terms[~(q < F(SAT))] = SAT
        total = int(terms.sum(dtype=np.uint64))
        maxd = F(np.fmax.reduce(d2, initial=F(0)))
        if K is None:
            return total, maxd, F(0)
        K = np.asarray(K, np.float32).reshape(9)
        a, b = _apply(As, x, y, z), _apply(Bf, x, y, z)
        behind = (a[2] <= F(0)) | (b[2] <= F(0))
        ua, wa = K[0] * a[0] / a[2] + K[2], K[4] * a[1] / a[2] + K[5]
        ub, wb = K[0] * b[0] / b[2] + K[2], K[4] * b[1] / b[2] + K[5]
        du, dw = ua - ub, wa - wb
        pp = np.where(behind, F(0), du * du + dw * dw)
        assert pp.dtype == F
        maxp = F(np.inf) if behind.any() else F(np.fmax.reduce(pp, initial=F(0)))
    return total, maxd, maxp


def record(points, A, B, syms=None, K=None, per_candidate=False):
    """One pr_pose_dist record (a POSE_DIST scalar array of shape ()); per_candidate: also the list of (sum, maxd, maxp) per k."""
    S = _poses(syms) if syms is not None and len(syms) else np.eye(4, dtype=np.float32)[None]
    cands = [candidate(points, A, B, S[k], K) for k in range(len(S))]
    out = np.zeros((), _lib.POSE_DIST)
    ks = min(range(len(S)), key=lambda k: (cands[k][0], k))
    kd = min(range(len(S)), key=lambda k: (cands[k][1], k))
    out["disp_sum_q16"], out["sym_sum"] = cands[ks][0], ks
    out["max_disp_sq"], out["sym_disp"] = cands[kd][1], kd
    if K is not None:
        kp = min(range(len(S)), key=lambda k: (cands[k][2], k))
        out["max_proj_sq"], out["sym_proj"] = cands[kp][2], kp
    out["n_points"] = len(np.asarray(points).reshape(-1, 3))
    return (out, cands) if per_candidate else out


def pairs(points, a, b, syms=None, K=None):
    a, b = _poses(a), _poses(b)
    if len(b) == 1 and len(a) != 1:
        b = np.repeat(b, len(a), 0)
    assert len(a) == len(b)
    return np.array([record(points, a[i], b[i], syms, K) for i in range(len(a))], _lib.POSE_DIST).reshape(len(a))


def matrix(points, a, b=None, syms=None, K=None):
    a = _poses(a)
    b = a if b is None else _poses(b)
    return np.array([[record(points, a[i], b[j], syms, K) for j in range(len(b))] for i in range(len(a))], _lib.POSE_DIST).reshape(len(a), len(b))


def truth64(points, A, B, S, K=None):
    """The same three figures of one candidate in float64 from the float32 inputs: (mean mm, max mm, max px or None), and the bound's
    magnitude term mean_v || |D| |(v, 1)| ||."""
    v = np.asarray(points, np.float64).reshape(-1, 3)
    vh = np.concatenate([v, np.ones((len(v), 1))], 1)
    As = A.astype(np.float64) @ S.astype(np.float64)
    Bd = B.astype(np.float64)
    D = (As - Bd)[:3]
    d = vh @ D.T
    n = np.sqrt((d * d).sum(1))
    mag = np.sqrt(((np.abs(vh) @ np.abs(D).T) ** 2).sum(1)).mean()
    px = None
    if K is not None:
        K = np.asarray(K, np.float64).reshape(9)
        pa, pb = vh @ As[:3].T, vh @ Bd[:3].T
        ua, wa = K[0] * pa[:, 0] / pa[:, 2] + K[2], K[4] * pa[:, 1] / pa[:, 2] + K[5]
        ub, wb = K[0] * pb[:, 0] / pb[:, 2] + K[2], K[4] * pb[:, 1] / pb[:, 2] + K[5]
        px = np.sqrt((ua - ub) ** 2 + (wa - wb) ** 2).max()
    return n.mean(), n.max(), px, mag


def cluster_greedy(order, dist, max_disp_mm):
    """pr_cluster_greedy's rule in Python: (kept, representative of every i of order; -1 elsewhere)."""
    d2 = np.asarray(dist)["max_disp_sq"]
    r2 = F(max_disp_mm) * F(max_disp_mm)
    kept, rep = [], np.full(len(d2), -1, np.int64)
    for i in (int(i) for i in order):
        hit = next((j for j in kept if d2[i, j] <= r2 or d2[j, i] <= r2), None)
        if hit is None:
            kept.append(i)
        rep[i] = i if hit is None else hit
    return kept, rep
